"""-m gpu: the multigrid-preconditioned PCG of the periodic cell problems (``preconditioner="multigrid"``, vfem_hom_mg_*) against
tests/homogenization_mg_cpu.py, the scipy restatement (P by Kronecker products, A_l by sparse triple products, SuperLU at the
coarsest level), piece by piece and as a whole.

Cells (homogenization_mg_cpu.CELLS; random densities in [0.05, 1], gamma = 3, E_min = 1e-3):
    8x4x12    two levels, the coarse level 4x2x6 has coinciding wrapped neighbours
    12x8x16   three levels, coarsest 3x2x4, anisotropic tensor, voxels 1.0 x 0.8 x 1.3
    16x12     2-D, three levels, odd coarsest 4x3, anisotropic tensor, voxels 1.0 x 0.7
    5x3x7     no coarsening: the preconditioner is the exact inverse

Bounds, all relative to the largest entry.  Operators, sweeps: 1e-12, the bound of the existing apply test; transfers 1e-13.
V-cycle: ten times the difference the restatement itself shows between a SuperLU and an explicit numpy.linalg.inv coarsest solve,
measured on the CPU on these cells at 2.9e-15 (12x8x16), 6.9e-16 (16x12), 1.9e-15 (8x4x12), 3.8e-15 (5x3x7) -- so the floor 1e-12
holds.  Solve: ten times the restatement's own multigrid-PCG-versus-direct difference at tol = 1e-10, measured on the CPU:
    12x8x16   w 4.20e-10   Eh 9.76e-13   (20 .. 21 iterations; block Jacobi 205 .. 210)
    16x12     w 4.15e-10   Eh 1.75e-11   (30 .. 31 iterations; block Jacobi 194 .. 195)
Grid independence (spherical void of radius 0.3, isotropic E = 1, nu = 0.3, gamma = 1): the restatement takes 12 12 12 14 15 15
iterations at 16^3 and 14 14 14 16 17 18 at 32^3 (block Jacobi 129 .. 133 at 32^3); reproduce with
``python tests/homogenization_mg_cpu.py 16 16 16`` and ``.. 32 32 32`` (no GPU needed)."""
import functools

import numpy as np
import pytest
import torch

import homogenization_cpu as hc
import homogenization_mg_cpu as mg
import material_ref as mr

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor                           # noqa: E402
from ndr_amd import homogenization as hom                      # noqa: E402
from ndr_amd import pyVoxelFEM as pv                           # noqa: E402

TOL_OPERATOR = 1e-12
TOL_TRANSFER = 1e-13
TOL_VCYCLE = max(10 * 3.8e-15, 1e-12)
TOL_W = {"12x8x16": 10 * 4.20e-10, "16x12": 10 * 4.15e-10}
TOL_EH = {"12x8x16": 10 * 9.76e-13, "16x12": 10 * 1.75e-11}
SOLVER_TOL = 1e-10
VOID_ITERATIONS = {16: [12, 12, 12, 14, 15, 15], 32: [14, 14, 14, 16, 17, 18]}
COARSENABLE = ["8x4x12", "12x8x16", "16x12"]


def _tensor(kind):
    if kind == "aniso3":
        return ElasticityTensor(mr.ANISO_3D, dim=3)
    if kind == "aniso2":
        return ElasticityTensor(mr.ANISO_2D, dim=2)
    return ElasticityTensor(1.0, 0.3, dim=3)


def _sim(ne, dom, tensor, rho, gamma=3.0, Emin=1e-3):
    t = pv.TensorProductSimulator([1] * len(ne), [np.zeros(len(ne)), np.array(dom, dtype=np.float64)], list(ne))
    t.ETensor = tensor
    t.E_0, t.E_min, t.gamma = 1.0, Emin, gamma
    t.setElementDensities(np.asarray(rho, dtype=np.float64).reshape(-1))
    return t


def _make(name):
    ne, h, kind, _ = mg.CELLS[name]
    return _sim(ne, [n * v for n, v in zip(ne, h)], _tensor(kind), mg.cell_density(name))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the restatement's direct solution and hierarchy of one cell, computed once and shared (tests leave them unchanged)"""
    ref = mg.cell_reference(name)
    return ref, mg.Hierarchy(mg.CELLS[name][0], ref["K0"], ref["E"])


@functools.lru_cache(maxsize=None)
def _reference_pcg(name):
    ref, H = _reference(name)
    return mg.pcg_columns(H, ref["b"], SOLVER_TOL)


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random(H, l, seed):
    S = 3 if H.N == 2 else 6
    return np.random.default_rng(seed).standard_normal((S, H.K[l].shape[0]))


def _hierarchy(name, levels=None):
    return hom._Hierarchy(hom._Cell(_make(name)), levels)


@pytest.mark.parametrize("name", COARSENABLE)
def test_level_operators_match_the_galerkin_products(name):
    _, H = _reference(name)
    h = _hierarchy(name)
    assert h.dims == H.dims and h.bytes > 0
    for l in range(len(H.dims)):
        W = _random(H, l, 10 + l)
        out = h.level_apply(l, _dev(W).reshape(W.shape[0], -1, H.N)).cpu().numpy().reshape(W.shape)
        expect = np.stack([H.K[l] @ w for w in W])
        err = _relmax(out, expect)
        print("level apply %s level %d %s: %.2e" % (name, l, H.dims[l], err))
        assert err < TOL_OPERATOR
        assert np.array_equal(out[:, :H.N], W[:, :H.N])                              # the pin row is the identity
    h.close()


@pytest.mark.parametrize("name", COARSENABLE)
def test_transfers_match_the_interpolation(name):
    _, H = _reference(name)
    h = _hierarchy(name)
    for l in range(len(H.dims) - 1):
        F, C = _random(H, l, 20 + l), _random(H, l + 1, 30 + l)
        shape_f, shape_c = (F.shape[0], -1, H.N), (C.shape[0], -1, H.N)
        r = h.restrict(l, _dev(F).reshape(shape_f)).cpu().numpy().reshape(C.shape)
        err_r = _relmax(r, np.stack([H.R[l] @ f for f in F]))
        assert np.all(r[:, :H.N] == 0.0)                                             # zero at node 0
        p = h.prolong_add(l, _dev(C).reshape(shape_c), _dev(F).reshape(shape_f)).cpu().numpy().reshape(F.shape)
        err_p = _relmax(p, np.stack([f + H.P[l] @ c for f, c in zip(F, C)]))
        assert np.array_equal(p[:, :H.N], F[:, :H.N])                                # the coarse value of node 0 counts as zero
        print("transfers %s level %d: restrict %.2e, prolong %.2e" % (name, l, err_r, err_p))
        assert err_r < TOL_TRANSFER and err_p < TOL_TRANSFER
    h.close()


@pytest.mark.parametrize("name", COARSENABLE)
def test_colour_sweeps_match_the_restatement(name):
    """one forward and one backward sweep on every smoothed level from a random X and B; level 0 is the matrix-free one"""
    _, H = _reference(name)
    h = _hierarchy(name)
    for l in range(len(H.dims) - 1):
        X, B = _random(H, l, 40 + l), _random(H, l, 50 + l)
        shape = (X.shape[0], -1, H.N)
        x, b = _dev(X).reshape(shape).clone(), _dev(B).reshape(shape)
        expect = np.stack([v.copy() for v in X])
        for forward in (True, False):
            h.smooth(l, x, b, forward)
            for q in range(len(expect)):
                H.sweep(l, expect[q], B[q], forward)
            err = _relmax(x.cpu().numpy().reshape(X.shape), expect)
            print("sweep %s level %d %s: %.2e" % (name, l, "forward" if forward else "backward", err))
            assert err < TOL_OPERATOR
    h.close()


@pytest.mark.parametrize("name", COARSENABLE)
@pytest.mark.parametrize("smoothing", [1, 2])
def test_vcycle_matches_the_restatement_and_is_symmetric(name, smoothing):
    _, H = _reference(name)
    h = _hierarchy(name)
    B = _random(H, 0, 60)
    B[:, :H.N] = 0.0
    Z = h.vcycle(_dev(B).reshape(B.shape[0], -1, H.N), smoothing).cpu().numpy().reshape(B.shape)
    expect = np.stack([H.vcycle(b.copy(), smoothing) for b in B])
    err = _relmax(Z, expect)
    sym = abs(B[0] @ Z[1] - B[1] @ Z[0]) / max(abs(B[0] @ Z[1]), abs(B[1] @ Z[0]))
    print("V-cycle %s, %d sweeps: %.2e, symmetry %.2e" % (name, smoothing, err, sym))
    assert err < TOL_VCYCLE
    assert sym < 1e-12
    assert np.all(Z[:, :H.N] == 0.0)
    h.close()


@pytest.mark.parametrize("name", ["12x8x16", "16x12"])
def test_multigrid_solve_matches_direct_solve(name):
    ne = mg.CELLS[name][0]
    ref, H = _reference(name)
    _, its_cpu = _reference_pcg(name)
    sim = _make(name)
    w = hom.solveCellProblems(sim, tol=SOLVER_TOL, preconditioner="multigrid")
    S, N = len(w), len(ne)
    print("iterations %s: device %s, restatement %s, levels %s" % (name, hom.last_iterations, its_cpu, hom.last_levels))
    assert hom.last_levels == H.dims
    assert len(hom.last_iterations) == S and all(abs(g - c) <= 2 for g, c in zip(hom.last_iterations, its_cpu))
    assert all(r <= SOLVER_TOL for r in hom.last_relative_residuals)
    err_w = _relmax(np.stack(w), hc.to_full(ne, ref["W"]))
    Eh = hom.homogenizedElasticityTensor(w, sim)
    err_e = _relmax(Eh.D, ref["Eh"])
    G = hom.homogenizedElasticityTensorGradient(w, sim)
    err_id = _relmax(np.einsum("e,eqr->qr", ref["E"] / ref["dE"], G), Eh.D)
    print("%s: w %.2e, Eh %.2e, energy identity %.2e" % (name, err_w, err_e, err_id))
    assert err_w < TOL_W[name]
    assert err_e < TOL_EH[name]
    assert err_id < TOL_EH[name]


def _void_sim(n):
    return _sim((n, n, n), (1.0, 1.0, 1.0), ElasticityTensor(1.0, 0.3, dim=3), mg.void_density((n, n, n)), gamma=1.0)


def test_grid_independence():
    """spherical void at 16^3 and 32^3: the counts of the restatement, and at 32^3 at most a quarter of block Jacobi's"""
    counts = {}
    for n in (16, 32):
        hom.solveCellProblems_device(_void_sim(n), tol=SOLVER_TOL, preconditioner="multigrid")
        counts[n] = list(hom.last_iterations)
        print("void %d^3: multigrid %s (restatement %s), levels %s" % (n, counts[n], VOID_ITERATIONS[n], hom.last_levels))
    hom.solveCellProblems_device(_void_sim(32), tol=SOLVER_TOL)
    jacobi = list(hom.last_iterations)
    print("void 32^3: block Jacobi %s" % jacobi)
    for n in (16, 32):
        assert all(abs(g - c) <= 2 for g, c in zip(counts[n], VOID_ITERATIONS[n]))
    assert 4 * max(counts[32]) <= min(jacobi)


def test_two_multigrid_solves_are_bit_identical():
    W1 = hom.solveCellProblems_device(_make("12x8x16"), preconditioner="multigrid")
    its = list(hom.last_iterations)
    W2 = hom.solveCellProblems_device(_make("12x8x16"), preconditioner="multigrid")
    assert torch.equal(W1, W2) and its == hom.last_iterations


def test_default_is_the_block_jacobi_path():
    W1 = hom.solveCellProblems_device(_make("12x8x16"))
    its = list(hom.last_iterations)
    W2 = hom.solveCellProblems_device(_make("12x8x16"), preconditioner="jacobi")
    assert torch.equal(W1, W2) and its == hom.last_iterations
    assert min(its) > 100                                        # block Jacobi takes 205 .. 210 on this cell, multigrid 20 .. 21


def test_one_level_hierarchy_is_the_exact_inverse():
    ne = mg.CELLS["5x3x7"][0]
    ref, _ = _reference("5x3x7")
    w = hom.solveCellProblems(_make("5x3x7"), tol=SOLVER_TOL, preconditioner="multigrid")
    assert hom.last_levels == [[5, 3, 7]]
    assert hom.last_iterations == [1] * 6
    err = _relmax(np.stack(w), hc.to_full(ne, ref["W"]))
    print("5x3x7: w %.2e" % err)
    assert err < TOL_VCYCLE


def test_errors_and_the_simulator_is_left_alone():
    sim = _make("8x4x12")
    with pytest.raises(ValueError, match="preconditioner"):
        hom.solveCellProblems(sim, preconditioner="ilu")
    big = _sim((151, 151), (1.0, 1.0), ElasticityTensor(1.0, 0.3, dim=2), np.ones((151, 151)))
    with pytest.raises(RuntimeError, match=r"151x151.*limit of 40000"):
        hom.solveCellProblems(big, preconditioner="multigrid")
    with pytest.raises(ValueError, match="levels"):
        hom.solveCellProblems(sim, preconditioner="multigrid", levels=-1)
    hom.solveCellProblems(sim, preconditioner="multigrid", levels=0)
    assert hom.last_levels == [[8, 4, 12]] and hom.last_iterations == [1] * 6
    hom.solveCellProblems(sim, preconditioner="multigrid", levels=5)
    assert hom.last_levels == [[8, 4, 12], [4, 2, 6]]

    clamp = np.zeros((sim.numNodes(), 3), dtype=bool)
    clamp[:65] = True
    sim.dirichletMask = clamp
    loads = np.random.default_rng(4).standard_normal((sim.numNodes(), 3))
    sim.setLoads_device(loads)
    rho = sim.getDensities()
    u = np.random.default_rng(2).standard_normal((sim.numNodes(), 3))
    Ku = sim.applyK(u)
    with pytest.raises(RuntimeError, match=r"no convergence in 2 iterations.*\|r\|/\|b\| = "):
        hom.solveCellProblems(sim, maxIter=2, preconditioner="multigrid")
    assert hom.last_iterations == [2] * 6
    w = hom.solveCellProblems(sim, preconditioner="multigrid", smoothing=2)
    assert max(hom.last_iterations) < 18                          # two sweeps: fewer iterations than one (17 .. 18)
    assert np.array_equal(sim.dirichletMask, clamp)
    assert np.array_equal(sim.buildLoadVector(), loads)
    assert np.array_equal(rho, sim.getDensities()) and np.array_equal(Ku, sim.applyK(u))
    assert np.abs(np.stack(w)[:, 0]).max() == 0.0                # pinned, Dirichlet conditions ignored
