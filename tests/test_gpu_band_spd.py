"""-m gpu: the direct solve of TensorProductSimulator (band_spd.hip: band assembly, band Cholesky on 64 x 64 tiles, substitution;
the reference factorises with CHOLMOD, TPS.hh:834-865) -- standalone factor and solve through the C ABI against numpy, the
simulators' solve against the oracle's sparse LU, the kept factorisation, and the reference's 2-D bridge log without multigrid."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from helpers import BC_BRIDGE, BC_CANTILEVER, GOLDEN, MATERIAL, ROOT, make_hip, make_oracle, seeded_density

pytestmark = pytest.mark.gpu
BC2D_MBB = os.path.join(ROOT, "bcs", "2d", "mbb_beam.bc")
BC2D_BRIDGE = os.path.join(ROOT, "bcs", "2d", "bridge.bc")


def _lib():
    from ndr_amd import _lib as L
    L.require_gpu()
    return L.load()


def _check(status):
    if status != 0:
        raise RuntimeError(_lib().vfem_last_error().decode())


def _factor(A, w):
    from ndr_amd import band
    d = torch.from_numpy(band.band_pack(A, w)).cuda()
    _check(_lib().vfem_band_spd_factor(A.shape[0], w, ctypes.c_void_p(d.data_ptr()), None))
    return d


def _solve(d, n, w, B):
    x = torch.from_numpy(np.ascontiguousarray(B.T)).cuda()                 # [nrhs][n]
    _check(_lib().vfem_band_spd_solve(n, w, ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(x.data_ptr()), B.shape[1], None))
    return x.cpu().numpy().T


def _band_spd(n, w, seed):
    """random symmetric band matrix, diagonally dominant"""
    A = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, n))
    A = A + A.T
    A[np.abs(np.subtract.outer(np.arange(n), np.arange(n))) > w] = 0.0
    A[np.diag_indices(n)] = np.abs(A).sum(axis=1) + 1.0
    return A


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


CASES = sorted({(n, w) for n in (1, 63, 64, 65, 1000, 4097) for w in (0, 1, 63, 64, 65, 200, n - 1) if w <= n - 1})


@pytest.mark.parametrize("n,w", CASES)
def test_band_factor_and_solve_match_numpy(n, w):
    from ndr_amd import band
    A = _band_spd(n, w, n + 7 * w)
    d = _factor(A, w)
    L, Lr = band.band_unpack(d.cpu().numpy(), n, w), np.linalg.cholesky(A)
    assert np.abs(L - Lr).max() <= 1e-13 * np.abs(Lr).max()
    rng = np.random.default_rng(w)
    for nrhs in (1, 3):
        B = rng.standard_normal((n, nrhs))
        assert _rel(_solve(d, n, w, B), np.linalg.solve(A, B)) <= 1e-12


def test_band_factor_is_reproducible_and_names_the_failing_pivot():
    n, w = 1000, 130
    A = _band_spd(n, w, 5)
    d1, d2 = _factor(A, w), _factor(A, w)
    assert torch.equal(d1.view(torch.int64), d2.view(torch.int64))
    B = np.random.default_rng(0).standard_normal((n, 2))
    assert np.array_equal(_solve(d1, n, w, B), _solve(d1, n, w, B))
    A[700, 700] = -1.0
    with pytest.raises(RuntimeError, match=r"not positive definite \(pivot 701 of 1000\)"):
        _factor(A, w)


def _residual(t, u, f):
    r = t.applyK(u) - f
    r[t.dirichletMask] = 0.0
    return float(np.linalg.norm(r) / np.linalg.norm(f))


def _oracle_oc(ne, dom, bc, v0, steps):
    """the CPU oracle's OC loop as fem.ground_truth_topopt drives it: compliance history and the oracle simulator afterwards"""
    from oracle import vfem_oracle as vo
    sim = vo.OracleSim(dom, ne)
    sim.read_material(MATERIAL)
    sim.set_uniform_densities(v0)
    sim.apply_bc_file(bc)
    sim.E0, sim.Emin, sim.gamma = 1.0, 1e-4, 3.0
    top = vo.OracleProblem(sim, vo.OracleComplianceObjective(sim), [vo.OracleVolumeConstraint(v0)],
                           [vo.OracleSmoothingFilter(), vo.OracleProjectionFilter()])
    oc = vo.OracleOC(top)
    top.set_vars(sim.rho.copy())
    hist = []
    for _ in range(steps):
        hist.append(2.0 * top.evaluate_objective())
        oc.step()
    return sim, hist


def _sim2d(ne, dom, bc):
    from ndr_amd import pyVoxelFEM as pv
    t = pv.TensorProductSimulator([1, 1], dom, ne)
    t.readMaterial(MATERIAL)
    t.applyDisplacementsAndLoadsFromFile(bc)
    t.E_0, t.E_min, t.gamma = 1.0, 1e-4, 3.0
    return t


def test_2d_bridge_solve_after_five_oc_steps_matches_the_oracle():
    ne, dom = [250, 125], ([0, 0], [2, 1])
    sim, _ = _oracle_oc(ne, dom, BC2D_BRIDGE, 0.4, 5)
    t = _sim2d(ne, dom, BC2D_BRIDGE)
    t.setElementDensities(sim.rho)
    f = t.buildLoadVector()
    u = t.solve(f)
    assert t.numDirectFactorizations() == 1
    assert _rel(u, sim.solve(f)) <= 1e-10
    assert _residual(t, u, f) <= 5e-11


@pytest.mark.parametrize("N,ne,dom,bc", [(2, (15, 7), ([0, 0], [3, 1]), BC2D_MBB), (3, (5, 3, 3), ([0, 0, 0], [2, 1, 1]), BC_CANTILEVER)])
def test_degree2_solve_matches_the_oracle(N, ne, dom, bc):
    from ndr_amd import pyVoxelFEM as pv
    from oracle import generic_oracle as go
    t = pv.TensorProductSimulator([2] * N, dom, ne)
    t.readMaterial(MATERIAL)
    t.applyDisplacementsAndLoadsFromFile(bc)
    t.E_min = 1e-4
    o = go.GenericSim(N, 2, dom, ne, 1.0, 0.3)
    o.Emin = 1e-4
    o.apply_bc_file(bc)
    # densities in [0.3, 1]: K's condition number stays near 1e6, where two exact solvers agree well inside 1e-10 (at [0.05, 1]
    # the 2-D K reaches 3e7, and LAPACK's dense Cholesky and SuperLU already differ by 4e-11)
    o.rho = np.random.default_rng(3).uniform(0.3, 1.0, o.num_elems)
    t.setElementDensities(o.rho)
    f = t.buildLoadVector()
    u = t.solve(f)
    assert _rel(u, o.solve(f)) <= 1e-10
    assert _residual(t, u, f) <= 5e-11


def test_3d_odd_grid_that_the_standin_refused_matches_the_oracle():
    """45 x 21 x 21: no multigrid hierarchy, and the stand-in's dense coarsest level refused its 66 792 dofs"""
    ne, dom = (45, 21, 21), ([0, 0, 0], [2, 1, 1])
    rho = np.random.default_rng(11).uniform(0.3, 1.0, int(np.prod(ne)))      # K's condition number as in the degree-2 cases
    t, o = make_hip(ne, dom, BC_BRIDGE, rho), make_oracle(ne, dom, BC_BRIDGE, rho)
    f = o.build_load_vector()
    u = t.solve(f)
    assert _rel(u, o.solve(f)) <= 1e-10
    assert _residual(t, u, f) <= 5e-11


def test_forced_standin_agrees_with_the_factorisation_on_2d_300x100():
    t = _sim2d([300, 100], ([0, 0], [3, 1]), BC2D_MBB)
    t.setUniformDensities(0.3)
    f = t.buildLoadVector()
    assert t.directSolver == "auto" and t.directBandBytes() <= 8 << 30
    u = t.solve(f)
    assert t.numDirectFactorizations() == 1
    t.directSolver = "pcg"
    assert _rel(t.solve(f), u) <= 1e-9
    assert t.numDirectFactorizations() == 1
    t.directSolver = "cholesky"
    assert np.array_equal(t.solve(f), u)
    t.directSolver = "lu"
    with pytest.raises(RuntimeError, match="directSolver"):
        t.solve(f)


@pytest.mark.parametrize("dim", [3, 2])
def test_factorisation_is_kept_until_the_operator_changes(dim):
    if dim == 3:
        ne, dom = (16, 8, 8), ([0, 0, 0], [2, 1, 1])
        rho = seeded_density(ne, 9)
        t, o = make_hip(ne, dom, BC_CANTILEVER, rho), make_oracle(ne, dom, BC_CANTILEVER, rho)
    else:
        ne, dom = [40, 20], ([0, 0], [2, 1])
        rho = seeded_density(ne, 9)
        t, o = _sim2d(ne, dom, BC2D_MBB), make_oracle(ne, dom, BC2D_MBB, rho)
        t.setElementDensities(rho)
    f = t.buildLoadVector()
    u1 = t.solve(f)
    assert t.numDirectFactorizations() == 1 and _rel(u1, o.solve(f)) <= 1e-10
    assert np.array_equal(t.solve(f), u1) and t.numDirectFactorizations() == 1
    t.setElementDensity(3, 0.25)
    o.rho[3] = 0.25
    o._lu = None
    assert _rel(t.solve(f), o.solve(f)) <= 1e-10 and t.numDirectFactorizations() == 2
    mask = t.dirichletMask
    last = np.arange(o.num_nodes).reshape(tuple(int(n) + 1 for n in ne))[-1].reshape(-1)
    mask[last, 0] = True
    t.dirichletMask = mask
    o.dmask[last, 0] = 1
    o._lu = None
    assert _rel(t.solve(f), o.solve(f)) <= 1e-10 and t.numDirectFactorizations() == 3


def test_2d_bridge_reference_log_without_multigrid():
    from ndr_amd import fem
    k = json.load(open(os.path.join(GOLDEN, "reference_logs.json")))["2d_bridge_250x125"]
    ne, dom = [250, 125], [[0, 0], [2, 1]]
    _, _, _, hist = fem.ground_truth_topopt(MATERIAL, BC2D_BRIDGE, [1, 1], dom, ne, 3, 0.4, "OC", 0, use_multigrid=False,
                                            max_iter=3, obj_history=True, verbose=False)
    assert len(hist) == 3
    for a, b in zip(hist, k["compliance"]):
        assert abs(a - b) <= 1e-7 * b, (hist, k["compliance"])
    _, _, _, hist5 = fem.ground_truth_topopt(MATERIAL, BC2D_BRIDGE, [1, 1], dom, ne, 3, 0.4, "OC", 0, use_multigrid=False,
                                             max_iter=5, obj_history=True, verbose=False)
    _, ref = _oracle_oc(ne, dom, BC2D_BRIDGE, 0.4, 5)
    for a, b in zip(hist5, ref):
        assert abs(a - b) <= 1e-8 * b, (hist5, ref)
