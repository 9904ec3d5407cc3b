"""-m gpu: the cell-problem kernels (vfem_hom_*, vfem_hom_mg_*) where they run in several 256-thread workgroups, their two-stage
reductions with more than 256 (512) partials, the batched PCG with columns that finish far apart, and its breakdown error.  The
references are the pieces of tests/homogenization_cpu.py and tests/homogenization_mg_cpu.py (no direct solve on the large cells).

Cells (homogenization_mg_cpu.block_cell; random densities in [0.05, 1], gamma = 3, E_min = 1e-3 unless said otherwise):
    2d-blocks     72 x 64, levels 36x32, 18x16, 9x8: 18 workgroups of nodes, stored levels of 1152 and 288 nodes (ragged last workgroup),
                  a stored sweep of 288 threads, an odd coarsest level
    3d-blocks     28 x 24 x 28, levels 14x12x14, 7x6x7: a level-0 sweep of 2352 threads per colour, a stored level of 2352 nodes, a stored
                  sweep of 294 threads, the dense coarsest matrix from stored blocks on 294 nodes, a gemv with n = 882
    2d-partials   320 x 256, seven levels down to 5x4: 320 partials per reduction (the stride loop of sum_partials, 64 in its tail)
    tensor-2d/3d  520 x 260 / 52^3: 529 / 550 workgroups of elements, so the tensor's grid is capped at 512, its grid-stride loop makes a
                  ragged second pass and 512 partials are summed
    lam-2d        48 x 6, rho = 1 / 0.1 split at x = 24, isotropic (1, 0.3), gamma = 1, E_min = 0, h = 1/48
    lam-3d        64 x 4 x 4, rho = 1 / 0.5 split at x = 32, same material, h = 1/64; its case yz has a right-hand side of rounding noise
                  only (|b| = 8.9e-20 in the restatement)
    uniform       6x4x8 and 8x6 with rho = 0.7: every right-hand side is zero or rounding noise (max|b| 8.3e-17 / 2.8e-17)
    void-2d       12 x 12, isotropic, gamma = 1, E_min = 0, rho = 1 except a 4 x 4 block of zeros: nine nodes without any stiffness

Bounds, all relative to the largest entry; every figure below was measured with the restatement on the CPU.
  Operators, sweeps 1e-12, transfers 1e-13, apply 1e-12, gradient 1e-10: the bounds of the two existing files, imported.
  V-cycle: SuperLU against an explicit inverse at the coarsest level gives 6.6e-15 / 6.7e-15 (2d-blocks, 1 / 2 sweeps) and
    4.9e-15 / 5.0e-15 (3d-blocks); ten times that is below 1e-12, so TOL_VCYCLE (1e-12) holds on both cells.
  Tensor: hc.tensor against its element sum taken in numpy.longdouble: 3.7e-16 (tensor-2d), 2.0e-16 (tensor-3d); bound 1e-12.
  Eight iterations on 2d-partials: the restatement's 8 iterations against themselves with the dot products accumulated in
    numpy.longdouble: W 7.6e-16 (block Jacobi), 1.8e-14 (multigrid), |r|/|b| 4.4e-16 / 4.0e-15; bound 1e-12.  |r|/|b| after 8
    iterations: 7.2e-2, 6.5e-2, 7.8e-2 (block Jacobi), 1.06e-3, 1.05e-3, 1.81e-3 (multigrid).
  Full multigrid solve of 2d-partials at tol = 1e-10: the restatement takes 42, 42, 44 iterations and ends with true residuals
    6.68e-11, 7.24e-11, 5.91e-11, which differ from its recurrence residuals by 2.5e-18, 4.2e-18, 1.1e-17 (absolute); the bound on
    that gap is ten times the largest, 1.12e-16.
  Laminates at tol = 1e-10, block Jacobi: lam-2d takes 59, 59, 76 iterations, lam-3d 57, 57, 57, (87), 86, 86; the restatement's
    PCG-versus-direct difference per real column is at most 8.18e-12 (lam-2d) and 2.65e-12 (lam-3d), the bound ten times that.

Measured on an MI355X:
  level apply 3.9e-16 .. 1.8e-15 (2d-blocks), 6.1e-16 .. 2.4e-15 (3d-blocks); apply 2.9e-16 / 6.3e-16; transfers at most 3.5e-16;
  sweeps 2.7e-16 .. 2.1e-15; V-cycle 5.5e-13 (2d-blocks), 3.5e-13 (3d-blocks) with 1 and 2 sweeps alike, symmetry at most 2.2e-15.
  (The V-cycle figures are the simulator's K0 against the restatement's, see test_eight_iterations_equal_eight_iterations.)
  tensor 3.5e-16 / 2.5e-16; gradient 5.4e-16 / 1.1e-15.
  eight iterations: block Jacobi w 1.9e-15, |r|/|b| 1.6e-15, twice bit-identical; multigrid w 7.5e-14, |r|/|b| 5.7e-15 (with the
    simulator's own K0: 2.5e-12 and 3.4e-13).
  full solve of 2d-partials: 42, 42, 44 iterations, true residuals 6.68e-11, 7.24e-11, 5.91e-11, gap to the reported ones 1.06e-17.
  lam-2d: 59, 59, 76 iterations, w 8.0e-14 .. 3.2e-13; lam-3d: 57, 57, 57, (0), 86, 86, w 1.7e-13 .. 7.3e-13, the noise case has
    b = 0 exactly and w = 0; closed form 1.4e-14.
  uniform: max|w| 1.5e-14 (6x4x8: 63 .. 65 block-Jacobi iterations on the noise, 16 with multigrid), 1.3e-15 (8x6: 37 .. 38 / 12).
  void-2d: breakdown in strain case 0 after 0 iterations with both preconditioners, |r|/|b| = 1 reported; NaN modulus: NaN reported.
  Against the library of the parent commit the three breakdown tests fail: no error is raised and the status is 0."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import homogenization_cpu as hc
import homogenization_mg_cpu as mg
import material_ref as mr

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor, _lib                      # noqa: E402
from ndr_amd import homogenization as hom                      # noqa: E402
from ndr_amd import pyVoxelFEM as pv                           # noqa: E402
from test_gpu_homogenization import TOL_APPLY, TOL_EH, TOL_GRADIENT                       # noqa: E402
from test_gpu_homogenization_mg import TOL_OPERATOR, TOL_TRANSFER, TOL_VCYCLE, _dev, _relmax, _sim   # noqa: E402

SOLVER_TOL = 1e-10
BLOCKS = ["2d-blocks", "3d-blocks"]
TOL_VCYCLE_BLOCKS = {"2d-blocks": max(10 * 6.7e-15, TOL_VCYCLE), "3d-blocks": max(10 * 5.0e-15, TOL_VCYCLE)}
TOL_TENSOR = {"tensor-2d": max(10 * 3.7e-16, 1e-12), "tensor-3d": max(10 * 2.0e-16, 1e-12)}
TOL_EIGHT = {"jacobi": max(10 * 7.6e-16, 1e-12), "multigrid": max(10 * 1.8e-14, 1e-12)}
PARTIALS_ITERATIONS = [42, 42, 44]
PARTIALS_GAP = 10 * 1.12e-17
LAMINATE_ITERATIONS = {"lam-2d": [59, 59, 76], "lam-3d": [57, 57, 57, 87, 86, 86]}
LAMINATE_NOISE = {"lam-2d": [], "lam-3d": [3]}                   # strain cases whose right-hand side is rounding noise
TOL_LAMINATE = {"lam-2d": 10 * 8.18e-12, "lam-3d": 10 * 2.65e-12}


def _tensor(name):
    for table in (mg.BLOCK_CELLS, mg.UNIFORM_CELLS):
        if name in table:
            return ElasticityTensor(mr.ANISO_3D, dim=3) if table[name][2] == "aniso3" else ElasticityTensor(mr.ANISO_2D, dim=2)
    return ElasticityTensor(1.0, 0.3, dim=len(mg.block_cell(name)[0]))


def _make(name):
    ne, h, _, rho, gamma, Emin = mg.block_cell(name)
    return _sim(ne, [n * v for n, v in zip(ne, h)], _tensor(name), rho, gamma, Emin)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """the restatement's matrix, right-hand sides and element constants of one cell, computed once and shared (tests leave them unchanged)"""
    return mg.block_problem(name)


@functools.lru_cache(maxsize=None)
def _hierarchy_cpu(name):
    pr = _problem(name)
    return mg.Hierarchy(pr["ne"], pr["K0"], pr["E"])


def _random(H, l, seed):
    return np.random.default_rng(seed).standard_normal((3 if H.N == 2 else 6, H.K[l].shape[0]))


def _hierarchy(name):
    return hom._Hierarchy(hom._Cell(_make(name)))


def _true_residuals(pr, W):
    return np.array([np.linalg.norm(b - pr["K"] @ w) / np.linalg.norm(b) for b, w in zip(pr["b"], W)])


def _periodic(ne, w):
    """[S, numNodes, N] on the full node grid -> [S, nd] on the periodic one"""
    w = np.asarray(w).reshape([len(w)] + [n + 1 for n in ne] + [len(ne)])
    for d, n in enumerate(ne):
        w = np.take(w, np.arange(n), axis=d + 1)
    return w.reshape(len(w), -1)


# ---- operators, transfers, sweeps and the V-cycle across workgroups ----

@pytest.mark.parametrize("name", BLOCKS)
def test_level_operators_match_the_galerkin_products(name):
    pr, H = _problem(name), _hierarchy_cpu(name)
    assert H.dims == mg.level_dims(pr["ne"])
    h = _hierarchy(name)
    c = h.cell
    assert h.dims == H.dims and h.bytes > 0
    assert _relmax(c.K0, pr["K0"]) < 1e-13 and _relmax(c.L, pr["L"]) < 1e-13 and _relmax(c.E.cpu().numpy(), pr["E"]) < 1e-15
    for l in range(len(H.dims)):
        W = _random(H, l, 10 + l)
        out = h.level_apply(l, _dev(W).reshape(W.shape[0], -1, H.N)).cpu().numpy().reshape(W.shape)
        err = _relmax(out, np.stack([H.K[l] @ w for w in W]))
        print("level apply %s level %d %s: %.2e" % (name, l, H.dims[l], err))
        assert err < TOL_OPERATOR
        assert np.array_equal(out[:, :H.N], W[:, :H.N])                              # the pin row is the identity
    # the handle-free apply against the assembled matrix
    W = _random(H, 0, 7)
    Win = _dev(W)
    Wout = torch.full_like(Win, float("nan"))
    _lib.check(_lib.load().vfem_hom_apply(*c.head(), pv._ptr(Win), pv._ptr(Wout), pv._stream()))
    err = _relmax(Wout.cpu().numpy(), np.stack([pr["K"] @ w for w in W]))
    print("apply %s: %.2e" % (name, err))
    assert err < TOL_APPLY
    assert np.array_equal(Wout.cpu().numpy()[:, :c.N], W[:, :c.N])
    h.close()


@pytest.mark.parametrize("name", BLOCKS)
def test_transfers_match_the_interpolation(name):
    H = _hierarchy_cpu(name)
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


@pytest.mark.parametrize("name", BLOCKS)
def test_colour_sweeps_match_the_restatement(name):
    """one forward and one backward sweep on every smoothed level from a random X and B; level 0 is the matrix-free one"""
    H = _hierarchy_cpu(name)
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


@pytest.mark.parametrize("name", BLOCKS)
@pytest.mark.parametrize("smoothing", [1, 2])
def test_vcycle_matches_the_restatement_and_is_symmetric(name, smoothing):
    H = _hierarchy_cpu(name)
    h = _hierarchy(name)
    B = _random(H, 0, 60)
    B[:, :H.N] = 0.0
    Z = h.vcycle(_dev(B).reshape(B.shape[0], -1, H.N), smoothing).cpu().numpy().reshape(B.shape)
    expect = np.stack([H.vcycle(b.copy(), smoothing) for b in B])
    err = _relmax(Z, expect)
    sym = abs(B[0] @ Z[1] - B[1] @ Z[0]) / max(abs(B[0] @ Z[1]), abs(B[1] @ Z[0]))
    print("V-cycle %s, %d sweeps: %.2e, symmetry %.2e" % (name, smoothing, err, sym))
    assert err < TOL_VCYCLE_BLOCKS[name]
    assert sym < 1e-12
    assert np.all(Z[:, :H.N] == 0.0)
    h.close()


# ---- tensor and gradient of a given field ----

def _random_field(pr, seed):
    Wp = np.random.default_rng(seed).standard_normal((pr["L"].shape[1], pr["N"] * int(np.prod(pr["ne"]))))
    return Wp, hc.to_full(pr["ne"], Wp)


@pytest.mark.parametrize("name", ["tensor-2d", "tensor-3d"])
def test_tensor_of_a_given_field_with_a_capped_grid(name):
    pr = _problem(name)
    assert mg.workgroups(np.prod(pr["ne"])) > 512                                    # more workgroups of elements than the grid takes
    Wp, full = _random_field(pr, 70)
    Eh = hom.homogenizedElasticityTensor_device(torch.from_numpy(full), _make(name)).D
    err = _relmax(Eh, hc.tensor(pr["ne"], Wp, pr["L"], pr["D"], pr["vol"], pr["E"]))
    print("tensor %s: %.2e" % (name, err))
    assert err < TOL_TENSOR[name]


@pytest.mark.parametrize("name", BLOCKS)
def test_gradient_of_a_given_field(name):
    pr = _problem(name)
    Wp, full = _random_field(pr, 71)
    G = hom.homogenizedElasticityTensorGradient(list(full), _make(name))
    expect = pr["dE"][:, None, None] * hc.gradient(pr["ne"], Wp, pr["K0"], pr["L"], pr["D"], pr["vol"])
    err = _relmax(G, expect)
    print("gradient %s: %.2e" % (name, err))
    assert err < TOL_GRADIENT
    assert np.array_equal(G, np.transpose(G, (0, 2, 1)))                              # the upper triangle mirrored


# ---- reductions over more than 256 partials ----

def _eight(solve, c):
    """(status, error text, W [S, nd], iterations, |r|/|b|) of ``solve(Wp, its, res)`` stopped after 8 iterations"""
    Wp = torch.empty((c.S, c.pn, c.N), dtype=torch.float64, device="cuda")
    its, res = (ctypes.c_int * c.S)(), (ctypes.c_double * c.S)()
    status = solve(Wp, its, res)
    return status, _lib.load().vfem_last_error().decode(), Wp, list(its), np.array(list(res))


def test_eight_iterations_equal_eight_iterations():
    """2d-partials, max_iter = 8: the field left in place and the reported |r|/|b| against the restatement's eighth iterate"""
    name = "2d-partials"
    pr = _problem(name)
    assert mg.workgroups(np.prod(pr["ne"])) == 320
    c = hom._Cell(_make(name))
    lib = _lib.load()

    def jacobi(Wp, its, res):
        return lib.vfem_hom_solve_cells(*c.head(), pv._ptr(Wp), SOLVER_TOL, 8, its, res, pv._stream())

    status, text, W, its, res = _eight(jacobi, c)
    assert status == 1 and "no convergence in 8 iterations" in text
    assert its == [8, 8, 8]
    X, its_cpu = hc.pcg_columns(pr["K"], pr["b"], 2, SOLVER_TOL, max_iter=8)
    assert its_cpu == [8, 8, 8]
    err_w, err_r = _relmax(W.cpu().numpy().reshape(X.shape), X), _relmax(res, _true_residuals(pr, X))
    print("eight iterations, block Jacobi: w %.2e, |r|/|b| %.2e (%s)" % (err_w, err_r, res))
    assert err_w < TOL_EIGHT["jacobi"] and err_r < TOL_EIGHT["jacobi"]
    # the fixed summation order with more than 256 partials
    status, _, W2, its2, res2 = _eight(jacobi, c)
    assert status == 1 and torch.equal(W, W2) and its2 == its and np.array_equal(res, res2)

    # For the multigrid half the device is handed the restatement's element constants.  The simulator's K0 and the restatement's own
    # quadrature differ in the last bit (2.6e-16), by the same amount in every element, and a Galerkin product adds such a difference
    # up coherently: the level operators of the two drift apart four-fold per level (3.5e-16 on level 0, 1.4e-13 on the seventh), the
    # coarsest solve (condition 86) carries that into the V-cycle (1.0e-12 on b) and the truncated iterates differ by 2.5e-12.  That
    # is a property of the inputs, not of the arithmetic this bound was derived for; with equal inputs the seventh level agrees to
    # 5.2e-15.  (A converged solve does not see any of it: test_full_solve_with_more_than_256_partials uses the simulator's own K0.)
    c = hom._Cell(_make(name))
    assert _relmax(c.K0, pr["K0"]) < 1e-13 and _relmax(c.L, pr["L"]) < 1e-13
    c.K0, c.L = np.ascontiguousarray(pr["K0"]), np.ascontiguousarray(pr["L"])
    h = hom._Hierarchy(c)
    H = _hierarchy_cpu(name)
    assert h.dims == H.dims and len(H.dims) == 7
    status, text, W, its, res = _eight(lambda Wp, i, r: h.solve(Wp, SOLVER_TOL, 8, 1, i, r), c)
    h.close()
    assert status == 1 and "no convergence in 8 iterations" in text
    assert its == [8, 8, 8]
    X, its_cpu = mg.pcg_columns(H, pr["b"], SOLVER_TOL, 1, max_iter=8)
    assert its_cpu == [8, 8, 8]
    err_w, err_r = _relmax(W.cpu().numpy().reshape(X.shape), X), _relmax(res, _true_residuals(pr, X))
    print("eight iterations, multigrid: w %.2e, |r|/|b| %.2e (%s)" % (err_w, err_r, res))
    assert err_w < TOL_EIGHT["multigrid"] and err_r < TOL_EIGHT["multigrid"]


def test_full_solve_with_more_than_256_partials():
    """2d-partials by multigrid PCG: the restatement's iteration counts, and the true residual of the device's field formed with the
    restatement's matrix (no direct solve)"""
    name = "2d-partials"
    pr = _problem(name)
    W = hom.solveCellProblems_device(_make(name), tol=SOLVER_TOL, preconditioner="multigrid")
    its, reported = list(hom.last_iterations), np.array(hom.last_relative_residuals)
    assert hom.last_levels == mg.level_dims(pr["ne"])
    true = _true_residuals(pr, _periodic(pr["ne"], W.cpu().numpy()))
    print("2d-partials: iterations %s (restatement %s), |r|/|b| reported %s, true %s, gap %.2e"
          % (its, PARTIALS_ITERATIONS, reported, true, np.abs(reported - true).max()))
    assert len(its) == 3 and all(abs(g - c) <= 2 for g, c in zip(its, PARTIALS_ITERATIONS))
    assert np.all(reported <= SOLVER_TOL)
    assert np.all(true <= SOLVER_TOL + PARTIALS_GAP)
    assert np.abs(reported - true).max() <= PARTIALS_GAP


# ---- the per-column state machine ----

@pytest.mark.parametrize("name", ["lam-2d", "lam-3d"])
def test_columns_that_finish_far_apart(name):
    """a laminate's normal and shear cases need very different numbers of block-Jacobi iterations: the first columns to converge stay
    frozen through several read-backs of the host while the last ones iterate on"""
    pr = _problem(name)
    ne, real = pr["ne"], [q for q in range(len(pr["b"])) if q not in LAMINATE_NOISE[name]]
    X, its_cpu = hc.pcg_columns(pr["K"], pr["b"], pr["N"], SOLVER_TOL)
    assert its_cpu == LAMINATE_ITERATIONS[name]
    # the cell is fit for this test only while a frozen column passes at least one read-back (every 8 iterations)
    assert max(its_cpu[q] for q in real) - min(its_cpu[q] for q in real) >= 9
    sim = _make(name)
    w = np.stack(hom.solveCellProblems(sim, tol=SOLVER_TOL))
    its = list(hom.last_iterations)
    print("iterations %s: device %s, restatement %s" % (name, its, its_cpu))
    assert np.all(np.isfinite(w))
    assert all(r <= SOLVER_TOL for r in hom.last_relative_residuals)
    full = hc.to_full(ne, X)
    for q in real:
        err = _relmax(w[q], full[q])
        print("%s case %d: w %.2e" % (name, q, err))
        assert abs(its[q] - its_cpu[q]) <= 2
        assert err < TOL_LAMINATE[name]
    for q in LAMINATE_NOISE[name]:
        print("%s noise case %d: max|w| %.2e of %.2e, %d iterations" % (name, q, np.abs(w[q]).max(), np.abs(w).max(), its[q]))
        assert np.abs(w[q]).max() < 1e-12 * np.abs(w).max()
    if name == "lam-3d":
        lam, mu = hc.lame(1.0, 0.3)
        exact = hc.laminate_closed_form([(lam, mu), (0.5 * lam, 0.5 * mu)], [0.5, 0.5])
        err = _relmax(hom.homogenizedElasticityTensor(list(w), sim).D, exact)
        print("laminate 64x4x4: %.2e" % err)
        assert err < TOL_EH["3d"]


@pytest.mark.parametrize("name", list(mg.UNIFORM_CELLS))
@pytest.mark.parametrize("preconditioner", ["jacobi", "multigrid"])
def test_uniform_cell(name, preconditioner):
    """no fluctuation: the right-hand sides are zero or rounding noise, which must neither raise nor grow"""
    _, _, D, rho, gamma, Emin = mg.block_cell(name)
    sim = _make(name)
    w = np.stack(hom.solveCellProblems(sim, tol=SOLVER_TOL, preconditioner=preconditioner))
    print("uniform %s, %s: max|w| %.2e, iterations %s" % (name, preconditioner, np.abs(w).max(), hom.last_iterations))
    assert np.all(np.isfinite(w)) and np.all(np.isfinite(hom.last_relative_residuals))
    assert np.abs(w).max() < 1e-12
    Eh = hom.homogenizedElasticityTensor(list(w), sim).D
    assert np.all(np.isfinite(Eh))
    assert _relmax(Eh, hc.moduli(rho, 1.0, Emin, gamma)[0][0] * D) < 1e-13


# ---- a singular cell is an error ----

@pytest.mark.parametrize("preconditioner", ["jacobi", "multigrid"])
def test_a_void_wider_than_one_element_is_a_breakdown(preconditioner):
    """void-2d: nine nodes have no diagonal block to invert, so r . z is NaN at the first preconditioning.  With multigrid the same
    happens in the first V-cycle: the hierarchy itself is built (12x12, 6x6, 3x3; the coarse nodes of the 3x3 level all carry
    stiffness, so the coarsest matrix is positive definite: smallest eigenvalue 0.20 in the restatement), and the level-0 sweep
    spreads the NaN of the inverted blocks"""
    sim = _make("void-2d")
    hom.last_iterations, hom.last_relative_residuals = [], []
    with pytest.raises(RuntimeError, match=r"breakdown in strain case 0 after 0 iterations.*zero modulus"):
        hom.solveCellProblems(sim, tol=SOLVER_TOL, preconditioner=preconditioner)
    print("void-2d, %s: iterations %s, |r|/|b| %s" % (preconditioner, hom.last_iterations, hom.last_relative_residuals))
    assert hom.last_iterations == [0, 0, 0]
    assert len(hom.last_relative_residuals) == 3 and all(not r <= SOLVER_TOL for r in hom.last_relative_residuals)


def test_a_nan_modulus_is_a_breakdown():
    c = hom._Cell(_make("8x6"))
    c.E[13] = float("nan")
    Wp = torch.empty((c.S, c.pn, c.N), dtype=torch.float64, device="cuda")
    its, res = (ctypes.c_int * c.S)(), (ctypes.c_double * c.S)()
    lib = _lib.load()
    status = lib.vfem_hom_solve_cells(*c.head(), pv._ptr(Wp), SOLVER_TOL, 100, its, res, pv._stream())
    text = lib.vfem_last_error().decode()
    print("NaN modulus: %s; |r|/|b| %s" % (text, list(res)))
    assert status == 1 and "breakdown" in text and "non-finite moduli" in text
    assert list(its) == [0, 0, 0]
    assert all(math.isnan(r) for r in res)                       # every right-hand side holds the NaN: not a residual of 0
