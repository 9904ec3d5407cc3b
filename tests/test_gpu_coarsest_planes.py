"""-m gpu: the plane-block coarsest-level solver (plane_spd.hip; MultigridSolver1_1_1.coarsestSolver = "planes", and "auto" above the
dense inverse's 40 000 dofs).  The reference solves its coarsest level with CHOLMOD at any size (TPS.hh:834-865).

The yardstick of the solve is the dense path on the same input: both are exact up to eps x condition number with different
elimination orders, and the residual is evaluated by the level's own operator kernel (applyK), which shares nothing with either
factorisation.  Residuals measured on the MI355X (relative, 2-norm over the free dofs; planes / dense): DESIGN section 3.2."""
import numpy as np
import pytest

from helpers import BC_BRIDGE, BC_CANTILEVER, make_hip, record_deltas, seeded_density

pytestmark = pytest.mark.gpu

DOMAIN = ([0, 0, 0], [2, 1, 1])
BCS = {"cantilever": BC_CANTILEVER, "bridge": BC_BRIDGE}


def _density(ne, kind, seed=5):
    """random in [0.1, 1]; "void": a quarter of the elements at 0 on top (the modulus contrast of a late design)"""
    rng = np.random.default_rng(seed)
    rho = rng.uniform(0.1, 1.0, int(np.prod(ne)))
    if kind == "void":
        rho[rng.permutation(rho.size)[:rho.size // 4]] = 0.0
    return rho


def _hierarchy(ne, bc, levels, rho, mode=None, domain=DOMAIN):
    t = make_hip(ne, domain, BCS[bc], rho)
    mg = t.multigridSolver(levels)
    if mode is not None:
        mg.coarsestSolver = mode
    return t, mg


def _rel_residual(mg, x, b, mask):
    r = (b - mg.applyK(mg.L, x))[~mask]
    return float(np.linalg.norm(r) / np.linalg.norm(b[~mask]))


def _check_solve(mg, tag):
    """planes against dense on one operator: residual within 10 x max(dense, n 2^-52); x = 0 and b ignored on the fixed dofs"""
    mask = mg.getSimulator(mg.L).dirichletMask
    n = mask.size
    b = np.random.default_rng(17).standard_normal(mask.shape)
    b2 = b.copy()
    b2[mask] = 7.0 - 3.0 * b[mask]
    mg.coarsestSolver = "planes"
    x = mg.coarsestSolve_device(b).cpu().numpy()
    x2 = mg.coarsestSolve_device(b2).cpu().numpy()
    res_p = _rel_residual(mg, x, b, mask)
    mg.coarsestSolver = "dense"
    xd = mg.coarsestSolve_device(b).cpu().numpy()
    res_d = _rel_residual(mg, xd, b, mask)
    print("%s: n = %d, residual planes %.3e, dense %.3e" % (tag, n, res_p, res_d))
    record_deltas("coarsest_planes/" + tag, {"n": n, "residual_planes": res_p, "residual_dense": res_d})
    assert np.all(np.isfinite(x))
    assert not mask.any() or np.abs(x[mask]).max() == 0.0
    assert np.array_equal(x, x2)
    assert res_p <= 10.0 * max(res_d, n * 2.0 ** -52), (res_p, res_d)
    return xd


@pytest.mark.parametrize("kind", ["random", "void"])
@pytest.mark.parametrize("bc", ["cantilever", "bridge"])
@pytest.mark.parametrize("ne,levels", [((16, 12, 8), 1), ((32, 16, 16), 2), ((8, 6, 4), 0)])
def test_plane_solve_matches_the_dense_residual(ne, levels, bc, kind):
    """coarsest 9 x 7 x 5 nodes (m = 105, no multiple of 64; the stencil is the temporary of a one-level hierarchy), 9 x 5 x 5 (the
    level's own stencil) and 9 x 7 x 5 with no coarsening at all; a cantilever's plane 0 is entirely fixed (S_0 = I), a bridge's
    planes partly"""
    _, mg = _hierarchy(ne, bc, levels, _density(ne, kind))
    _check_solve(mg, "%dx%dx%d_L%d_%s_%s" % (ne + (levels, bc, kind)))


@pytest.mark.parametrize("fmg", [False, True])
@pytest.mark.parametrize("bc", ["cantilever", "bridge"])
def test_whole_solves_agree_between_the_two_coarsest_solvers(bc, fmg):
    """PCG to 1e-8 preconditioned by V-cycles / full-multigrid cycles: same iteration count, compliance to 1e-9"""
    ne = (32, 16, 16)
    out = {}
    for mode in ("planes", "dense"):
        t, mg = _hierarchy(ne, bc, 2, seeded_density(ne, 88, "proxy"), mode)
        f = t.buildLoadVector_device()
        u = mg.preconditionedConjugateGradient_device(np.zeros((t.numNodes(), 3)), f, 200, 1e-8, fullMultigrid=fmg)
        assert mg.last_iterations < 200
        out[mode] = (mg.last_iterations, float((f * u).sum()))
    print("%s fmg=%d: planes %r, dense %r" % (bc, fmg, out["planes"], out["dense"]))
    assert out["planes"][0] == out["dense"][0]
    assert abs(out["planes"][1] - out["dense"][1]) <= 1e-9 * abs(out["dense"][1])


def test_coarsest_level_above_the_dense_limit_solves_in_auto_mode():
    """64 x 64 x 32 with one coarsening level: 33 x 33 x 17 nodes = 55 539 dofs on the coarsest level, which the dense inverse
    refuses; m = 1 683, 0.75 GB of blocks.  Against the same problem with four levels (dense coarsest)"""
    ne, dom = (64, 64, 32), ([0, 0, 0], [2, 2, 1])
    rho = seeded_density(ne, 88, "proxy")
    comp = {}
    for levels in (1, 4):
        t, mg = _hierarchy(ne, "cantilever", levels, rho, domain=dom)
        assert mg.coarsestSolver == "auto"
        f = t.buildLoadVector_device()
        u = mg.preconditionedConjugateGradient_device(np.zeros((t.numNodes(), 3)), f, 300, 1e-10, fullMultigrid=True)
        assert mg.last_iterations < 300 and mg.last_relative_residual <= 1e-10, (levels, mg.last_iterations, mg.last_relative_residual)
        comp[levels] = float((f * u).sum())
        if levels == 1:
            m, nx, nn = 3 * 33 * 17, 33, 33 * 33 * 17
            assert mg.coarsestBytes() == 8 * (nx * m * m + 243 * nn)        # the blocks and the solver's copy of the rows
        else:
            assert mg.coarsestBytes() == 8 * (3 * 5 * 5 * 3) ** 2
        print("levels %d: %d iterations, compliance %.15e" % (levels, mg.last_iterations, comp[levels]))
    assert abs(comp[1] - comp[4]) <= 1e-8 * abs(comp[4])


def test_unknown_mode_and_oversized_planes_are_refused():
    from ndr_amd import _lib
    t, mg = _hierarchy((8, 6, 4), "cantilever", 0, None)
    with pytest.raises(RuntimeError, match="coarsestSolver"):
        mg.coarsestSolver = "cholmod"
    assert mg.coarsestSolver == "auto"
    lib = _lib.load()
    assert lib.vfem_mg_set_coarsest_solver(mg._h, 3) == 1 and b"unknown coarsest-level solver mode" in lib.vfem_last_error()
    # 8 x 512 x 512 with one level: planes of 3 x 257 x 257 = 198 147 dofs, 314 GB per block
    t, mg = _hierarchy((8, 512, 512), "cantilever", 1, None, domain=([0, 0, 0], [1, 64, 64]))
    for mode in ("auto", "planes"):
        mg.coarsestSolver = mode
        with pytest.raises(RuntimeError, match="coarsest grid too large .* use more coarsening levels"):
            mg.updateElementStiffnessMatrices()
        assert mg.coarsestBytes() == 0


def test_factorisation_follows_the_operator_and_the_mode():
    from ndr_amd import pyVoxelFEM as pv
    ne = (16, 12, 8)
    t, mg = _hierarchy(ne, "bridge", 1, _density(ne, "random"), "dense")
    mask = mg.getSimulator(1).dirichletMask
    b = np.random.default_rng(17).standard_normal(mask.shape)
    x_dense = mg.coarsestSolve_device(b).cpu().numpy()
    assert mg.coarsestBytes() == 8 * mask.size ** 2

    def factorisations():
        return pv.benchmark_to_dict().get("coarsestPlaneFactorization", {"invocations": 0})["invocations"]

    pv.benchmark_reset()
    mg.coarsestSolver = "planes"
    x1 = mg.coarsestSolve_device(b).cpu().numpy()
    assert factorisations() == 1 and mg.coarsestBytes() == 8 * (9 * 105 * 105 + 243 * 315)
    x2 = mg.coarsestSolve_device(b).cpu().numpy()
    mg.coarsestSolver = "planes"                                           # the same mode again: nothing is discarded
    f = t.buildLoadVector_device()
    mg.preconditionedConjugateGradient_device(np.zeros((t.numNodes(), 3)), f, 100, 1e-8)
    assert factorisations() == 1 and np.array_equal(x1, x2)                # unchanged densities: the factorisation is kept
    t.setElementDensities(_density(ne, "void", seed=6))
    _check_solve(mg, "16x12x8_L1_bridge_after_setElementDensities")        # planes on the new operator, then dense
    assert factorisations() == 2
    t.setElementDensities(_density(ne, "random"))
    mg.coarsestSolver = "planes"
    assert np.array_equal(mg.coarsestSolve_device(b).cpu().numpy(), x1)    # fixed summation order: the first factorisation again
    mg.coarsestSolver = "dense"
    assert np.array_equal(mg.coarsestSolve_device(b).cpu().numpy(), x_dense)
    assert factorisations() == 3
