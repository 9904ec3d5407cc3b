"""-m gpu: linearised buckling on the device (ndr_amd.buckling, vfem_buckling_*): the geometric stiffness operator, the adjoint load
and the gradient kernels, the block eigensolver on (K_G, K), the p-norm objective, its autograd node and its use as an MMA
constraint, against tests/buckling_cpu.py.

Bounds.  Every figure named "restatement" was measured on the CPU with tests/buckling_cpu.py (tests/test_buckling_cpu.py prints them).
  Kernels (apply, adjoint load, gradient): the reference is the restatement evaluated in np.longdouble; the rounding floor of the
    formula is what the same restatement in float64 differs from it, relative to the largest entry, and the bound is 16 times that
    floor (another summation order), computed per case and printed with it.
  bucklingModes at tol 1e-9, four modes, two guard columns: the restatement's LOBPCG differs from scipy.linalg.eigh by 3.3e-14
    (column2), 5.8e-14 (column3) and 2.5e-15 (cantilever2) of |nu_1|: ten times these is below the floor 1e-12.  Mode overlap and
    Phi^T K Phi - I: 1.3e-14 / 5.3e-14 / 1.1e-15 and 3.7e-14 / 3.4e-14 / 2.4e-15 in the restatement; bounded at ten times these,
    not below 1e-12.  It takes 19 / 18 / 25 iterations: the caps are 38 / 36 / 50.
  Objective at tol 1e-9: the restatement's LOBPCG chain differs from its dense chain by J 3.3e-14 / 5.8e-14 (relative) and gradient
    9.9e-13 / 1.5e-13 of the largest entry (column2 / column3): ten times these is below the floor 1e-11, which is the bound.
  Central difference of J along a default_rng(1) direction, step 1e-5, eigensolves to 1e-10: the restatement's mismatch (dense
    solves) is 2.43e-8 (column2) and 3.69e-9 (column3); the bounds are ten times these.
  The 2-level V-cycle runs on column3even (8 x 4 x 4, otherwise column3): no multigrid hierarchy of this library halves the 8 x 4 x 3
    elements of column3 (the solver's constructor raises "Grid size currently must be divisible by 2^numCoarseningLevels").  The
    bounds follow the same rule:
    the restatement differs from eigh by 8.0e-14 (nu), 4.0e-14 (overlap), 1.4e-14 (orthonormality) in 17 iterations.
  Through MultigridComplianceObjective (column3even, 2 levels, PCG to a relative residual of 1e-12 for u and for the adjoint v): the
    same rule as the objective above, with both CPU mismatches of this fixture.  The restatement's LOBPCG chain differs from its
    dense chain by J 7.6e-14 and gradient 1.5e-12; the restatement's chain with u and v from a conjugate gradient to 1e-12
    (stress_cpu.solve_cg) differs from its direct chain by J 7.9e-15 and gradient 2.7e-12 (tests/test_buckling_cpu.py prints both).
    The bounds are ten times the larger of the two, not below 1e-11: J 1e-11, gradient 2.7e-11.
  The refusal of a load that compresses nothing is tested on a 2 x 1 bar in pure tension.  column2 with the load reversed is no such
    load: it has 20 buckling modes of its own (lambda_1 = 0.780), see test_the_pulled_column_has_the_pushed_column_s_operator_negated.

Measured on an MI355X:
  apply 1.6e-16 .. 4.5e-16 of the largest entry over the 24 cases against floors of 1.3e-16 .. 4.1e-16 (bounds 2.1e-15 .. 6.6e-15);
    adjoint load 1.9e-16 / 2.2e-16 (floors 5.6e-16 / 8.3e-16), gradient kernel 1.8e-16 / 2.8e-16 (floors 1.1e-15 / 7.9e-15) on 7 x 5 /
    6 x 4 x 5; off-line buffers and a second run bit-identical.
  bucklingModes column2: 19 iterations, nu 3.8e-13, 1 - overlap 4.2e-14, Phi^T K Phi - I 1.4e-13, residuals 8.5e-10; column3: 18, 1.9e-13,
    3.9e-14, 1.4e-13, 2.8e-10; cantilever2: 25, 1.6e-13, 1.1e-15, 2.2e-15, 4.6e-10; column3even (2-level V-cycle): 22, 1.6e-13, 9.1e-15,
    8.3e-14, 2.7e-10; P dropped 1 / 0 / 0 / 0 times; every warm start from the converged block: 0 iterations.
  objective: J 3.8e-13 / 1.9e-13, gradient 9.5e-13 / 4.9e-13 (column2 / column3); central difference 9.8e-9 / 1.5e-9; cantilever2 42
    positive and 150 negative entries; through multigrid J 1.3e-13, gradient 2.2e-12.
  three MMA steps on column2: J 297.725 -> 229.079 under the bound 312.612, the restatement at the final densities within 3.1e-13.
  The whole file runs in 5 s.
  Against the parent commit every test fails at import: the module and the entry points do not exist.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import buckling_cpu as bc
import stress_cpu as sc

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor, _lib, buckling, mma         # noqa: E402
from ndr_amd import pyVoxelFEM as pv                              # noqa: E402

MARGIN = 16.0
FLOOR = 1e-12
TOL_SOLVE = 1e-9
NAMES = ["column2", "column3", "cantilever2"]
TOL_NU = {"column2": max(10 * 3.3e-14, FLOOR), "column3": max(10 * 5.8e-14, FLOOR), "cantilever2": max(10 * 2.5e-15, FLOOR),
          "column3even": max(10 * 8.0e-14, FLOOR)}
TOL_OVERLAP = {"column2": max(10 * 1.3e-14, FLOOR), "column3": max(10 * 5.3e-14, FLOOR), "cantilever2": max(10 * 1.1e-15, FLOOR),
               "column3even": max(10 * 4.0e-14, FLOOR)}
TOL_ORTH = {"column2": max(10 * 3.7e-14, FLOOR), "column3": max(10 * 3.4e-14, FLOOR), "cantilever2": max(10 * 2.4e-15, FLOOR),
            "column3even": max(10 * 1.4e-14, FLOOR)}
MAX_ITERATIONS = {"column2": 2 * 19, "column3": 2 * 18, "cantilever2": 2 * 25, "column3even": 2 * 17}
TOL_J = {"column2": max(10 * 3.3e-14, 1e-11), "column3": max(10 * 5.8e-14, 1e-11)}
TOL_GRADIENT = {"column2": max(10 * 9.9e-13, 1e-11), "column3": max(10 * 1.5e-13, 1e-11)}
FD_STEP = 1e-5
TOL_FD = {"column2": 10 * 2.43e-8, "column3": 10 * 3.69e-9}
TOL_MG_J, TOL_MG_GRADIENT = max(10 * 7.6e-14, 10 * 7.9e-15, 1e-11), max(10 * 1.5e-12, 10 * 2.7e-12, 1e-11)

# 40 x 37 and 12 x 10 x 9 span several workgroups of the node kernel (64 lanes along the last axis by 4 rows, one block per layer of
# axis 0 in 3-D); 5 x 70 and 3 x 3 x 70 have 71 nodes along the last axis and so cross the block edge at 64
SHAPES = [(7, 5), (40, 37), (5, 70), (6, 4, 5), (12, 10, 9), (3, 3, 70)]
EDGES = {2: (0.5, 0.3), 3: (0.5, 0.3, 0.7)}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _name(ne):
    return "x".join(map(str, ne))


def _dev(a, off=False):
    """a device copy; off: a view that starts 8 bytes off a 16-byte line"""
    a = np.ascontiguousarray(a)
    if not off:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    view = buf[1:].reshape(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8
    return view


def _head(ne, h, D):
    n, hh, DD = np.asarray(ne, dtype=np.int64), np.ascontiguousarray(h, dtype=np.float64), np.ascontiguousarray(D, dtype=np.float64)
    return (len(ne), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(hh), _dp(DD)), (n, hh, DD)    # (the arrays stay alive)


def _rel(got, ref):
    """the largest difference relative to the largest entry of the (longdouble) reference"""
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max() / np.abs(ref).max())


# ---- the three kernels against the restatement in extended precision ----

@functools.lru_cache(maxsize=None)
def _kernel_case(ne):
    N = len(ne)
    rng = np.random.default_rng(400 + int(np.prod(ne)))
    nn, nel = sc.num_nodes(ne), int(np.prod(ne))
    h = EDGES[N]
    A = rng.standard_normal((3 if N == 2 else 6,) * 2)
    D = bc.hc.isotropic_D(1.3, 0.3, N) + 0.05 * (A + A.T)                     # symmetric, every entry filled
    c = dict(ne=ne, N=N, h=h, D=D, T=bc.geometric_element_matrices(D, h), K0=bc.hc.element_constants(D, h)[0],
             mG=rng.uniform(0.05, 1.0, size=nel), dmG=rng.uniform(0.05, 1.0, size=nel), dE=rng.uniform(0.05, 1.0, size=nel),
             u=rng.standard_normal(nn * N), v=rng.standard_normal(nn * N), X=rng.standard_normal((3, nn * N)),
             coef=rng.standard_normal(3), cK=rng.standard_normal(3), fixed=rng.uniform(size=(nn, N)) < 0.2)
    bits = np.zeros(nn, dtype=np.uint8)
    for a in range(N):
        bits |= c["fixed"][:, a].astype(np.uint8) << a
    c["bits"] = bits
    return c


@functools.lru_cache(maxsize=None)
def _apply_reference(ne, ncols, masked):
    c = _kernel_case(ne)
    args = (c["ne"], c["T"], c["mG"], c["u"], c["X"][:ncols], c["fixed"] if masked else None)
    ref = bc.kernel_apply(*args, dtype=np.longdouble)
    return ref, _rel(bc.kernel_apply(*args), ref)


def _run_apply(c, ncols, masked, off=False):
    args, keep = _head(c["ne"], c["h"], c["D"])
    X, mG, u = _dev(c["X"][:ncols], off), _dev(c["mG"], off), _dev(c["u"], off)
    Y = _dev(np.full((ncols, c["X"].shape[1]), np.nan), off)
    mask = torch.from_numpy(c["bits"]).cuda() if masked else None
    _lib.check(_lib.load().vfem_buckling_geom_apply(*args, _p(mG), _p(u), _p(mask), ncols, _p(X), _p(Y), pv._stream()))
    torch.cuda.synchronize()
    return Y


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_geometric_apply_matches_the_assembled_operator(ne, ncols, masked):
    c = _kernel_case(ne)
    ref, floor = _apply_reference(ne, ncols, masked)
    Y = _run_apply(c, ncols, masked)
    err = _rel(Y.cpu().numpy(), ref)
    print("geometric apply %s, %d columns, %s: %.2e (floor %.2e, bound %.2e)" % (_name(ne), ncols, "masked" if masked else "free", err,
                                                                                floor, MARGIN * floor))
    assert err < MARGIN * floor
    if masked:
        assert not Y.cpu().numpy()[:, c["fixed"].reshape(-1)].any()
    assert torch.equal(_run_apply(c, ncols, masked), Y)                                # run to run


@pytest.mark.parametrize("ne", [(40, 37), (12, 10, 9)], ids=_name)
def test_geometric_apply_on_buffers_8_bytes_off_a_16_byte_line(ne):
    c = _kernel_case(ne)
    assert torch.equal(_run_apply(c, 3, True, off=True), _run_apply(c, 3, True))


def _run_adjoint_load(c, masked, off=False):
    args, keep = _head(c["ne"], c["h"], c["D"])
    Phi, mG = _dev(c["X"], off), _dev(c["mG"], off)
    a = _dev(np.full(c["u"].shape, np.nan), off)
    mask = torch.from_numpy(c["bits"]).cuda() if masked else None
    coef = np.ascontiguousarray(c["coef"])
    _lib.check(_lib.load().vfem_buckling_adjoint_load(*args, _p(mG), _p(mask), 3, _dp(coef), _p(Phi), _p(a), pv._stream()))
    torch.cuda.synchronize()
    return a


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("ne", [(7, 5), (6, 4, 5)], ids=_name)
def test_adjoint_load_kernel_matches_the_restatement(ne, masked):
    c = _kernel_case(ne)
    args = (c["ne"], c["T"], c["mG"], c["X"], c["coef"], c["fixed"] if masked else None)
    ref = bc.kernel_adjoint_load(*args, dtype=np.longdouble)
    floor = _rel(bc.kernel_adjoint_load(*args), ref)
    a = _run_adjoint_load(c, masked)
    err = _rel(a.cpu().numpy(), ref)
    print("adjoint load %s %s: %.2e (floor %.2e, bound %.2e)" % (_name(ne), "masked" if masked else "free", err, floor, MARGIN * floor))
    assert err < MARGIN * floor
    if masked:
        assert not a.cpu().numpy()[c["fixed"].reshape(-1)].any()
    assert torch.equal(_run_adjoint_load(c, masked), a)
    assert torch.equal(_run_adjoint_load(c, masked, off=True), a)


def _run_gradient(c, off=False):
    args, keep = _head(c["ne"], c["h"], c["D"])
    t = {k: _dev(c[k], off) for k in ("dmG", "dE", "u", "v", "X")}
    g = _dev(np.full(c["mG"].shape, np.nan), off)
    K0, cG, cK = np.ascontiguousarray(c["K0"]), np.ascontiguousarray(c["coef"]), np.ascontiguousarray(c["cK"])
    _lib.check(_lib.load().vfem_buckling_gradient(*args, 3, _dp(K0), _dp(cG), _dp(cK), _p(t["dmG"]), _p(t["dE"]), _p(t["u"]), _p(t["v"]),
                                                  _p(t["X"]), _p(g), pv._stream()))
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("ne", [(7, 5), (6, 4, 5)], ids=_name)
def test_gradient_kernel_matches_the_restatement(ne):
    c = _kernel_case(ne)
    args = (c["ne"], c["T"], c["K0"], c["dmG"], c["dE"], c["u"], c["v"], c["X"], c["coef"], c["cK"])
    ref = bc.kernel_gradient(*args, dtype=np.longdouble)
    floor = _rel(bc.kernel_gradient(*args), ref)
    g = _run_gradient(c)
    err = _rel(g.cpu().numpy(), ref)
    print("gradient kernel %s: %.2e (floor %.2e, bound %.2e)" % (_name(ne), err, floor, MARGIN * floor))
    assert err < MARGIN * floor
    assert torch.equal(_run_gradient(c), g) and torch.equal(_run_gradient(c, off=True), g)


# ---- the public operator and the eigensolver ----

def _simulator(name, reverse=False):
    ne, h, D, rho, fixed, f = bc.case(name)
    N = len(ne)
    sim = pv.TensorProductSimulator([1] * N, [np.zeros(N), np.array(ne) * np.array(h)], list(ne))
    sim.ETensor = ElasticityTensor(*bc.CASES[name][2], dim=N)
    sim.E_0, sim.E_min, sim.gamma = bc.E0, bc.EMIN, bc.GAMMA
    sim.setElementDensities(rho)
    sim.dirichletMask = fixed
    sim.setLoads_device(torch.from_numpy(-f if reverse else f).cuda())
    return sim


def _solved(name, **kw):
    sim = _simulator(name, **kw)
    return sim, pv.ComplianceObjective(sim)


def test_public_geometric_operator():
    name = "column3"
    ref = bc.reference(name)
    op = ref["op"]
    sim = _simulator(name)
    X = np.random.default_rng(5).standard_normal((2, sim.numNodes(), 3))
    want = bc.kernel_apply(op["ne"], op["T"], op["mG"], op["u"], X.reshape(2, -1), op["fixed"])
    got = buckling.applyKG(sim, op["u"].reshape(-1, 3), X)
    assert got.shape == X.shape and np.abs(got.reshape(2, -1) - want).max() < 1e-13 * np.abs(want).max()
    one = buckling.applyKG_device(sim, torch.from_numpy(op["u"]).cuda(), torch.from_numpy(X[0]).cuda(), project=False)
    assert one.shape == (sim.numNodes(), 3)
    want = bc.kernel_apply(op["ne"], op["T"], op["mG"], op["u"], X[:1].reshape(1, -1))[0]
    assert np.abs(one.cpu().numpy().reshape(-1) - want).max() < 1e-13 * np.abs(want).max()
    mG, dmG = buckling.geometricMultipliers(sim)
    assert np.abs(mG.cpu().numpy() - op["mG"]).max() < 1e-14 and np.abs(dmG.cpu().numpy() - op["dmG"]).max() < 1e-14 * op["dmG"].max()
    half = buckling.geometricMultipliers(sim, stressExponent=0.5)[0].cpu().numpy()
    assert np.abs(half - bc.geometric_multiplier(bc.case(name)[3], 0.5)[0]).max() < 1e-14


@pytest.mark.parametrize("name,preconditioner", [("column2", "auto"), ("column3", "auto"), ("cantilever2", "auto"), ("column3even", "multigrid")])
def test_buckling_modes_match_the_dense_solver(name, preconditioner):
    ref = bc.reference(name)
    op = ref["op"]
    sim, solved = _solved(name)
    k = bc.NUM_MODES
    T = sim.multigridSolver(1) if preconditioner == "multigrid" else "auto"
    lam, Phi, info = buckling.bucklingModes(sim, solved._u, k, tol=TOL_SOLVE, preconditioner=T)
    assert isinstance(lam, np.ndarray) and lam.shape == (k,) and (lam > 0).all() and (np.diff(lam) > 0).all()
    assert np.array_equal(lam, -1.0 / info["nu"])
    assert Phi.shape == (k, sim.numNodes(), sim.N) and Phi.is_cuda
    P = Phi.cpu().numpy().reshape(k, -1).T
    Kf, free = op["K"], op["free"]
    err = np.abs(info["nu"] - ref["nu"]).max() / abs(ref["nu"][0])
    overlap = np.abs(np.einsum("ni,ni->i", ref["Phi"][free], Kf @ P[free]))
    orth = np.abs(P[free].T @ (Kf @ P[free]) - np.eye(k)).max()
    print("bucklingModes %s %s: %d iterations (P dropped %d times), nu %.2e, 1 - overlap %.2e, orthonormality %.2e, residuals %.2e"
          % (name, preconditioner, info["iterations"], info["droppedP"], err, np.abs(1.0 - overlap).max(), orth, info["residuals"].max()))
    assert err < TOL_NU[name]
    assert np.abs(1.0 - overlap).max() < TOL_OVERLAP[name] and orth < TOL_ORTH[name]
    assert info["residuals"].shape == (k,) and info["residuals"].max() <= TOL_SOLVE
    assert info["iterations"] <= MAX_ITERATIONS[name]
    assert not P[op["fixed"]].any()
    # a warm start from the converged block
    lam2, Phi2, info2 = buckling.bucklingModes(sim, solved._u, k, tol=TOL_SOLVE, preconditioner=T, X0=info["X"])
    print("  warm start: %d iterations" % info2["iterations"])
    assert info2["iterations"] <= 2 and np.abs(lam2 - lam).max() < FLOOR * lam.max()
    # and the same bits from the same start
    lam3, Phi3, _ = buckling.bucklingModes(sim, solved._u, k, tol=TOL_SOLVE, preconditioner=T)
    assert np.array_equal(lam3, lam) and torch.equal(Phi3, Phi)


def test_buckling_modes_that_do_not_converge_raise_and_name_the_residual():
    sim, solved = _solved("column2")
    with pytest.raises(RuntimeError, match=r"bucklingModes: no convergence in 2 iterations: the worst residual is \d\.\d+e-\d+"):
        buckling.bucklingModes(sim, solved._u, 2, tol=1e-12, maxIter=2)


# ---- the objective ----

def _objective(name, tol=TOL_SOLVE, **kw):
    sim, solved = _solved(name)
    return sim, buckling.BucklingObjective(solved, numModes=bc.NUM_MODES, P=bc.P_NORM, tol=tol, **kw)


@pytest.mark.parametrize("name", ["column2", "column3"])
def test_objective_matches_the_restatement(name):
    ref = bc.reference(name)
    sim, obj = _objective(name)
    J = obj.evaluate()
    g = obj.gradient()
    scale = np.abs(ref["gradient"]).max()
    errs = abs(J - ref["J"]) / ref["J"], np.abs(g - ref["gradient"]).max() / scale
    a, v = obj.adjointLoad_device().cpu().numpy().reshape(-1), obj.adjoint_device().cpu().numpy().reshape(-1)
    print("objective %s: J %.2e gradient %.2e (bounds %.1e %.1e), adjoint load %.2e adjoint %.2e; %d positive and %d negative entries"
          % (name, errs[0], errs[1], TOL_J[name], TOL_GRADIENT[name], np.abs(a - ref["a"]).max() / np.abs(ref["a"]).max(),
             np.abs(v - ref["v"]).max() / np.abs(ref["v"]).max(), (g > 0).sum(), (g < 0).sum()))
    assert errs[0] < TOL_J[name] and errs[1] < TOL_GRADIENT[name]
    assert not a[ref["op"]["fixed"]].any()
    lam = obj.loadFactors()
    assert np.array_equal(lam, -1.0 / obj.info()["nu"]) and 1.0 / J <= lam[0] <= bc.NUM_MODES ** (1.0 / bc.P_NORM) / J
    assert np.allclose(lam, -1.0 / ref["nu"], rtol=1e-11, atol=0.0)
    assert obj.modes_device().shape == (bc.NUM_MODES, sim.numNodes(), sim.N) and "X" not in obj.info()
    assert torch.equal(obj.gradient_device(), obj.gradient_device())
    # the state belongs to the displacement: nothing is solved again until `solved` solves again
    modes = obj.modes_device()
    assert obj.evaluate() == J and obj.modes_device() is modes
    # an update at the same densities is a warm start, guard columns included
    obj.updateCache(torch.from_numpy(bc.case(name)[3]).cuda())
    assert obj.modes_device() is not modes
    assert obj.info()["iterations"] <= 2 and abs(obj.evaluate() - J) < FLOOR * J


def test_gradient_of_the_cantilever_has_both_signs():
    ref = bc.reference("cantilever2")
    sim, obj = _objective("cantilever2")
    g = obj.gradient()
    print("cantilever2: %d positive and %d negative entries, gradient %.2e" % ((g > 0).sum(), (g < 0).sum(),
                                                                              np.abs(g - ref["gradient"]).max() / np.abs(ref["gradient"]).max()))
    assert (g > 0).any() and (g < 0).any()
    assert ((g > 0) == (ref["gradient"] > 0))[np.abs(ref["gradient"]) > 1e-6 * np.abs(ref["gradient"]).max()].all()


@pytest.mark.parametrize("name", ["column2", "column3"])
def test_central_difference_of_the_objective(name):
    sim, obj = _objective(name, tol=1e-10)
    rho0 = torch.from_numpy(bc.case(name)[3]).cuda()
    d = torch.from_numpy(np.random.default_rng(1).standard_normal(rho0.numel())).cuda()
    an = float(obj.gradient_device() @ d)
    fd = (obj.evaluate(rho0 + FD_STEP * d) - obj.evaluate(rho0 - FD_STEP * d)) / (2.0 * FD_STEP)
    err = abs(fd - an) / abs(an)
    print("central difference %s: %.2e (directional derivative %.6e, bound %.2e)" % (name, err, an, TOL_FD[name]))
    assert err < TOL_FD[name]


def test_objective_through_a_multigrid_compliance_objective():
    name = "column3even"
    ref = bc.reference(name)
    sim = _simulator(name)
    solved = pv.MultigridComplianceObjective(sim.multigridSolver(1))
    solved.tol, solved.cgIter = 1e-12, 400
    solved.updateCache(None)
    obj = buckling.BucklingObjective(solved, numModes=bc.NUM_MODES, P=bc.P_NORM, tol=TOL_SOLVE)
    J, g = obj.evaluate(), obj.gradient()
    errs = abs(J - ref["J"]) / ref["J"], np.abs(g - ref["gradient"]).max() / np.abs(ref["gradient"]).max()
    print("objective %s through multigrid: J %.2e gradient %.2e, %d iterations" % (name, errs[0], errs[1], obj.info()["iterations"]))
    assert errs[0] < TOL_MG_J and errs[1] < TOL_MG_GRADIENT


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_backward_is_the_gradient_times_the_incoming_gradient(dtype):
    name = "column2"
    ne = bc.CASES[name][0]
    sim, obj = _objective(name)
    rho = torch.from_numpy(bc.case(name)[3]).cuda().to(dtype).reshape(ne).requires_grad_(True)
    J = buckling.bucklingMeasure(rho, obj)
    J.backward()
    assert rho.grad.dtype == dtype and rho.grad.shape == rho.shape and J.dtype == torch.float64
    assert float(J.detach()) == obj.evaluate()
    assert torch.equal(rho.grad.reshape(-1), obj.gradient_device().to(dtype))              # bit for bit
    rho2 = rho.detach().clone().requires_grad_(True)
    (2.5 * buckling.bucklingMeasure(rho2, obj)).backward()
    assert torch.equal(rho2.grad.reshape(-1), (2.5 * obj.gradient_device()).to(dtype))
    J3 = buckling.bucklingMeasure(rho.detach().clone().requires_grad_(True), obj)
    obj.updateCache(None)
    with pytest.raises(RuntimeError, match="updated between forward and backward"):
        J3.backward()


# ---- as a constraint of the MMA optimiser ----

def test_objective_constraint_and_three_mma_steps():
    name = "column2"
    c = bc.case(name)
    sim, compliance = _solved(name)
    obj = buckling.BucklingObjective(compliance, numModes=bc.NUM_MODES, P=bc.P_NORM, tol=TOL_SOLVE)
    J0 = obj.evaluate()
    bound = 1.05 * J0
    cap = mma.ObjectiveConstraint(obj, bound)
    x0 = torch.from_numpy(c[3]).cuda()
    value = cap.evaluate_dev(x0)
    assert value == 1.0 - obj.evaluate() / bound and abs(obj.evaluate() - J0) < FLOOR * J0
    assert torch.equal(cap.backprop_dev(x0), obj.gradient_device() * (-1.0 / bound))
    problem = pv.TopologyOptimizationProblem(sim, compliance, [pv.TotalVolumeConstraint(0.6), cap], [])
    problem.setVars(x0)
    opt = mma.MMAOptimizer(problem, xmin=0.2, xmax=1.0, move=0.1)
    for _ in range(3):
        change = opt.step()
        assert 0.0 < change <= 0.1 * 0.8 + 1e-15
    x = problem.getVars_device()
    value = cap.evaluate_dev(x)                                    # solves at the final densities
    J = obj.evaluate()
    assert value == 1.0 - J / bound and torch.equal(sim.getDensities_device()[:x.numel()], x)
    want = bc.evaluate(c, x.cpu().numpy(), want_gradient=False)["J"]
    print("after three MMA steps: J %.6f (start %.6f, bound %.6f), restatement %.2e" % (J, J0, bound, abs(J - want) / want))
    assert abs(J - want) < TOL_J[name] * want


# ---- refusals ----

def test_refusals():
    q2 = pv.TensorProductSimulator([2, 2], [np.zeros(2), np.ones(2)], [2, 2])
    with pytest.raises(RuntimeError, match="degree-1"):
        buckling.bucklingModes(q2, np.zeros((q2.numNodes(), 2)), 1)
    padded = pv.TensorProductSimulator1_1_1([np.zeros(3), np.ones(3)], [2, 2, 2], _element_padding=(1, 0))
    with pytest.raises(RuntimeError, match="padding"):
        buckling.bucklingModes(padded, np.ones((padded.numNodes(), 3)), 1)
    with pytest.raises(RuntimeError, match="padding"):
        buckling.applyKG(padded, np.ones((padded.numNodes(), 3)), np.ones((padded.numNodes(), 3)))
    free = pv.TensorProductSimulator([1, 1], [np.zeros(2), np.ones(2)], [4, 4])
    with pytest.raises(RuntimeError, match="rigid modes"):
        buckling.bucklingModes(free, np.ones((free.numNodes(), 2)), 1)
    sim, solved = _solved("column2")
    u = solved._u
    for k in (0, 9):
        with pytest.raises(RuntimeError, match="numModes must be 1 to 8"):
            buckling.bucklingModes(sim, u, k)
        with pytest.raises(RuntimeError, match="numModes must be 1 to 8"):
            buckling.BucklingObjective(solved, numModes=k)
    for P in (0.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="P must be finite and at least 1"):
            buckling.BucklingObjective(solved, P=P)
    for q in (0.0, -1.0):
        with pytest.raises(RuntimeError, match="stressExponent must be positive"):
            buckling.BucklingObjective(solved, stressExponent=q)
        with pytest.raises(RuntimeError, match="stressExponent must be positive"):
            buckling.bucklingModes(sim, u, 2, stressExponent=q)
    with pytest.raises(TypeError, match="ComplianceObjective"):
        buckling.BucklingObjective(sim)
    with pytest.raises(RuntimeError, match="numGuard"):
        buckling.bucklingModes(sim, u, 7, numGuard=2)
    with pytest.raises(RuntimeError, match="preconditioner"):
        buckling.bucklingModes(sim, u, 2, preconditioner="jacobi")
    with pytest.raises(RuntimeError, match="displacement is zero"):
        buckling.bucklingModes(sim, torch.zeros_like(u), 2)
    with pytest.raises(RuntimeError, match="Invalid input size"):
        buckling.bucklingModes(sim, u[:-1], 2)
    values = np.zeros((sim.numNodes(), 2))
    values[0, 0] = 0.5
    sim.dirichletValues = values
    with pytest.raises(RuntimeError, match="nonzero Dirichlet"):
        buckling.bucklingModes(sim, u, 2)
    with pytest.raises(RuntimeError, match="nonzero Dirichlet"):
        buckling.BucklingObjective(solved)


def test_a_bar_in_pure_tension_is_refused():
    """a uniform solid bar of 2 x 1 elements with Poisson's ratio 0, pulled by the consistent end load: sigma_xx is constant and
    positive, every other stress is zero, so K_G is sigma_xx times the x-part of the Laplacian: positive definite on the free
    components, no nu is negative.  The block of 6 + 2 columns spans all 8 free components, so the first Rayleigh-Ritz step is exact
    and the block converges at once.  (On a larger grid the positive nu are the end of the spectrum of K^-1 K_G that accumulates at
    zero; the solve then ends with "no convergence", naming a positive nu.)  Pushed, the same bar has its 6 modes."""
    ne, h = (2, 1), 0.25
    for sign in (1.0, -1.0):
        sim = pv.TensorProductSimulator([1, 1], [np.zeros(2), np.array(ne) * h], list(ne))
        sim.ETensor = ElasticityTensor(1.0, 0.0, dim=2)
        sim.E_0, sim.E_min, sim.gamma = bc.E0, bc.EMIN, bc.GAMMA
        sim.setElementDensities(np.ones(2))
        sim.dirichletMask = sc.cantilever(ne)[0]
        sim.setLoads_device(torch.from_numpy(sign * bc.end_load(ne, True)).cuda())
        solved = pv.ComplianceObjective(sim)
        if sign > 0:
            lam, Phi, info = buckling.bucklingModes(sim, solved._u, 6, tol=TOL_SOLVE, numGuard=2)
            assert (lam > 0).all() and info["blockSize"] == 8
            continue
        with pytest.raises(RuntimeError, match=r"6 buckling modes asked for, 0 found: 6 of the 6 lowest nu are not negative"):
            buckling.bucklingModes(sim, solved._u, 6, tol=TOL_SOLVE, numGuard=2)
        with pytest.raises(RuntimeError, match="not negative"):
            buckling.BucklingObjective(solved, numModes=6, tol=TOL_SOLVE, numGuard=2).evaluate()


def test_the_pulled_column_has_the_pushed_column_s_operator_negated():
    """K_G is linear in u, so column2 with the load reversed, which looks like a column in pure tension, has the pushed column's
    spectrum negated: 20 negative nu, the lowest -1.283 (tests/test_buckling_cpu.py pins them), buckling modes of its own at lambda_1 = 0.780
    by lateral compression around the stiff inclusions.  No correct solver refuses it as "not negative"; the refusal is shown on a
    load that compresses nothing (test_a_bar_in_pure_tension_is_refused).  Here: the device operator of -u is minus that of u."""
    sim, solved = _solved("column2")
    pulled_sim, pulled = _solved("column2", reverse=True)
    assert torch.equal(pulled._u, -solved._u)
    X = torch.from_numpy(np.random.default_rng(6).standard_normal((3, sim.numNodes(), 2))).cuda()
    Y = buckling.applyKG_device(sim, solved._u, X)
    assert bool(Y.abs().max() > 0) and torch.equal(buckling.applyKG_device(pulled_sim, pulled._u, X), -Y)


def test_the_c_boundary_refuses_before_any_device_call():
    c = _kernel_case((7, 5))
    lib = _lib.load()
    args, keep = _head(c["ne"], c["h"], c["D"])
    nn = sc.num_nodes(c["ne"])
    X, mG, u, v = _dev(c["X"]), _dev(c["mG"]), _dev(c["u"]), _dev(c["v"])
    Y, a, g = _dev(np.full((3, nn * 2), np.nan)), _dev(np.full(nn * 2, np.nan)), _dev(np.full(35, np.nan))
    s = pv._stream()
    err = lambda: lib.vfem_last_error().decode()
    apply = lambda *t: lib.vfem_buckling_geom_apply(*t, s)
    assert apply(*args, None, _p(u), None, 3, _p(X), _p(Y)) == 1 and "null" in err()
    assert apply(*args, _p(mG), None, None, 3, _p(X), _p(Y)) == 1
    assert apply(*args, _p(mG), _p(u), None, 3, None, _p(Y)) == 1
    assert apply(*args, _p(mG), _p(u), None, 3, _p(X), None) == 1
    assert apply(*args[:3], None, _p(mG), _p(u), None, 3, _p(X), _p(Y)) == 1 and "null" in err()
    for ncols in (0, 25):
        assert apply(*args, _p(mG), _p(u), None, ncols, _p(X), _p(Y)) == 1 and "ncols must be 1 to 24" in err()
    assert apply(*args, _p(mG), _p(u), None, 3, _p(X), _p(X)) == 1 and "aliases X" in err()
    assert apply(*args, _p(mG), _p(u), None, 1, _p(X), _p(u)) == 1 and "aliases u" in err()
    big = _dev(np.ones(3 * nn * 2))                                                    # multipliers in a buffer long enough to be an output
    assert apply(*args, _p(big), _p(u), None, 1, _p(X), _p(big)) == 1 and "aliases the multipliers" in err()
    bits = torch.zeros(8 * 3 * nn * 2, dtype=torch.uint8, device="cuda")              # (long enough to be written as Y, were it not refused)
    assert apply(*args, _p(mG), _p(u), _p(bits), 3, _p(X), _p(bits)) == 1 and "aliases the mask" in err()
    assert apply(4, *args[1:], _p(mG), _p(u), None, 3, _p(X), _p(Y)) == 1 and "dim" in err()
    bad, keep2 = _head((7, 0), c["h"], c["D"])
    assert apply(*bad, _p(mG), _p(u), None, 3, _p(X), _p(Y)) == 1 and "extent" in err()
    bad, keep3 = _head((7, 5), (0.5, 0.0), c["D"])
    assert apply(*bad, _p(mG), _p(u), None, 3, _p(X), _p(Y)) == 1 and "edge lengths" in err()
    bad, keep4 = _head((7, 5), c["h"], np.full((3, 3), np.nan))
    assert apply(*bad, _p(mG), _p(u), None, 3, _p(X), _p(Y)) == 1 and "tensor" in err()
    # the adjoint load
    co = np.ones(8)
    load = lambda *t: lib.vfem_buckling_adjoint_load(*t, s)
    for nmodes in (0, 9):
        assert load(*args, _p(mG), None, nmodes, _dp(co), _p(X), _p(a)) == 1 and "nmodes must be 1 to 8" in err()
    assert load(*args, None, None, 3, _dp(co), _p(X), _p(a)) == 1 and "null" in err()
    assert load(*args, _p(mG), None, 3, None, _p(X), _p(a)) == 1
    assert load(*args, _p(mG), None, 3, _dp(co), None, _p(a)) == 1
    assert load(*args, _p(mG), None, 3, _dp(co), _p(X), None) == 1
    assert load(*args, _p(mG), None, 3, _dp(np.array([1.0, np.inf, 1.0])), _p(X), _p(a)) == 1 and "not finite" in err()
    assert load(*args, _p(mG), None, 3, _dp(co), _p(X), _p(X[1])) == 1 and "aliases" in err()
    assert load(*args, _p(big), None, 3, _dp(co), _p(X), _p(big[10:])) == 1 and "aliases the multipliers" in err()
    assert load(*args, _p(mG), _p(bits), 3, _dp(co), _p(X), _p(bits)) == 1 and "aliases the mask" in err()
    # the gradient
    K0 = np.eye(8)
    grad = lambda *t: lib.vfem_buckling_gradient(*t, s)
    tail = (_p(mG), _p(mG), _p(u), _p(v), _p(X))
    for nmodes in (0, 9):
        assert grad(*args, nmodes, _dp(K0), _dp(co), _dp(co), *tail, _p(g)) == 1 and "nmodes must be 1 to 8" in err()
    assert grad(*args, 2, None, _dp(co), _dp(co), *tail, _p(g)) == 1 and "null" in err()
    assert grad(*args, 2, _dp(K0), None, _dp(co), *tail, _p(g)) == 1
    assert grad(*args, 2, _dp(K0), _dp(co), _dp(co), *tail, None) == 1
    assert grad(*args, 2, _dp(K0), _dp(co), _dp(co), _p(mG), _p(mG), _p(u), None, _p(X), _p(g)) == 1
    assert grad(*args, 2, _dp(np.full((8, 8), np.nan)), _dp(co), _dp(co), *tail, _p(g)) == 1 and "element matrix" in err()
    assert grad(*args, 2, _dp(K0), _dp(np.array([np.nan, 1.0])), _dp(co), *tail, _p(g)) == 1 and "not finite" in err()
    assert grad(*args, 2, _dp(K0), _dp(co), _dp(co), *tail, _p(u)) == 1 and "aliases" in err()
    torch.cuda.synchronize()
    for t in (Y, a, g):
        assert torch.isnan(t).all()
    assert bool((big == 1.0).all()) and not bool(bits.any())
