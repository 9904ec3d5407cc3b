"""GPU: the multigrid-preconditioned CG of the scalar conduction operator (``vfem_thermal_mg_*``, ``HeatConductionSimulator.pcg_device``
with ``preconditioner="multigrid"``, ``ThermalComplianceObjective(solver="pcg", preconditioner="multigrid")``) against tests/thermal_mg_cpu.py.

Shapes, each the smallest that reaches a distinct path: 16 x 12 (three levels), 12 x 8 x 16 (three levels in 3-D), 12 x 264 (a colour row
of 133 nodes: more than two waves), 4 x 4 x 136 (69 per colour row: a second wave with 5 lanes; coarse rows of 35), 4 x 4 (a 3 x 3-node
coarsest level), 7 x 5 and 2 x 2 (one level).  Data: random kappa from rho in [0.05, 1], the anisotropic conductivity and the edge
lengths of thermal_cpu, and two masks: the middle-third sink and 20 % random fixed nodes.

Bounds.  One operation: 16 floors, a floor being the float64 restatement against the np.longdouble one on the same data (the rule of
tests/test_gpu_thermal.py), all relative to the largest entry of the reference.  V-cycle: max(10 floors, 1e-12), the rule of
tests/test_gpu_homogenization_mg.py.  PCG: the count within the restatement's pinned count + 2 (the device sums in another order; the
host looks after every iteration, so the count is otherwise exact); the true residual within tol + 10 times the restatement's
recurrence-to-true gap; the solution within 10 times the restatement's own PCG-to-direct difference, relative to max |T|.

Measured on an MI355X: operators at most 3.7 floors, level_apply 5.7, transfers 1.0, sweeps 5.5; V-cycle 2.8e-17 .. 9.9e-14 against floors of
3.8e-17 .. 3.6e-14, symmetry at most 9.6e-17; the PCG takes the restatement's counts exactly (23 / 18, 25 / 20, 12 / 9, 14 / 11; 25 on
128 x 128, 12 on 32 x 32 x 32), its solution differs from the direct one by what the restatement's does (1.2e-11 .. 5.9e-10 of max |T|); the
objective with the multigrid preconditioner against "direct": T 9.1e-8 / 3.6e-7, J 1.9e-9 / 2.7e-9, gradient 4.1e-6 / 7.0e-6; three OC steps end within
2.1e-10 of the direct solver's J.  The whole file runs in 5 s.

Against the parent commit every test fails: the entry points, the ``preconditioner`` arguments and the build counters do not exist there.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import thermal_cpu as tc
import thermal_mg_cpu as mg

pytestmark = pytest.mark.gpu

from ndr_amd import _lib                                                            # noqa: E402
from ndr_amd import pyVoxelFEM as pv                                                # noqa: E402
from ndr_amd.thermal import HeatConductionSimulator, PNormTemperatureObjective, ThermalComplianceObjective      # noqa: E402

MARGIN = 16.0
SHAPES = [(16, 12), (12, 8, 16), (12, 264), (4, 4, 136), (4, 4), (7, 5), (2, 2)]
MASKS = ["sink", "random"]
MULTILEVEL = [ne for ne in SHAPES if len(mg.level_extents(ne)) > 1]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _name(ne):
    return "x".join(map(str, ne))


def _dev(a, off=False):
    """a device copy; off: a view that starts 8 bytes off a 16-byte line"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not off:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    view = buf[1:].reshape(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8
    return view


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max() / np.abs(ref).max())


class Handle:
    """a vfem_thermal_mg with the arrays it reads kept alive"""

    def __init__(self, ne, Kc0, kap, fixed, max_coarsenings=-1, off=False):
        self.ne, self.lib = ne, _lib.load()
        self.n = np.asarray(ne, dtype=np.int64)
        self.Kc0 = np.ascontiguousarray(Kc0)
        self.kap = _dev(kap, off)
        self.fixed = None if fixed is None else torch.from_numpy(np.asarray(fixed).astype(np.uint8)).cuda()
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.vfem_thermal_mg_create(ctypes.byref(self.h), len(ne), self.n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                   _dp(self.Kc0), _p(self.kap), _p(self.fixed), max_coarsenings, pv._stream()))
        self.levels = self.lib.vfem_thermal_mg_num_levels(self.h)

    def close(self):
        if self.h:
            self.lib.vfem_thermal_mg_destroy(self.h)
            self.h = None

    def dims(self, l):
        n = np.zeros(len(self.ne), dtype=np.int64)
        _lib.check(self.lib.vfem_thermal_mg_level_dims(self.h, l, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return tuple(int(v) for v in n)

    def nodes(self, l):
        return tc.num_nodes(self.dims(l))

    def level_fixed(self, l):
        out = torch.full((self.nodes(l),), 7, dtype=torch.uint8, device="cuda")
        _lib.check(self.lib.vfem_thermal_mg_level_fixed(self.h, l, _p(out), pv._stream()))
        return out.cpu().numpy()

    def apply(self, l, X):
        X, Y = _dev(X), _dev(np.full(self.nodes(l), np.nan))
        _lib.check(self.lib.vfem_thermal_mg_level_apply(self.h, l, _p(X), _p(Y), pv._stream()))
        return Y.cpu().numpy()

    def smooth(self, l, X, B, forward):
        X, B = _dev(X), _dev(B)
        _lib.check(self.lib.vfem_thermal_mg_smooth(self.h, l, _p(X), _p(B), int(forward), pv._stream()))
        return X.cpu().numpy()

    def restrict(self, l, fine):
        fine, coarse = _dev(fine), _dev(np.full(self.nodes(l + 1), np.nan))
        _lib.check(self.lib.vfem_thermal_mg_restrict(self.h, l, _p(fine), _p(coarse), pv._stream()))
        return coarse.cpu().numpy()

    def prolong_add(self, l, coarse, fine):
        coarse, fine = _dev(coarse), _dev(fine)
        _lib.check(self.lib.vfem_thermal_mg_prolong_add(self.h, l, _p(coarse), _p(fine), pv._stream()))
        return fine.cpu().numpy()

    def vcycle(self, B, smoothing, off=False):
        B, X = _dev(B, off), _dev(np.full(self.nodes(0), np.nan), off)
        _lib.check(self.lib.vfem_thermal_mg_vcycle(self.h, _p(B), _p(X), smoothing, pv._stream()))
        return X.cpu().numpy()

    def pcg(self, b, x0=None, tol=1e-8, max_iter=200, smoothing=1, off=False):
        """(x, iterations, relres, status, message)"""
        b = _dev(b, off)
        x = _dev(np.zeros(self.nodes(0)) if x0 is None else x0, off)
        it, rel = ctypes.c_int(-1), ctypes.c_double(-1.0)
        status = self.lib.vfem_thermal_mg_pcg(self.h, _p(b), _p(x), tol, max_iter, smoothing, ctypes.byref(it), ctypes.byref(rel), pv._stream())
        return x, it.value, rel.value, status, self.lib.vfem_last_error().decode() if status else ""


@functools.lru_cache(maxsize=None)
def _handle(ne, mask):
    c = mg.case(ne, mask)
    return Handle(ne, c["Kc0"], c["kap"], c["fixed"])


def _both(ne, mask):
    return mg.case_hierarchy(ne, mask), mg.case_hierarchy(ne, mask, long=True)


def _vectors(H, l, seed):
    rng = np.random.default_rng(4200 + seed + 10 * l)
    n = H.A[l].shape[0]
    return rng.standard_normal(n), rng.standard_normal(n)


def _check(what, got, f64, ref):
    """the device within MARGIN floors of the longdouble reference, the floor being the float64 restatement against it"""
    err, floor = _rel(got, ref), _rel(f64, ref)
    print("%s: %.2e against a floor of %.2e (%.1f floors)" % (what, err, floor, err / floor if floor else 0.0))
    assert err <= MARGIN * floor
    return err, floor


# ---- one operation at a time ----

@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_levels_masks_and_operators(ne, mask):
    """the level extents and masks are the restatement's; every level's operator, read through the 3^N probing vectors (each output
    is one coefficient of the stencil, or of the matrix-free level 0), and its product with a random vector"""
    h = _handle(ne, mask)
    H, HL = _both(ne, mask)
    assert h.levels == len(H.ne) and [h.dims(l) for l in range(h.levels)] == H.ne
    assert int(_lib.load().vfem_thermal_mg_bytes(h.h)) > 0
    for l in range(h.levels):
        assert np.array_equal(h.level_fixed(l), H.fixed[l].astype(np.uint8))
        probes = mg.probing_vectors(H.ne[l])
        got = np.stack([h.apply(l, v) for v in probes])
        _check("operator %s %s level %d" % (_name(ne), mask, l), got, np.stack([H.A[l].matvec(v) for v in probes]),
               np.stack([HL.A[l].matvec(v.astype(np.longdouble)) for v in probes]))
        x = _vectors(H, l, 1)[0]
        got = h.apply(l, x)
        _check("level_apply %s %s level %d" % (_name(ne), mask, l), got, H.A[l].matvec(x), HL.A[l].matvec(x.astype(np.longdouble)))
        assert np.array_equal(got[H.fixed[l]], x[H.fixed[l]])


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("ne", MULTILEVEL, ids=_name)
def test_restrict_and_prolong_add(ne, mask):
    h = _handle(ne, mask)
    H, HL = _both(ne, mask)
    for l in range(h.levels - 1):
        r, xf = _vectors(H, l, 2)
        xc = _vectors(H, l + 1, 3)[0]
        got = h.restrict(l, r)
        _check("restrict %s %s level %d" % (_name(ne), mask, l), got, H.restrict(l, r), HL.restrict(l, r))
        assert np.all(got[H.fixed[l + 1]] == 0.0)
        got = h.prolong_add(l, xc, xf)
        _check("prolong_add %s %s level %d" % (_name(ne), mask, l), got, H.prolong_add(l, xc, xf), HL.prolong_add(l, xc, xf))
        assert np.array_equal(got[H.fixed[l]], xf[H.fixed[l]])              # fixed fine nodes stay untouched
        # the two are transposes of each other: (P xc) . r = xc . (P^T r), to rounding
        a, b = float((got - xf) @ r), float(xc @ h.restrict(l, r))
        assert abs(a - b) <= 1e-13 * np.linalg.norm(got - xf) * np.linalg.norm(r)


@pytest.mark.parametrize("forward", [1, 0], ids=["forward", "backward"])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_one_sweep_on_every_level(ne, mask, forward):
    h = _handle(ne, mask)
    H, HL = _both(ne, mask)
    for l in range(h.levels):
        x, b = _vectors(H, l, 4)
        got = h.smooth(l, x, b, forward)
        _check("sweep %s %s level %d %s" % (_name(ne), mask, l, "forward" if forward else "backward"), got,
               H.sweep(l, x, b, bool(forward)), HL.sweep(l, x, b, bool(forward)))
        # a fixed node gets x = b (to the rounding of x + (b - x))
        f = H.fixed[l]
        assert np.abs(got[f] - b[f]).max(initial=0.0) <= 4 * 2.0 ** -52 * max(np.abs(x).max(), np.abs(b).max())


# ---- the V-cycle ----

@pytest.mark.parametrize("smoothing", [1, 2])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_vcycle_matches_the_restatement_and_is_symmetric(ne, mask, smoothing):
    h = _handle(ne, mask)
    H, HL = _both(ne, mask)
    u, v = _vectors(H, 0, 5)
    Mu, Mv = h.vcycle(u, smoothing), h.vcycle(v, smoothing)
    ref = HL.vcycle(u.astype(np.longdouble), smoothing)
    err, floor = _rel(Mu, ref), _rel(H.vcycle(u, smoothing), ref)
    sym = abs(float(u @ Mv) - float(v @ Mu)) / (np.linalg.norm(u) * np.linalg.norm(Mv))
    print("V-cycle %s %s, %d sweeps: %.2e (floor %.2e), symmetry %.2e" % (_name(ne), mask, smoothing, err, floor, sym))
    assert err <= max(10 * floor, 1e-12)
    assert sym < 1e-12 and float(u @ Mu) > 0.0
    if h.levels == 1:                                                       # the exact inverse, the identity at the fixed nodes
        assert np.array_equal(Mu[H.fixed[0]], u[H.fixed[0]])
    # the same bits from buffers 8 bytes off a 16-byte line, and on a second run
    assert np.array_equal(h.vcycle(u, smoothing, off=True), Mu) and np.array_equal(h.vcycle(u, smoothing), Mu)


# ---- the PCG ----

@functools.lru_cache(maxsize=None)
def _pcg_handle(ne, off=False):
    f = mg.pcg_data(ne)
    return Handle(ne, f["Kc0"], tc.kappa(f["rho"]), f["fixed"], off=off)


def _true_residual(h, b, x):
    f = mg.pcg_data(h.ne)
    out = torch.empty_like(x)
    _lib.check(_lib.load().vfem_thermal_apply(len(h.ne), h.n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(h.Kc0), _p(h.kap), _p(h.fixed),
                                              1, _p(x), _p(out), pv._stream()))
    bd = torch.from_numpy(f["Q"]).cuda()
    return float((bd - out).norm() / bd.norm())


@pytest.mark.parametrize("smoothing", [1, 2])
@pytest.mark.parametrize("ne", mg.PCG_SHAPES, ids=_name)
def test_pcg_on_the_pinned_grids(ne, smoothing):
    f, h = mg.pcg_data(ne), _pcg_handle(ne)
    xr, info = mg.pcg_solution(ne, smoothing)
    T = mg.pcg_direct(ne)
    own = np.abs(xr - T).max() / np.abs(T).max()
    x, its, rel, status, msg = h.pcg(f["Q"], smoothing=smoothing)
    assert status == 0, msg
    true = _true_residual(h, f["Q"], x)
    sol = np.abs(x.cpu().numpy() - T).max() / np.abs(T).max()
    print("multigrid-PCG %s, %d sweeps: %d iterations (restatement %d), |r|/|b| %.3e, true %.3e (gap of the restatement %.1e), solution %.2e of "
          "max |T| (restatement %.2e)" % (_name(ne), smoothing, its, info["iterations"], rel, true, info["gap"], sol, own))
    assert info["iterations"] == mg.PCG_COUNT[smoothing][ne]
    assert 0 < its <= mg.PCG_COUNT[smoothing][ne] + 2
    assert rel <= 1e-8 and true <= 1e-8 + 10 * info["gap"]
    assert sol <= 10 * own
    # two runs give the same bits, and so does a run from buffers 8 bytes off a 16-byte line (the hierarchy's kappa too)
    x2, its2 = h.pcg(f["Q"], smoothing=smoothing)[:2]
    assert its2 == its and torch.equal(x2, x)
    x3, its3 = _pcg_handle(ne, True).pcg(f["Q"], smoothing=smoothing, off=True)[:2]
    assert its3 == its and torch.equal(x3, x)


@pytest.mark.parametrize("ne", [(128, 128), (32, 32, 32)], ids=_name)
def test_iteration_count_does_not_grow_with_the_grid(ne):
    """the restatement's 25 and 12 iterations (20 at 32 x 32, 11 at 16 x 16 x 16); Jacobi-PCG takes 730 and 201"""
    f = mg.pcg_data(ne)
    h = Handle(ne, f["Kc0"], tc.kappa(f["rho"]), f["fixed"])
    try:
        assert [h.dims(l) for l in range(h.levels)] == mg.level_extents(ne)
        x, its, rel, status, msg = h.pcg(f["Q"])
        assert status == 0, msg
        print("multigrid-PCG %s: %d iterations (restatement %d), |r|/|b| %.3e" % (_name(ne), its, mg.GROWTH_COUNT[ne], rel))
        assert 0 < its <= mg.GROWTH_COUNT[ne] + 2 and rel <= 1e-8
    finally:
        h.close()


def test_pcg_status_returns():
    """the failures are status returns of kernels that ran normally"""
    ne = (40, 36)
    f, h = mg.pcg_data(ne), _pcg_handle(ne)
    x, its, rel, status, msg = h.pcg(f["Q"], max_iter=3)
    assert status == 1 and its == 3 and 1e-8 < rel < 10.0
    assert "vfem_thermal_mg_pcg: not converged after 3 iterations: |r|/|b| = " in msg and "(tol 1.000e-08)" in msg
    # a zero right-hand side: the zero solution in no iteration
    x, its, rel, status, msg = h.pcg(np.zeros(tc.num_nodes(ne)), x0=np.ones(tc.num_nodes(ne)))
    assert status == 0 and its == 0 and float(x.abs().max()) == 0.0
    # the void case of tests/test_gpu_thermal.py: no conductivity at all around the free node (4, 4) of a 7 x 5 grid (k_min = 0).  The
    # grid has one level, whose matrix is then singular: the hierarchy reports the breakdown when it factorises it
    rho = np.full((7, 5), 0.5)
    rho[3:5, 3:5] = 0.0
    kap = tc.kappa(rho.reshape(-1), k_min=0.0)
    with pytest.raises(RuntimeError, match=r"vfem_thermal_mg_create: breakdown at the coarsest level of the hierarchy 7x5: .*not positive definite"):
        Handle((7, 5), tc.conductivity_matrix(1.0, (1.0, 1.0)), kap, tc.face_mask((7, 5), 0, 0))
    sim = HeatConductionSimulator([[0, 0], [7, 5]], [7, 5])
    sim.setElementDensities(rho.reshape(-1))
    sim.fixedTemperatureMask = tc.face_mask((7, 5), 0, 0)
    sim.setHeatSources(volumetric=1.0)
    sim.k_min = 0.0
    with pytest.raises(RuntimeError, match="breakdown"):
        sim.pcg_device(sim.buildLoadVector_device(), preconditioner="multigrid")
    assert sim.numMultigridBuilds() == 0
    # the same hole around the odd node (5, 3) of an 8 x 6 grid, which has a coarse level: the hierarchy stands (the coarse operators are
    # positive definite) and the PCG reports the breakdown as the Jacobi-PCG does
    ne = (8, 6)
    rho = np.full(ne, 0.5)
    rho[4:6, 2:4] = 0.0
    h2 = Handle(ne, tc.conductivity_matrix(1.0, (1.0, 1.0)), tc.kappa(rho.reshape(-1), k_min=0.0), tc.face_mask(ne, 0, 0))
    try:
        assert h2.levels == 2
        x, its, rel, status, msg = h2.pcg(tc.load(ne, (1.0, 1.0), tc.face_mask(ne, 0, 0), volumetric=1.0))
        assert status == 1 and its == 1, msg
        assert "vfem_thermal_mg_pcg: breakdown at iteration 1: p . Ap = " in msg and "is not positive (|r|/|b| = " in msg
    finally:
        h2.close()


def test_refusals_that_need_a_handle():
    h = _handle((16, 12), "sink")
    lib, err = h.lib, lambda: h.lib.vfem_last_error().decode()
    n = h.nodes(0)
    X = torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    a, b = X[:n], X[n // 2:n // 2 + n]
    for l in (-1, 3):
        assert lib.vfem_thermal_mg_level_apply(h.h, l, _p(a), _p(X[n:]), None) == 1 and "level %d out of range" % l in err()
        assert lib.vfem_thermal_mg_smooth(h.h, l, _p(a), _p(X[n:]), 1, None) == 1 and "out of range" in err()
        assert lib.vfem_thermal_mg_level_fixed(h.h, l, _p(a), None) == 1 and "out of range" in err()
    for f in (lib.vfem_thermal_mg_restrict, lib.vfem_thermal_mg_prolong_add):
        assert f(h.h, 2, _p(a), _p(X[n:]), None) == 1 and "level 2 out of range" in err()
    assert lib.vfem_thermal_mg_level_apply(h.h, 0, _p(a), _p(b), None) == 1 and "aliases" in err()
    assert lib.vfem_thermal_mg_smooth(h.h, 0, _p(a), _p(b), 1, None) == 1 and "aliases" in err()
    assert lib.vfem_thermal_mg_vcycle(h.h, _p(a), _p(b), 1, None) == 1 and "X aliases B" in err()
    it, rel = ctypes.c_int(0), ctypes.c_double(0.0)
    assert lib.vfem_thermal_mg_pcg(h.h, _p(a), _p(a), 1e-8, 10, 1, ctypes.byref(it), ctypes.byref(rel), None) == 1 and "x aliases b" in err()


def test_a_coarsest_level_that_is_too_large_is_refused():
    """a 96-cube that may not be coarsened: 912 673 nodes at the coarsest level, refused before anything large is allocated"""
    free = torch.cuda.mem_get_info()[0]
    kap = torch.ones(8, dtype=torch.float64, device="cuda")                # never read: the refusal comes first
    n = np.array([96, 96, 96], dtype=np.int64)
    h = ctypes.c_void_p()
    K = np.ascontiguousarray(tc.conductivity_matrix(1.0, (1.0, 1.0, 1.0)))
    status = _lib.load().vfem_thermal_mg_create(ctypes.byref(h), 3, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(K), _p(kap), None, 0,
                                                pv._stream())
    msg = _lib.load().vfem_last_error().decode()
    assert status == 1 and not h.value
    assert "the coarsest level of the hierarchy 96x96x96 has 912673 nodes, above the limit of 40000" in msg
    assert free - torch.cuda.mem_get_info()[0] < (64 << 20)
    # the simulator raises with that message
    sim = HeatConductionSimulator([[0, 0], [1, 1]], [399, 399])
    sim.fixTemperatureInBox([0.0, 0.0], [0.0, 1.0])
    with pytest.raises(RuntimeError, match="the coarsest level of the hierarchy 399x399 has 160000 nodes"):
        sim.pcg_device(torch.ones(sim.numNodes(), dtype=torch.float64, device="cuda"), preconditioner="multigrid")
    with pytest.raises(RuntimeError, match="preconditioner is \"jacobi\" or \"multigrid\""):
        sim.pcg_device(torch.ones(sim.numNodes(), dtype=torch.float64, device="cuda"), preconditioner="ilu")
    with pytest.raises(RuntimeError, match="solver is \"direct\" or \"pcg\""):
        ThermalComplianceObjective(sim, solver="amg", skipSolve=True)
    with pytest.raises(RuntimeError, match="preconditioner is \"jacobi\" or \"multigrid\""):
        ThermalComplianceObjective(sim, solver="pcg", skipSolve=True, preconditioner="ilu")
    with pytest.raises(RuntimeError, match="a preconditioner goes with solver=\"pcg\""):
        ThermalComplianceObjective(sim, solver="direct", skipSolve=True, preconditioner="multigrid")


# ---- Python ----

def _simulator(ne, h, k, rho, fixed, nodal=None, volumetric=None):
    sim = HeatConductionSimulator([np.zeros(len(ne)), np.array(ne) * np.array(h)], list(ne))
    sim.conductivity = k
    sim.setElementDensities(rho)
    sim.fixedTemperatureMask = fixed
    sim.setHeatSources(nodal=nodal, volumetric=volumetric)
    return sim


@pytest.mark.parametrize("ne", [(16, 12), (12, 8, 16)], ids=_name)
def test_objective_with_multigrid_agrees_with_direct(ne):
    """T, J and the gradient of solver="pcg" with preconditioner="multigrid" against solver="direct" on the direct fixture (anisotropic k, both sources).  Bounds as
    tests/test_gpu_thermal.py has them for its PCG path: dT = 10 times the restatement's own PCG-to-direct difference; |dJ| <= |Q|_1 dT;
    and, from g_e = -kappa'_e T_e^T Kc0 T_e, |dg_e| <= 2 kappa'_e sum |Kc0| max |T| dT"""
    f = tc.direct_fixture(ne)
    sims = [_simulator(ne, f["h"], f["k"], f["rho"], f["fixed"], f["nodal"], f["volumetric"]) for _ in range(2)]
    direct = ThermalComplianceObjective(sims[0], solver="direct")
    obj = ThermalComplianceObjective(sims[1], solver="pcg", preconditioner="multigrid")
    assert sims[1].numMultigridBuilds() == 1 and sims[1].numDirectFactorizations() == 0 and obj.iterations > 0
    assert sims[1].multigridLevels() == [list(e) for e in mg.level_extents(ne)] and sims[1].multigridBytes() > 0
    Kc0 = tc.conductivity_matrix(f["k"], f["h"])
    H = mg.Hierarchy(ne, Kc0, tc.kappa(f["rho"]), f["fixed"])
    Q = tc.load(ne, f["h"], f["fixed"], f["nodal"], f["volumetric"])
    xr, info = H.pcg(Q, tol=1e-8)
    Tref = mg.direct_solve(H, Q)
    dT = 10 * np.abs(xr - Tref).max()
    T, Td = obj.temperature(), direct.temperature()
    gb = 2 * tc.dkappa(f["rho"]).max() * np.abs(Kc0).sum() * np.abs(Td).max() * dT
    eT, eJ, eg = np.abs(T - Td).max(), abs(obj.evaluate() - direct.evaluate()), np.abs(obj.gradient() - direct.gradient()).max()
    print("multigrid objective %s: %d iterations (restatement %d), T %.2e (bound %.2e), J %.2e (bound %.2e), gradient %.2e (bound %.2e)"
          % (_name(ne), obj.iterations, info["iterations"], eT, dT, eJ, np.abs(Q).sum() * dT, eg, gb))
    assert obj.iterations <= info["iterations"] + 2
    assert eT <= dT and eJ <= np.abs(Q).sum() * dT and eg <= gb
    # one hierarchy per design, none at unchanged densities (the warm start then takes no iteration)
    rho = torch.from_numpy(f["rho"]).cuda()
    obj.updateCache(rho)
    assert sims[1].numMultigridBuilds() == 1 and obj.iterations == 0
    obj.updateCache((rho * 0.9).contiguous())
    assert sims[1].numMultigridBuilds() == 2 and obj.iterations > 0
    # the adjoint solve of the peak-temperature measure reuses the hierarchy
    peak = PNormTemperatureObjective(obj, P=8.0)
    peak_direct = PNormTemperatureObjective(direct, P=8.0)
    direct.updateCache((rho * 0.9).contiguous())
    JP = peak.evaluate()
    assert sims[1].numMultigridBuilds() == 2 and obj.iterations > 0
    assert abs(JP - peak_direct.evaluate()) <= tc.num_nodes(ne) ** (1.0 / 8.0) * dT
    assert bool(torch.isfinite(peak.gradient_device()).all())
    # a change of the material or of the mask drops it
    sims[1].k_min = 2e-3
    obj.updateCache(None)
    assert sims[1].numMultigridBuilds() == 3
    sims[1].fixedTemperatureMask = f["fixed"] | tc.face_mask(ne, 0, 1)
    obj.updateCache(None)
    assert sims[1].numMultigridBuilds() == 4


def _heated_square(n=16):
    sim = HeatConductionSimulator([[0, 0], [1, 1]], [n, n])
    assert sim.fixTemperatureInBox([0.0, 0.4], [0.0, 0.6]) > 0
    sim.setHeatSources(volumetric=1.0)
    return sim


def test_three_oc_steps_with_multigrid_reach_the_direct_solvers_objective():
    """the loop of tests/test_gpu_thermal.py with both solvers.  A solve to |r| <= tol |Q| leaves J = Q . T off by T . r <= tol |Q| |T|; the
    bound allows ten times that for what three design updates pass on"""
    J = {}
    for solver in ("direct", "multigrid"):
        sim = _heated_square()
        obj = (ThermalComplianceObjective(sim, skipSolve=True) if solver == "direct" else
               ThermalComplianceObjective(sim, solver="pcg", skipSolve=True, preconditioner="multigrid"))
        smooth = pv.SmoothingFilter()
        smooth.radius = 1
        problem = pv.TopologyOptimizationProblem(sim, obj, [pv.TotalVolumeConstraint(0.4)], [smooth])
        problem.setVars(torch.full((sim.numElements(),), 0.4, dtype=torch.float64, device="cuda"))
        J[solver] = [problem.evaluateObjective()]
        opt = pv.OCOptimizer(problem)
        for _ in range(3):
            opt.step()
            J[solver].append(problem.evaluateObjective())
        if solver == "multigrid":
            assert sim.numDirectFactorizations() == 0 and sim.numMultigridBuilds() >= 3
            assert sim.multigridLevels() == [[16, 16], [8, 8], [4, 4], [2, 2]]
            bound = 10 * 1e-8 * float(obj._f.norm() * obj._u.norm())
        else:
            assert sim.numMultigridBuilds() == 0
    diff = abs(J["multigrid"][-1] - J["direct"][-1])
    print("three OC steps: direct %s, multigrid %s, difference %.2e (bound %.2e)" %
          (" -> ".join("%.6f" % v for v in J["direct"]), " -> ".join("%.6f" % v for v in J["multigrid"]), diff, bound))
    assert J["multigrid"][3] < J["multigrid"][2] < J["multigrid"][1] < J["multigrid"][0]
    assert diff <= bound


def test_the_defaults_still_take_the_jacobi_path():
    f = tc.pcg_fixture((40, 37))
    sim = _simulator((40, 37), f["h"], 1.0, f["rho"], f["fixed"], volumetric=1.0)
    Q = sim.buildLoadVector_device()
    x = sim.pcg_device(Q)
    assert sim.last_iterations % tc.CHECK == 0 and 0 < sim.last_iterations <= tc.pcg_iteration_bound((40, 37))
    assert torch.equal(x, sim.pcg_device(Q, None, 1e-8, 2000, "jacobi"))
    obj = ThermalComplianceObjective(sim, solver="pcg")
    assert ThermalComplianceObjective(sim).solver == "direct" and obj.preconditioner == "jacobi"
    assert sim.numMultigridBuilds() == 0 and obj.iterations == sim.last_iterations > 0
    # and on 40 x 36 (40 x 37 has an odd extent: one level) the multigrid reaches the same temperature in a fraction of the iterations
    sim2 = _simulator((40, 36), 1.0 * np.ones(2), 1.0, mg.pcg_data((40, 36))["rho"], mg.pcg_data((40, 36))["fixed"], volumetric=1.0)
    Q2 = sim2.buildLoadVector_device()
    xj = sim2.pcg_device(Q2)
    jac = sim2.last_iterations
    xm = sim2.pcg_device(Q2, preconditioner="multigrid")
    print("40x36: Jacobi-PCG %d iterations, multigrid-PCG %d" % (jac, sim2.last_iterations))
    assert sim2.last_iterations <= mg.PCG_COUNT[1][(40, 36)] + 2 and jac > 4 * sim2.last_iterations
    assert float((xm - xj).abs().max() / xj.abs().max()) < 1e-6 and sim2.numMultigridBuilds() == 1
