"""-m gpu: transient heat conduction on the device (ndr_amd.transient, vfem_transient_*): the two-term kernels, the band, the
time-accumulated gradient, the multigrid handle of a step's operator, the direct chain of both objectives, the closed forms, the
multigrid-PCG march, a design loop and the autograd nodes, against tests/transient_cpu.py.

Bounds: the rules of tests/test_gpu_thermal.py and tests/test_gpu_thermal_mg.py.  Every figure named "restatement" was measured on the
CPU with tests/transient_cpu.py (tests/test_transient_cpu.py prints and pins them).
  Kernels (apply, diagonal, band, gradient): the reference is the restatement in np.longdouble; the floor is what the same restatement
    in float64 differs from it, relative to the largest entry; the bound is 16 floors, per case.  Each case runs with the capacity term
    of the size of the conduction term, 1e4 times it and 1e-4 times it.
  Multigrid handle: every level's operator through the probing vectors, 16 floors; V-cycle max(10 floors, 1e-12); PCG count within the
    restatement's pinned count + 2 (10 / 9 / 12 / 10, and 10 / 9 without any fixed node), true residual within tol + 10 gaps, solution
    within 10 times the restatement's own PCG-to-direct difference.
  Direct chain (T, Lam, both objectives, both gradients): 1e-11 of the largest entry.
  Closed forms: ten times the restatement's own errors (decay 3.7e-15 / 3.3e-15 / 3.7e-15, energy balance 6.1e-16 / 3.5e-16), none of
    which is within one rounding.
  Multigrid-PCG march against the direct march (tol 1e-10): ten times the restatement's difference (3.1e-12 / 1.3e-12).

Measured on an MI355X (DESIGN 3.18 has the same figures):
  apply at 1, 3, 8 columns, with and without b, iota 0 and 1, three ratios, 216 cases: 7.6e-17 .. 4.6e-16 of the largest entry against
    floors of 5.7e-17 .. 2.8e-16 (at most 2.7 floors); diagonal at most 1.9 floors, gradient at S = 1, 3, 9 at most 1.7, band 1.9; off-line
    buffers and a second run bit-identical.
  multigrid handle: level operators at most 7.1 floors, sweeps 3.7; V-cycle 5.6e-17 .. 4.8e-16 against floors of 5.7e-17 .. 1.8e-16, symmetry
    at most 3.6e-17; the PCG takes the restatement's counts exactly (10 / 9 / 12 / 10; 10 / 9 without any fixed node) and its solution
    differs from the direct one by what the restatement's does (3.5e-10 .. 3.4e-9); Jacobi-PCG without a sink 56 iterations, as the restatement.
  direct chain (bound 1e-11): at most 3.6e-15 over T, J, Lam, both gradients, J_P and C T0, on 16 x 6 and 8 x 4 x 3, theta 1 and 0.5; one
    factorisation for two objectives with their adjoints.
  closed forms: decay 3.1e-15 / 3.4e-15 / 4.0e-15 (bounds 3.7e-14 / 3.3e-14 / 3.7e-14), energy balance 4.7e-16 .. 9.8e-16 (bounds 6.1e-15 / 3.5e-15).
  multigrid-PCG march: 3.0e-12 / 1.3e-12 of the largest temperature (bounds 3.1e-11 / 1.3e-11), counts 19, 18, 16, 16, 14 / 15, 14, 13, 12, 11 as
    the restatement's, one hierarchy for the march and the adjoint march.
  three MMA steps under a pulse on 32 x 16: J 0.040802 -> 0.040618, J_P 0.480994 -> 0.480711 under 0.505044, constraint 7.8e-16, its gradient
    8.0e-15 of the largest entry, one factorisation per step.
  The whole file runs in 5 s.
  Against the parent commit every test fails at import: the module and the entry points do not exist.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import thermal_cpu as tc
import thermal_mg_cpu as mg
import transient_cpu as tr

pytestmark = pytest.mark.gpu

from ndr_amd import _lib, mma, transient                                            # noqa: E402
from ndr_amd import pyVoxelFEM as pv                                                # noqa: E402
from ndr_amd.thermal import HeatConductionSimulator                                 # noqa: E402
from ndr_amd.transient import (TransientComplianceObjective, TransientHeatSimulator,       # noqa: E402
                               TransientPNormTemperatureObjective)

MARGIN = 16.0
TOL_DIRECT = 1e-11

# the shapes of tests/test_gpu_thermal.py: several workgroups of the cell kernels, 71 nodes along the last axis (the block edge at 64),
# and for the band one tile with padding rows, w < 64 over many tile rows and w > 64
SHAPES = [(7, 5), (40, 37), (5, 70), (6, 4, 5), (12, 10, 9), (3, 3, 70)]
COLUMNS = [1, 3, 8]
RATIOS = [1.0, 1e4, 1e-4]           # the capacity term against the conduction term


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


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


def _head(ne):
    n = np.asarray(ne, dtype=np.int64)
    return (len(ne), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), n          # (the array stays alive)


def _rel(got, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max() / np.abs(ref).max())


def _check(what, ne, got, f64, ref):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    floor, err = _rel(f64, ref), _rel(got, ref)
    print("%s %s: %.2e of the largest entry, floor %.2e (%.1f floors)" % (what, _name(ne), err, floor, err / floor if floor else 0.0))
    assert err <= MARGIN * floor


# ---- the kernels against the restatement in extended precision ----

@functools.lru_cache(maxsize=None)
def _case(ne, ratio=1.0):
    """random fields, the anisotropic conductivity; Ka = 0.7 Kc0 and mb scaled so that the largest capacity entry is `ratio` times
    the largest conduction entry"""
    N = len(ne)
    rng = np.random.default_rng(2200 + int(np.prod(ne)))
    nn, nel = tc.num_nodes(ne), tc.num_elements(ne)
    Kc0 = tc.conductivity_matrix(tc.K_ANISO[N], tc.EDGES[N])
    m = tr.capacity_entries(tc.EDGES[N], lumping=0.25)
    return dict(ne=ne, N=N, Kc0=np.ascontiguousarray(Kc0), m=np.ascontiguousarray(m), Ka=np.ascontiguousarray(0.7 * Kc0),
                mb=np.ascontiguousarray(m * (ratio * np.abs(0.7 * Kc0).max() / m.max())),
                kap=rng.uniform(0.05, 1.0, size=nel), cp=rng.uniform(0.05, 1.0, size=nel), dk=rng.uniform(0.05, 1.0, size=nel),
                dc=rng.uniform(0.05, 1.0, size=nel), fixed=rng.uniform(size=nn) < 0.2, X=rng.standard_normal((10, nn)),
                Z=rng.standard_normal((10, nn)))


def _mask(c):
    return torch.from_numpy(c["fixed"].astype(np.uint8)).cuda()


def _operator(c, off=False):
    """the arguments every operator call takes after the grid (the tensors stay alive with the tuple)"""
    kap, cp, mask = _dev(c["kap"], off), _dev(c["cp"], off), _mask(c)
    return (_dp(c["Ka"]), _dp(c["mb"]), _p(kap), _p(cp), _p(mask)), (kap, cp, mask)


def _run_apply(c, ncols, with_b, identity, off=False):
    args, keep = _head(c["ne"])
    op, alive = _operator(c, off)
    X, out = _dev(c["X"][:ncols], off), _dev(np.full((ncols, c["X"].shape[1]), np.nan), off)
    b = _dev(c["Z"][:ncols], off) if with_b else None
    _lib.check(_lib.load().vfem_transient_apply(*args, *op, identity, ncols, _p(X), _p(b), _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


def _run_diagonal(c, off=False):
    args, keep = _head(c["ne"])
    op, alive = _operator(c, off)
    out = _dev(np.full(c["X"][0].shape, np.nan), off)
    _lib.check(_lib.load().vfem_transient_diagonal(*args, *op, _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


def _run_gradient(c, steps, dt=0.05, theta=0.7, off=False):
    args, keep = _head(c["ne"])
    T, Lam, dk, dc = _dev(c["X"][:steps + 1], off), _dev(c["Z"][:steps + 1], off), _dev(c["dk"], off), _dev(c["dc"], off)
    out = _dev(np.full(c["dk"].shape, np.nan), off)
    _lib.check(_lib.load().vfem_transient_gradient(*args, steps, _dp(c["Kc0"]), _dp(c["mb"]), dt, theta, _p(dk), _p(dc), _p(T), _p(Lam),
                                                   _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("ncols", COLUMNS)
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_apply_kernel_matches_the_restatement(ne, ncols, ratio):
    c = _case(ne, ratio)
    for with_b in (False, True):
        for identity in (1, 0):
            args = (ne, c["Ka"], c["mb"], c["kap"], c["cp"], c["fixed"], c["X"][:ncols], c["Z"][:ncols] if with_b else None, identity)
            got = _run_apply(c, ncols, with_b, identity)
            _check("apply[%d cols, b %d, iota %d, ratio %g]" % (ncols, with_b, identity, ratio), ne, got, tr.apply(*args),
                   tr.apply(*args, dtype=np.longdouble))
            f = torch.from_numpy(c["fixed"]).cuda()
            want = torch.from_numpy(c["X"][:ncols]).cuda()[:, f] if identity else torch.zeros((ncols, int(f.sum())), dtype=torch.float64, device="cuda")
            assert torch.equal(got[:, f], want)                              # a fixed node: iota times its own value, b projected away


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_diagonal_and_gradient_kernels_match_the_restatement(ne, ratio):
    c = _case(ne, ratio)
    args = (ne, c["Ka"], c["mb"], c["kap"], c["cp"], c["fixed"])
    _check("diagonal[ratio %g]" % ratio, ne, _run_diagonal(c), tr.diagonal(*args), tr.diagonal(*args, dtype=np.longdouble))
    for steps in (1, 3, 9):
        args = (ne, c["Kc0"], c["mb"], c["dk"], c["dc"], 0.05, 0.7, c["X"][:steps + 1], c["Z"][:steps + 1])
        _check("gradient[S %d, ratio %g]" % (steps, ratio), ne, _run_gradient(c, steps), tr.gradient(*args), tr.gradient(*args, dtype=np.longdouble))


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_kernels_off_line_and_bit_identical_run_to_run(ne):
    """every kernel on buffers 8 bytes off a 16-byte line, and a second run: the same bits as the first"""
    c = _case(ne)
    runs = {"apply": lambda **kw: _run_apply(c, 3, True, 0, **kw), "diagonal": lambda **kw: _run_diagonal(c, **kw),
            "gradient": lambda **kw: _run_gradient(c, 3, **kw)}
    for name, run in runs.items():
        first = run()
        assert not bool(torch.isnan(first).any()), name
        assert torch.equal(first, run()), name
        assert torch.equal(first, run(off=True)), name


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_band_assembly_matches_the_dense_operator(ne, ratio):
    c = _case(ne, ratio)
    args, keep = _head(ne)
    op, alive = _operator(c)
    n, w = tc.num_nodes(ne), tc.band_width(ne)
    band = _dev(np.full(tc.band_doubles(n, w), np.nan))
    _lib.check(_lib.load().vfem_transient_band_assemble(*args, *op, _p(band), pv._stream()))
    torch.cuda.synchronize()
    band = band.cpu().numpy()
    Mb = tr.capacity_matrix(c["mb"])
    ref = tr.assemble(ne, c["Ka"], tr.capacity_matrix(c["mb"].astype(np.longdouble)), c["kap"], c["cp"], c["fixed"], dtype=np.longdouble)
    f64 = tr.assemble(ne, c["Ka"], Mb, c["kap"], c["cp"], c["fixed"])
    i, j = np.nonzero(np.tril(np.ones((n, n), dtype=bool)) & ~np.tril(np.ones((n, n), dtype=bool), -w - 1))
    got = band[tc.band_offset(i, j, w)]
    floor, err = _rel(f64[i, j], ref[i, j]), _rel(got, ref[i, j])
    print("band %s ratio %g (n %d, w %d, %d entries): %.2e of the largest entry, floor %.2e" % (_name(ne), ratio, n, w, i.size, err, floor))
    assert err <= MARGIN * floor
    assert np.array_equal(got == 0.0, f64[i, j] == 0.0)                     # the sparsity, and the identity of the fixed nodes
    fixed = np.nonzero(c["fixed"])[0]
    assert np.all(band[tc.band_offset(fixed, fixed, w)] == 1.0)
    if n % 64:                                                              # the padding rows are the identity
        pad = np.arange(n, (n + 63) // 64 * 64)
        assert np.all(band[tc.band_offset(pad, pad, w)] == 1.0)


# ---- the multigrid handle of a step's operator ----

from test_gpu_thermal_mg import Handle as _SteadyHandle                             # noqa: E402


class Handle(_SteadyHandle):
    """a vfem_thermal_mg made by vfem_transient_mg_create, with the arrays it reads kept alive; every other call is the steady handle's"""

    def __init__(self, ne, Ka, mb, kap, cp, fixed, max_coarsenings=-1, off=False):
        self.ne, self.lib = ne, _lib.load()
        self.n = np.asarray(ne, dtype=np.int64)
        self.Ka, self.mb = np.ascontiguousarray(Ka), np.ascontiguousarray(mb)
        self.kap, self.cp = _dev(kap, off), _dev(cp, off)
        self.fixed = torch.from_numpy(np.asarray(fixed).astype(np.uint8)).cuda() if np.any(fixed) else None
        self.h = ctypes.c_void_p()
        _lib.check(self.lib.vfem_transient_mg_create(ctypes.byref(self.h), len(ne), self.n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                     _dp(self.Ka), _dp(self.mb), _p(self.kap), _p(self.cp), _p(self.fixed), max_coarsenings,
                                                     pv._stream()))
        self.levels = self.lib.vfem_thermal_mg_num_levels(self.h)


@functools.lru_cache(maxsize=None)
def _handle(ne, mask="sink"):
    c = tr.mg_case(ne, mask)
    return Handle(ne, c["Ka"], c["mb"], c["kap"], c["cp"], c["fixed"])


@pytest.mark.parametrize("ne", tr.MG_SHAPES, ids=_name)
def test_multigrid_levels_operators_and_vcycle(ne):
    h = _handle(ne)
    H, HL = tr.mg_hierarchy(ne), tr.mg_hierarchy(ne, long=True)
    assert h.levels == len(H.ne) and [h.dims(l) for l in range(h.levels)] == H.ne
    for l in range(h.levels):
        assert np.array_equal(h.level_fixed(l), H.fixed[l].astype(np.uint8))
        probes = mg.probing_vectors(H.ne[l])
        got = np.stack([h.apply(l, v) for v in probes])
        _check("operator level %d" % l, ne, got, np.stack([H.A[l].matvec(v) for v in probes]),
               np.stack([HL.A[l].matvec(v.astype(np.longdouble)) for v in probes]))
        rng = np.random.default_rng(4400 + l)
        x, b = rng.standard_normal(H.A[l].shape[0]), rng.standard_normal(H.A[l].shape[0])
        _check("sweep level %d" % l, ne, h.smooth(l, x, b, 1), H.sweep(l, x, b, True), HL.sweep(l, x, b, True))
    c = tr.mg_case(ne)
    u, v = c["X"], c["B"]
    Mu, Mv = h.vcycle(u, 1), h.vcycle(v, 1)
    ref = HL.vcycle(u.astype(np.longdouble), 1)
    err, floor = _rel(Mu, ref), _rel(H.vcycle(u, 1), ref)
    sym = abs(float(u @ Mv) - float(v @ Mu)) / (np.linalg.norm(u) * np.linalg.norm(Mv))
    print("V-cycle %s: %.2e (floor %.2e), symmetry %.2e" % (_name(ne), err, floor, sym))
    assert err <= max(10 * floor, 1e-12)
    assert sym < 1e-12 and float(u @ Mu) > 0.0
    assert np.array_equal(h.vcycle(u, 1, off=True), Mu) and np.array_equal(h.vcycle(u, 1), Mu)


@pytest.mark.parametrize("key", sorted(tr.MG_PCG_COUNT), ids=lambda k: "%s-%s" % (_name(k[0]), k[1]))
def test_multigrid_pcg_on_the_handle(key):
    """vfem_thermal_mg_pcg on the transient handle; mask "none": no fixed node at all, where the steady operator is singular"""
    ne, mask = key
    c, h = tr.mg_case(ne, mask), _handle(ne, mask)
    xr, info, direct = tr.mg_pcg_solution(ne, mask)
    own = np.abs(xr - direct).max() / np.abs(direct).max()
    b = np.where(c["fixed"], 0.0, c["B"])
    x, its, rel, status, msg = h.pcg(b)
    assert status == 0, msg
    # the true residual through vfem_transient_apply
    args, keep = _head(ne)
    bd, out = _dev(b), torch.empty_like(x)
    _lib.check(_lib.load().vfem_transient_apply(*args, _dp(h.Ka), _dp(h.mb), _p(h.kap), _p(h.cp), _p(h.fixed), 1, 1, _p(x), None, _p(out), pv._stream()))
    true = float((bd - out).norm() / bd.norm())
    sol = np.abs(x.cpu().numpy() - direct).max() / np.abs(direct).max()
    print("multigrid-PCG %s %s: %d iterations (restatement %d), |r|/|b| %.3e, true %.3e (gap of the restatement %.1e), solution %.2e (restatement %.2e)"
          % (_name(ne), mask, its, info["iterations"], rel, true, info["gap"], sol, own))
    assert info["iterations"] == tr.MG_PCG_COUNT[key]
    assert 0 < its <= tr.MG_PCG_COUNT[key] + 2
    assert rel <= 1e-8 and true <= 1e-8 + 10 * info["gap"]
    assert sol <= 10 * own
    x2, its2 = h.pcg(b)[:2]
    assert its2 == its and torch.equal(x2, x)


def test_jacobi_pcg_of_the_two_term_operator():
    """vfem_transient_pcg: the steady loop on the two-term operator; it agrees with the multigrid-PCG solution to the tolerance"""
    ne = (16, 12)
    c, h = tr.mg_case(ne, "none"), _handle(ne, "none")
    direct = tr.mg_pcg_solution(ne, "none")[2]
    args, keep = _head(ne)
    b, x = _dev(c["B"]), _dev(np.zeros(tc.num_nodes(ne)))
    it, rel = ctypes.c_int(-1), ctypes.c_double(-1.0)
    _lib.check(_lib.load().vfem_transient_pcg(*args, _dp(h.Ka), _dp(h.mb), _p(h.kap), _p(h.cp), None, _p(b), _p(x), 1e-10, 2000, ctypes.byref(it),
                                              ctypes.byref(rel), pv._stream()))
    A = tr.mg_hierarchy(ne, "none").A[0].dense()
    xr, info = tc.pcg(A, c["B"], tol=1e-10)
    sol, own = np.abs(x.cpu().numpy() - direct).max() / np.abs(direct).max(), np.abs(xr - direct).max() / np.abs(direct).max()
    print("Jacobi-PCG %s without a sink: %d iterations (restatement %d), |r|/|b| %.3e, solution %.2e (restatement %.2e)" % (_name(ne), it.value, info["iterations"], rel.value, sol, own))
    assert 0 < it.value <= info["iterations"] + tc.CHECK and it.value % tc.CHECK == 0 and rel.value <= 1e-10
    assert sol <= 10 * own


# ---- simulators of the restatement's problems ----

def _simulator(ne, h, k, rho, fixed, nodal=None, volumetric=None):
    sim = HeatConductionSimulator([np.zeros(len(ne)), np.array(ne) * np.array(h)], list(ne))
    sim.conductivity = k
    sim.setElementDensities(rho)
    if np.any(fixed):
        sim.fixedTemperatureMask = fixed
    sim.setHeatSources(nodal=nodal, volumetric=volumetric)
    return sim


def _chain(ne, theta):
    f = tr.chain_fixture(ne, theta)
    heat = _simulator(ne, f["h"], f["k"], f["rho"], f["fixed"], f["nodal"], f["volumetric"])
    sim = TransientHeatSimulator(heat, capacity=f["capacity"], capacityExponent=f["q"], c_min=f["c_min"], lumping=f["lumping"])
    kw = dict(steps=f["steps"], dt=f["dt"], theta=theta, T0=f["T0"], sourceScale=f["s"])
    return f, heat, sim, kw


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("ne", [(16, 6), (8, 4, 3)], ids=_name)
def test_direct_chain_matches_the_restatement(ne, theta):
    f, heat, sim, kw = _chain(ne, theta)
    pr = tr.chain_problem(f)
    J, g, Lam = pr.compliance()
    JP, gP, LamP, top, step = pr.pnorm(8.0)
    work = TransientComplianceObjective(sim, **kw)
    assert sim.numDirectFactorizations() == 1
    rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    errs = dict(T=rel(work.trajectory(), pr.T), J=abs(work.evaluate() - J) / abs(J), Lam=rel(work.adjoint_device().cpu().numpy(), Lam),
                g=rel(work.gradient(), g))
    assert sim.numDirectFactorizations() == 1                              # the march and the adjoint march: one factorisation
    peak = TransientPNormTemperatureObjective(sim, P=8.0, **kw)
    errs.update(JP=abs(peak.evaluate() - JP) / JP, LamP=rel(peak.adjoint_device().cpu().numpy(), LamP), gP=rel(peak.gradient(), gP),
                c=rel(sim.elementCapacities()[0], pr.cp), dc=rel(sim.elementCapacities()[1], pr.dcp),
                C=rel(sim.applyC(f["T0"]), tr.assemble(ne, 0 * pr.Kc0, tr.capacity_matrix(pr.m), pr.kap, pr.cp, f["fixed"], 0) @ f["T0"]))
    print("direct chain %s theta %.1f: %s" % (_name(ne), theta, " ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < TOL_DIRECT
    assert sim.numDirectFactorizations() == 1                              # a second objective at the same design and scheme: none
    assert peak.maxTemperature()[1] == step and abs(peak.maxTemperature()[0] - top) < TOL_DIRECT * top <= peak.evaluate()
    # unchanged densities: no factorisation, but a new trajectory; other densities, another step or another capacity: one each
    u = work._u
    work.updateCache(torch.from_numpy(f["rho"]).cuda())
    assert sim.numDirectFactorizations() == 1 and work._u is not u and torch.equal(work._u, u)
    work.updateCache(torch.from_numpy(0.9 * f["rho"]).cuda())
    assert sim.numDirectFactorizations() == 2
    assert abs(work.evaluate() - tr.chain_problem(f, 0.9 * f["rho"]).compliance()[0]) < TOL_DIRECT * abs(J) * 2
    sim.march_device(2, 0.5 * f["dt"], theta)
    assert sim.numDirectFactorizations() == 3
    sim.lumping = 1.0
    sim.march_device(2, 0.5 * f["dt"], theta)
    assert sim.numDirectFactorizations() == 4
    heat.exponent = 2.0
    sim.march_device(2, 0.5 * f["dt"], theta)
    assert sim.numDirectFactorizations() == 5


# ---- the closed forms on the device ----

@pytest.mark.parametrize("theta,lumping", tr.DECAY_CASES)
def test_decay_of_a_discrete_mode_on_the_device(theta, lumping):
    pr, exact = tr.decay_case(theta, lumping)
    heat = _simulator(pr.ne, pr.h, 1.0, np.ones(16), pr.fixed)
    sim = TransientHeatSimulator(heat, lumping=lumping)
    T = sim.march(3, pr.dt, theta, T0=np.sin(np.pi * tc.node_coordinates(pr.ne, pr.h)[:, 0]))
    err, bound = np.abs(T[3] - exact).max() / np.abs(exact).max(), tc.analytic_bound(tr.DECAY_MEASURED[(theta, lumping)], pr.ne)
    print("decay on the device theta %.1f lumping %.0f: %.2e (bound %.2e)" % (theta, lumping, err, bound))
    assert err < bound and np.all(T[:, pr.fixed] == 0.0)


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("ne", tr.ENERGY_SHAPES, ids=_name)
def test_energy_balance_without_a_sink_on_the_device(ne, theta):
    f = tr.energy_case(ne, theta)
    heat = _simulator(ne, f["h"], f["k"], f["rho"], f["fixed"], volumetric=f["q"])
    sim = TransientHeatSimulator(heat)
    T = sim.march(f["steps"], f["dt"], theta, T0=f["T0"])
    Q = tc.load(ne, f["h"], None, volumetric=f["q"])
    C = tr.assemble(ne, np.zeros((2 ** len(ne),) * 2), tr.capacity_matrix(tr.capacity_entries(f["h"])), tc.kappa(f["rho"]), tr.cap(f["rho"]), None)
    err, bound = tr.energy_error(ne, C, T, Q, f["dt"]), tc.analytic_bound(tr.ENERGY_MEASURED[ne], ne)
    print("energy balance on the device %s theta %.1f: %.2e (bound %.2e)" % (_name(ne), theta, err, bound))
    assert err < bound and sim.numDirectFactorizations() == 1


# ---- the multigrid-PCG march against the direct march ----

@pytest.mark.parametrize("ne", tr.MARCH_SHAPES, ids=_name)
def test_multigrid_pcg_march_against_the_direct_march(ne):
    f = tr.march_fixture(ne)
    heat = _simulator(ne, f["h"], 1.0, f["rho"], f["fixed"], volumetric=1.0)
    sim = TransientHeatSimulator(heat)
    Td = sim.march_device(f["steps"], f["dt"], f["theta"])
    peak = TransientPNormTemperatureObjective(sim, f["steps"], f["dt"], f["theta"], solver="pcg", preconditioner="multigrid", skipSolve=True)
    peak.tol = 1e-10
    peak.updateCache(None)
    Tp, counts = peak._u, peak.iterations
    err, bound = float((Tp - Td).abs().max() / Td.abs().max()), 10 * tr.MARCH_MEASURED[ne]
    ref = tr.march_both(ne)[0]
    print("multigrid-PCG march %s: counts %s (restatement %s), %.2e of the largest temperature (bound %.2e); direct march against the restatement %.2e"
          % (_name(ne), counts, tr.MARCH_COUNTS[ne], err, bound, np.abs(Td.cpu().numpy() - ref).max() / np.abs(ref).max()))
    assert err <= bound
    assert max(counts[1:]) <= counts[0]                                     # warm starts: no step takes more than the cold first one
    g = peak.gradient_device()
    assert sim.numMultigridBuilds() == 1 and bool(torch.isfinite(g).all())  # the march and the adjoint march: one hierarchy
    assert all(n > 0 for n in sim.last_adjoint_iterations)


def test_jacobi_pcg_march_against_the_direct_march():
    """the march through vfem_transient_pcg: within ten times the restatement's difference from the direct march (1.9e-12), every count
    at most one look interval past where the restatement's loop stops (88, 88, 80, 80, 72)"""
    ne = (16, 12)
    f = tr.march_fixture(ne)
    heat = _simulator(ne, f["h"], 1.0, f["rho"], f["fixed"], volumetric=1.0)
    sim = TransientHeatSimulator(heat)
    Td = sim.march_device(f["steps"], f["dt"], f["theta"])
    Tj = sim.march_device(f["steps"], f["dt"], f["theta"], solver="pcg", tol=1e-10)
    counts, err = sim.last_iterations, float((Tj - Td).abs().max() / Td.abs().max())
    print("Jacobi-PCG march %s: counts %s (restatement %s), %.2e of the largest temperature (bound %.2e)"
          % (_name(ne), counts, tr.MARCH_JACOBI_COUNTS[ne], err, 10 * tr.MARCH_JACOBI_MEASURED[ne]))
    assert err <= 10 * tr.MARCH_JACOBI_MEASURED[ne]
    assert all(0 < got <= want + tc.CHECK and got % tc.CHECK == 0 for got, want in zip(counts, tr.MARCH_JACOBI_COUNTS[ne]))
    assert sim.numDirectFactorizations() == 1 and sim.numMultigridBuilds() == 0


# ---- a design loop ----

def test_three_mma_steps_with_a_cap_on_the_peak_temperature_of_a_pulse():
    n = (32, 16)
    heat = HeatConductionSimulator([[0, 0], [2, 1]], list(n))
    assert heat.fixTemperatureInBox([0.0, 0.4], [0.0, 0.6]) > 0
    heat.setHeatSources(volumetric=1.0)
    sim = TransientHeatSimulator(heat, capacity=2.0)
    pulse = np.where(np.arange(7) <= 3, 1.0, 0.2)
    kw = dict(steps=6, dt=0.05, theta=0.5, sourceScale=pulse)
    peak = TransientPNormTemperatureObjective(sim, P=8.0, skipSolve=True, **kw)
    work = TransientComplianceObjective(sim, skipSolve=True, **kw)
    x0 = torch.full((heat.numElements(),), 0.5, dtype=torch.float64, device="cuda")
    start = peak.evaluate(x0)
    cap = mma.ObjectiveConstraint(peak, 1.05 * start)
    smooth = pv.SmoothingFilter()
    smooth.radius = 1
    problem = pv.TopologyOptimizationProblem(heat, work, [pv.TotalVolumeConstraint(0.5), cap], [smooth])
    problem.setVars(x0)
    opt = mma.MMAOptimizer(problem, xmin=0.05, xmax=1.0, move=0.1)
    problem.evaluateConstraints()
    n0 = sim.numDirectFactorizations()
    J = [problem.evaluateObjective()]
    for step in range(3):
        opt.step()
        values = problem.evaluateConstraints()
        J.append(problem.evaluateObjective())
        assert sim.numDirectFactorizations() - n0 == step + 1              # one factorisation per step, for both objectives
    xPhys = problem._cached[-1]
    assert torch.equal(heat.getDensities_device(), xPhys)
    pr = tr.Problem(n, tuple(heat._h), 1.0, xPhys.cpu().numpy(), heat.fixedTemperatureMask, tc.load(n, tuple(heat._h), heat.fixedTemperatureMask, volumetric=1.0),
                    6, 0.05, 0.5, None, pulse, capacity=2.0)
    JP, gP = pr.pnorm(8.0)[:2]
    got = cap.backprop_dev(xPhys).cpu().numpy()
    errs = abs(values[1] - (1.0 - JP / cap.upperBound)), np.abs(got - (-gP / cap.upperBound)).max() / np.abs(gP / cap.upperBound).max()
    print("three MMA steps under a pulse: J %s, J_P %.6f -> %.6f under %.6f, constraint %.2e, its gradient %.2e of the largest entry"
          % (" -> ".join("%.6f" % v for v in J), start, peak.evaluate(), cap.upperBound, errs[0], errs[1]))
    assert errs[0] < TOL_DIRECT and errs[1] < TOL_DIRECT
    assert abs(J[-1] - pr.compliance()[0]) < TOL_DIRECT * abs(J[-1])
    assert sim.numDirectFactorizations() - n0 == 3


# ---- the autograd nodes and the refusals ----

@pytest.mark.parametrize("which", ["compliance", "peak"])
def test_autograd_nodes_return_the_objectives_gradient_bit_for_bit(which):
    f, heat, sim, kw = _chain((16, 6), 0.5)
    if which == "compliance":
        target, node = TransientComplianceObjective(sim, skipSolve=True, **kw), transient.transientCompliance
    else:
        target, node = TransientPNormTemperatureObjective(sim, P=8.0, skipSolve=True, **kw), transient.transientPNormTemperature
    rho = torch.from_numpy(f["rho"]).cuda().requires_grad_(True)
    loss = node(rho, target)
    assert loss.dtype == torch.float64 and float(loss.detach()) == target.evaluate()
    loss.backward()
    assert torch.equal(rho.grad, target.gradient_device())
    rho32 = torch.from_numpy(f["rho"]).cuda().to(torch.float32).reshape(16, 6).requires_grad_(True)
    (3.0 * node(rho32, target)).backward()
    assert rho32.grad.dtype == torch.float32 and rho32.grad.shape == (16, 6)
    assert torch.equal(rho32.grad, (3.0 * target.gradient_device()).to(torch.float32).reshape(16, 6))
    loss = node(rho, target)
    target.updateCache(torch.from_numpy(0.9 * f["rho"]).cuda())
    with pytest.raises(RuntimeError, match="was updated between forward and backward"):
        loss.backward()
    with pytest.raises(TypeError):
        node(rho, sim)


def test_refusals_of_the_c_layer():
    """each before any device call: status 1 and its message"""
    lib = _lib.load()
    c = _case((7, 5))
    args, keep = _head((7, 5))
    op, alive = _operator(c)
    nn = tc.num_nodes((7, 5))
    X, Y, g = _dev(c["X"][:2]), _dev(np.zeros((2, nn))), _dev(np.zeros(35))
    T, dk = _dev(c["X"][:4]), _dev(c["dk"])
    it, rel = ctypes.c_int(0), ctypes.c_double(0.0)
    grad = lambda steps=3, dt=0.1, theta=1.0, K=c["Kc0"], m=c["m"], out=g: lib.vfem_transient_gradient(
        *args, steps, _dp(K), _dp(m), dt, theta, _p(dk), _p(dk), _p(T), _p(T), _p(out), pv._stream())
    bad = np.array(c["mb"])
    bad[1] = np.inf
    badK = np.array(c["Ka"])
    badK[3] = np.nan
    cases = [(lambda: lib.vfem_transient_apply(*args, *op, 1, 2, None, None, _p(Y), pv._stream()), "vfem_transient_apply: null argument"),
             (lambda: lib.vfem_transient_apply(*args, op[0], op[1], op[2], None, op[4], 1, 2, _p(X), None, _p(Y), pv._stream()), "vfem_transient_apply: null argument"),
             (lambda: lib.vfem_transient_apply(*args, op[0], _dp(bad), *op[2:], 1, 2, _p(X), None, _p(Y), pv._stream()), "the capacity entries are not finite"),
             (lambda: lib.vfem_transient_apply(*args, _dp(badK), *op[1:], 1, 2, _p(X), None, _p(Y), pv._stream()), "the element matrix is not finite"),
             (lambda: lib.vfem_transient_apply(*args, *op, 2, 2, _p(X), None, _p(Y), pv._stream()), "identity must be 0 or 1"),
             (lambda: lib.vfem_transient_apply(*args, *op, 1, 9, _p(X), None, _p(Y), pv._stream()), "ncols must be 1 to 8"),
             (lambda: lib.vfem_transient_apply(*args, *op, 1, 2, _p(X), None, _p(X), pv._stream()), "Y aliases X"),
             (lambda: lib.vfem_transient_apply(*args, *op, 1, 2, _p(X), _p(Y), _p(Y), pv._stream()), "Y aliases b"),
             (lambda: lib.vfem_transient_apply(3 + 1, *args[1:], *op, 1, 2, _p(X), None, _p(Y), pv._stream()), "dim must be 2 or 3"),
             (lambda: lib.vfem_transient_diagonal(*args, *op, None, pv._stream()), "vfem_transient_diagonal: null argument"),
             (lambda: lib.vfem_transient_band_assemble(*args, *op, None, pv._stream()), "vfem_transient_band_assemble: null argument"),
             (lambda: lib.vfem_transient_pcg(*args, *op, _p(X), _p(Y), 0.0, 10, ctypes.byref(it), ctypes.byref(rel), pv._stream()), "tol must be positive"),
             (lambda: lib.vfem_transient_pcg(*args, *op, _p(X), _p(X), 1e-8, 10, ctypes.byref(it), ctypes.byref(rel), pv._stream()), "x aliases b"),
             (lambda: lib.vfem_transient_mg_create(None, *args, *op, -1, pv._stream()), "vfem_transient_mg_create: null argument"),
             (lambda: grad(steps=0), "steps must be at least 1"),
             (lambda: grad(dt=0.0), "dt must be positive"),
             (lambda: grad(dt=float("nan")), "dt must be positive"),
             (lambda: grad(theta=0.4), r"theta must be in \[0.5, 1\]"),
             (lambda: grad(theta=1.1), r"theta must be in \[0.5, 1\]"),
             (lambda: grad(m=bad), "the capacity entries are not finite"),
             (lambda: grad(K=badK), "the element matrix is not finite"),
             (lambda: grad(out=dk), "g aliases an input")]
    import re
    for call, message in cases:
        assert call() == 1
        assert re.search(message, lib.vfem_last_error().decode()), (message, lib.vfem_last_error().decode())
    h = ctypes.c_void_p()
    assert lib.vfem_transient_mg_create(ctypes.byref(h), *args, op[0], op[1], op[2], None, op[4], -1, pv._stream()) == 1 and not h.value


def test_refusals_of_the_python_layer():
    f, heat, sim, kw = _chain((16, 6), 1.0)
    with pytest.raises(TypeError):
        TransientHeatSimulator(sim)
    for name, value, message in (("capacity", 0.0, "capacity must be positive"), ("capacityExponent", 0.5, "at least 1"),
                                 ("c_min", 1.0, r"c_min must be in \[0, 1\)"), ("lumping", 1.5, r"lumping must be in \[0, 1\]")):
        with pytest.raises(RuntimeError, match=message):
            setattr(sim, name, value)
    with pytest.raises(RuntimeError, match=r"theta must be in \[0.5, 1\]"):
        sim.march_device(3, 0.1, theta=0.3)
    with pytest.raises(RuntimeError, match="dt must be positive"):
        sim.march_device(3, -1.0)
    with pytest.raises(RuntimeError, match="steps must be at least 1"):
        sim.march_device(0, 0.1)
    with pytest.raises(RuntimeError, match="sourceScale holds steps \\+ 1 = 4"):
        sim.march_device(3, 0.1, sourceScale=np.ones(3))
    with pytest.raises(RuntimeError, match="solver is"):
        sim.march_device(3, 0.1, solver="multigrid")
    with pytest.raises(RuntimeError, match="a preconditioner goes with"):
        sim.march_device(3, 0.1, preconditioner="multigrid")
    with pytest.raises(RuntimeError, match="march_device has not been called"):
        sim.adjointMarch_device(torch.zeros((4, heat.numNodes()), dtype=torch.float64, device="cuda"))
    sim.march_device(3, 0.1)
    heat.setUniformDensities(0.5)
    with pytest.raises(RuntimeError, match="the simulator changed since the march"):
        sim.adjointMarch_device(torch.zeros((4, heat.numNodes()), dtype=torch.float64, device="cuda"))
    with pytest.raises(TypeError):
        TransientComplianceObjective(heat, 3, 0.1)
    with pytest.raises(RuntimeError, match="P must be finite and at least 1"):
        TransientPNormTemperatureObjective(sim, 3, 0.1, P=0.5)
    with pytest.raises(RuntimeError, match="updateCache\\(xPhys\\) has not been called"):
        TransientComplianceObjective(sim, 3, 0.1, skipSolve=True).evaluate()
