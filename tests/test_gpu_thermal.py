"""-m gpu: steady heat conduction on the device (ndr_amd.thermal, vfem_thermal_*): the element-wise kernels, the band assembly, the
direct chain of both objectives, the closed forms, the Jacobi-PCG with its status returns, the design loops and the autograd nodes,
against tests/thermal_cpu.py.

Bounds.  Every figure named "restatement" was measured on the CPU with tests/thermal_cpu.py (tests/test_thermal_cpu.py prints them).
  Kernels (apply, diagonal, source, gradient, flux) and the band: the reference is the restatement evaluated in np.longdouble; the
    rounding floor of the formula is what the same restatement in float64 differs from it, relative to the largest entry, and the
    bound is 16 times that floor (another summation order), computed per case and printed with it.
  Direct chain (T, J, J_P, both gradients, the flux): 1e-11 of the largest entry, the bound tests/test_gpu_buckling.py and
    tests/test_gpu_loadcases.py use for their direct chains.
  Closed forms: ten times the restatement's own errors (thermal_cpu.SLAB_MEASURED / LAYERS_MEASURED: slab 1.7e-13 / 1.4e-14, layers
    6.0e-13 / 1.6e-15 on 16 x 6 / 6 x 4 x 3), or nodes x 2^-52 where such a figure is no more than one rounding (none of the four is).
  PCG (40 x 37 and 12 x 10 x 9, tol 1e-8, max_iter 2000): the restatement's recurrence residual first meets the tolerance at
    iteration 234 / 71 and its loop, looking every 8 iterations, stops at 240 / 72; the device may stop one look later: at most 248 /
    80.  The true residual, recomputed with vfem_thermal_apply, is at most tol + 10 x 2.8e-13 (the restatement's recurrence-to-true
    gap); the solution lies within 10 x 5.2e-11 / 3.5e-10 of max |T| of the dense solution (what the restatement's PCG solution
    differs from it).

Measured on an MI355X (DESIGN 3.16 has the same figures):
  apply at 1, 3, 8 columns, 18 cases: 9.4e-17 .. 5.5e-16 of the largest entry against floors of 8.9e-17 .. 1.9e-16 (at most 5.1 floors);
    gradient at 1, 3, 8 column pairs, two blocks and one, 36 cases: 8.1e-17 .. 3.3e-16 against 1.5e-16 .. 8.3e-16 (at most 1.5 floors);
    diagonal at most 2.4 floors, source 1.3 floors (a nodal source alone is a copy: floor and error 0), flux 1.0 floor; in place,
    off-line buffers and a second run bit-identical.
  band, 6 grids (356 .. 342 006 entries): 9.2e-17 .. 2.3e-16 against floors of 1.3e-16 .. 1.8e-16 (at most 1.3 floors).
  direct chain (bound 1e-11): 16 x 6 T 7.3e-14, J 7.2e-14, gradient 1.4e-13, J_P 7.5e-14, lambda 6.4e-14, its gradient 1.5e-13, flux
    6.6e-14; 8 x 4 x 3 T 4.2e-15, J 1.9e-14, gradient 3.7e-14, J_P 3.3e-15, lambda 6.2e-16, its gradient 9.7e-16, flux 1.7e-14.
  closed forms: slab 8.3e-14 / 2.2e-15 (bounds 1.7e-12 / 1.4e-13), layers 6.0e-13 / 1.0e-15 (bounds 6.0e-12 / 1.6e-14).
  PCG: 240 / 72 iterations (bounds 248 / 80), |r|/|b| 2.971e-9 / 6.356e-9, true 2.972e-9 / 6.356e-9, solution 4.2e-11 / 2.9e-10 of
    max |T| (bounds 5.2e-10 / 3.5e-9); 0 iterations on the second update; a second run the same bits.
  three OC steps on the heated square: J 12.206 -> 5.065 -> 3.352 -> 2.810, the restatement at the final densities within 2.7e-15; three
    MMA steps with a temperature cap: J_P 13.92 -> 15.31 under 15.31, constraint 1.5e-14, its gradient 3.5e-14 of the largest entry,
    multipliers 58.2 (volume), 1.43 (temperature), one thermal factorisation per step.
  The whole file runs in 4 s.
  Against the parent commit every test fails at import: the module and the entry points do not exist.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import thermal_cpu as tc

pytestmark = pytest.mark.gpu

from ndr_amd import _lib, mma, thermal                                              # noqa: E402
from ndr_amd import pyVoxelFEM as pv                                                # noqa: E402
from ndr_amd.thermal import HeatConductionSimulator, PNormTemperatureObjective, ThermalComplianceObjective      # noqa: E402

MARGIN = 16.0
TOL_DIRECT = 1e-11

# 40 x 37 and 12 x 10 x 9 span several workgroups of the cell kernels (64 lanes along the last axis by 4 rows, one block per layer of
# axis 0 in 3-D); 5 x 70 and 3 x 3 x 70 have 71 nodes along the last axis and so cross the block edge at 64.  The band assembly meets
# one tile with padding rows (7 x 5: n = 48), w < 64 over many tile rows (40 x 37: n = 1558, w = 39) and w > 64 (5 x 70: 72, 12 x 10 x 9:
# 121, 3 x 3 x 70: 356)
SHAPES = [(7, 5), (40, 37), (5, 70), (6, 4, 5), (12, 10, 9), (3, 3, 70)]
COLUMNS = [1, 3, 8]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


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


def _head(ne):
    n = np.asarray(ne, dtype=np.int64)
    return (len(ne), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), n          # (the array stays alive)


def _rel(got, ref):
    """the largest difference relative to the largest entry of the (longdouble) reference"""
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max() / np.abs(ref).max())


# ---- the element-wise kernels against the restatement in extended precision ----

@functools.lru_cache(maxsize=None)
def _case(ne):
    N = len(ne)
    rng = np.random.default_rng(1600 + int(np.prod(ne)))
    nn, nel = tc.num_nodes(ne), tc.num_elements(ne)
    return dict(ne=ne, N=N, h=np.array(tc.EDGES[N]), k=tc.K_ANISO[N], Kc0=np.ascontiguousarray(tc.conductivity_matrix(tc.K_ANISO[N], tc.EDGES[N])),
                kap=rng.uniform(0.05, 1.0, size=nel), dk=rng.uniform(0.05, 1.0, size=nel), q=rng.standard_normal(nel),
                fixed=rng.uniform(size=nn) < 0.2, X=rng.standard_normal((8, nn)), Z=rng.standard_normal((8, nn)), c=rng.standard_normal(8))


def _mask(c):
    return torch.from_numpy(c["fixed"].astype(np.uint8)).cuda()


def _run_apply(c, ncols, off=False):
    args, keep = _head(c["ne"])
    mask = _mask(c)
    X, kap, out = _dev(c["X"][:ncols], off), _dev(c["kap"], off), _dev(np.full((ncols, c["X"].shape[1]), np.nan), off)
    _lib.check(_lib.load().vfem_thermal_apply(*args, _dp(c["Kc0"]), _p(kap), _p(mask), ncols, _p(X), _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


def _run_gradient(c, ncols, off=False, same=False):
    args, keep = _head(c["ne"])
    A, dk, out = _dev(c["X"][:ncols], off), _dev(c["dk"], off), _dev(np.full(c["dk"].shape, np.nan), off)
    B = A if same else _dev(c["Z"][:ncols], off)
    co = np.ascontiguousarray(c["c"][:ncols])
    _lib.check(_lib.load().vfem_thermal_gradient(*args, ncols, _dp(c["Kc0"]), _dp(co), _p(dk), _p(A), _p(B), _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


def _run_source(c, with_q, with_f, off=False, in_place=False):
    args, keep = _head(c["ne"])
    mask = _mask(c)
    q = _dev(c["q"], off) if with_q else None
    f_in = _dev(c["X"][0], off) if with_f else None
    out = f_in if in_place else _dev(np.full(c["X"][0].shape, np.nan), off)
    _lib.check(_lib.load().vfem_thermal_source(*args, _dp(c["h"]), _p(q), _p(mask), _p(f_in), _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


def _run_diagonal(c, off=False):
    args, keep = _head(c["ne"])
    mask = _mask(c)
    kap, out = _dev(c["kap"], off), _dev(np.full(c["X"][0].shape, np.nan), off)
    _lib.check(_lib.load().vfem_thermal_diagonal(*args, _dp(c["Kc0"]), _p(kap), _p(mask), _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


def _run_flux(c, off=False):
    args, keep = _head(c["ne"])
    kap, T, out = _dev(c["kap"], off), _dev(c["X"][0], off), _dev(np.full((c["kap"].size, c["N"]), np.nan), off)
    k = np.ascontiguousarray(c["k"])
    _lib.check(_lib.load().vfem_thermal_flux(*args, _dp(c["h"]), _dp(k), _p(kap), _p(T), _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


def _check(what, ne, got, f64, ref):
    floor, err = _rel(f64, ref), _rel(got.cpu().numpy(), ref)
    print("%s %s: %.2e of the largest entry, floor %.2e (%.1f floors)" % (what, _name(ne), err, floor, err / floor if floor else 0.0))
    assert err <= MARGIN * floor                    # (a copy has no rounding: floor and error are both 0)


@pytest.mark.parametrize("ncols", COLUMNS)
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_apply_kernel_matches_the_restatement(ne, ncols):
    c = _case(ne)
    args = (ne, c["Kc0"], c["kap"], c["fixed"], c["X"][:ncols])
    _check("apply[%d]" % ncols, ne, _run_apply(c, ncols), tc.apply(*args), tc.apply(*args, dtype=np.longdouble))


@pytest.mark.parametrize("same", [False, True], ids=["two-blocks", "one-block"])
@pytest.mark.parametrize("ncols", COLUMNS)
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_gradient_kernel_matches_the_restatement(ne, ncols, same):
    c = _case(ne)
    args = (ne, c["Kc0"], c["dk"], c["c"][:ncols], c["X"][:ncols], c["X"][:ncols] if same else c["Z"][:ncols])
    _check("gradient[%d]" % ncols, ne, _run_gradient(c, ncols, same=same), tc.gradient(*args), tc.gradient(*args, dtype=np.longdouble))


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_diagonal_source_and_flux_kernels_match_the_restatement(ne):
    c = _case(ne)
    args = (ne, c["Kc0"], c["kap"], c["fixed"])
    _check("diagonal", ne, _run_diagonal(c), tc.diagonal(*args), tc.diagonal(*args, dtype=np.longdouble))
    for with_q, with_f in ((True, False), (False, True), (True, True)):
        args = (ne, c["h"], c["q"] if with_q else None, c["fixed"], c["X"][0] if with_f else None)
        _check("source[q=%d f=%d]" % (with_q, with_f), ne, _run_source(c, with_q, with_f), tc.source(*args), tc.source(*args, dtype=np.longdouble))
    args = (ne, c["h"], c["k"], c["kap"], c["X"][0])
    _check("flux", ne, _run_flux(c), tc.flux(*args), tc.flux(*args, dtype=np.longdouble))


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_kernels_in_place_off_line_and_bit_identical_run_to_run(ne):
    """the source in place, every kernel on buffers 8 bytes off a 16-byte line, and a second run: the same bits as the first"""
    c = _case(ne)
    runs = {"apply": lambda **kw: _run_apply(c, 3, **kw), "gradient": lambda **kw: _run_gradient(c, 3, **kw),
            "diagonal": lambda **kw: _run_diagonal(c, **kw), "flux": lambda **kw: _run_flux(c, **kw),
            "source": lambda **kw: _run_source(c, True, True, **kw)}
    for name, run in runs.items():
        first = run()
        assert not bool(torch.isnan(first).any()), name
        assert torch.equal(first, run()), name
        assert torch.equal(first, run(off=True)), name
    assert torch.equal(runs["source"](), runs["source"](in_place=True))
    assert torch.equal(runs["source"](), runs["source"](in_place=True, off=True))


# ---- the band ----

@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_band_assembly_matches_the_dense_operator(ne):
    c = _case(ne)
    args, keep = _head(ne)
    n, w = tc.num_nodes(ne), tc.band_width(ne)
    band, kap, mask = _dev(np.full(tc.band_doubles(n, w), np.nan)), _dev(c["kap"]), _mask(c)
    _lib.check(_lib.load().vfem_thermal_band_assemble(*args, _dp(c["Kc0"]), _p(kap), _p(mask), _p(band), pv._stream()))
    torch.cuda.synchronize()
    band = band.cpu().numpy()
    ref = tc.assemble(ne, c["Kc0"], c["kap"], c["fixed"], dtype=np.longdouble)
    f64 = tc.assemble(ne, c["Kc0"], c["kap"], c["fixed"])
    i, j = np.nonzero(np.tril(np.ones((n, n), dtype=bool)) & ~np.tril(np.ones((n, n), dtype=bool), -w - 1))
    got = band[tc.band_offset(i, j, w)]
    floor, err = _rel(f64[i, j], ref[i, j]), _rel(got, ref[i, j])
    print("band %s (n %d, w %d, %d entries): %.2e of the largest entry, floor %.2e" % (_name(ne), n, w, i.size, err, floor))
    assert err <= MARGIN * floor
    assert np.array_equal(got == 0.0, f64[i, j] == 0.0)                     # the sparsity, and the identity of the fixed nodes
    fixed = np.nonzero(c["fixed"])[0]
    assert np.all(band[tc.band_offset(fixed, fixed, w)] == 1.0)
    assert np.abs(np.triu(f64, w + 1)).max() == 0.0                          # nothing lies outside the band
    if n % 64:                                                              # the padding rows are the identity
        pad = np.arange(n, (n + 63) // 64 * 64)
        assert np.all(band[tc.band_offset(pad, pad, w)] == 1.0)


# ---- simulators of the restatement's problems ----

def _simulator(ne, h, k, rho, fixed, nodal=None, volumetric=None):
    sim = HeatConductionSimulator([np.zeros(len(ne)), np.array(ne) * np.array(h)], list(ne))
    sim.conductivity = k
    sim.setElementDensities(rho)
    sim.fixedTemperatureMask = fixed
    sim.setHeatSources(nodal=nodal, volumetric=volumetric)
    return sim


def _direct(ne):
    f = tc.direct_fixture(ne)
    return f, _simulator(ne, f["h"], f["k"], f["rho"], f["fixed"], f["nodal"], f["volumetric"])


@pytest.mark.parametrize("ne", [(16, 6), (8, 4, 3)], ids=_name)
def test_direct_chain_matches_the_restatement(ne):
    f, sim = _direct(ne)
    args = (ne, f["h"], f["k"], f["rho"], f["fixed"])
    J, T, g, Q = tc.compliance(*args, f["nodal"], f["volumetric"])
    JP, _, gP, lam = tc.pnorm_temperature(*args, 8.0, f["nodal"], f["volumetric"])
    assert sim.numDirectFactorizations() == 0 and sim.directBandBytes() == 8 * tc.band_doubles(tc.num_nodes(ne), tc.band_width(ne))
    obj = ThermalComplianceObjective(sim)
    assert sim.numDirectFactorizations() == 1
    peak = PNormTemperatureObjective(obj, P=8.0)
    rel = lambda got, want: float(np.abs(got - want).max() / np.abs(want).max())
    errs = dict(Q=rel(sim.buildLoadVector(), Q), solve=rel(sim.solve(Q), T), T=rel(obj.temperature(), T), J=abs(obj.evaluate() - J) / J,
                g=rel(obj.gradient(), g), JP=abs(peak.evaluate() - JP) / JP, lam=rel(peak.adjoint_device().cpu().numpy(), lam),
                gP=rel(peak.gradient(), gP), flux=rel(sim.flux(obj.temperature_device()), tc.flux(ne, f["h"], f["k"], tc.kappa(f["rho"]), T)))
    print("direct chain %s: %s" % (_name(ne), " ".join("%s %.2e" % kv for kv in errs.items())))
    assert max(errs.values()) < TOL_DIRECT
    assert sim.numDirectFactorizations() == 1                              # the adjoint solve and the plain solve added none
    assert abs(peak.maxTemperature() - np.abs(T).max()) < TOL_DIRECT * np.abs(T).max() <= peak.evaluate()
    assert bool((obj.gradient_device() <= 0).all())
    # unchanged densities: no factorisation, but a new temperature; other densities: one
    u = obj._u
    peak.updateCache(torch.from_numpy(f["rho"]).cuda())
    assert sim.numDirectFactorizations() == 1 and obj._u is u
    obj.updateCache(torch.from_numpy(f["rho"]).cuda())
    assert sim.numDirectFactorizations() == 1 and obj._u is not u and torch.equal(obj._u, u)
    obj.updateCache(torch.from_numpy(0.9 * f["rho"]).cuda())
    assert sim.numDirectFactorizations() == 2
    assert abs(peak.evaluate() - tc.pnorm_temperature(ne, f["h"], f["k"], 0.9 * f["rho"], f["fixed"], 8.0, f["nodal"], f["volumetric"])[0]) < TOL_DIRECT * JP * 2
    assert sim.numDirectFactorizations() == 2
    # the material and the mask drop the factor too
    sim.exponent = 2.0
    sim.solve_device(sim.buildLoadVector_device())
    assert sim.numDirectFactorizations() == 3


def test_refusals_of_the_python_layer():
    f, sim = _direct((16, 6))
    with pytest.raises(RuntimeError, match="Nonzero fixed temperatures"):
        sim.fixTemperatureInBox([0, 0], [0, 1], value=20.0)
    free = HeatConductionSimulator([[0, 0], [1, 1]], [4, 4])
    free.setHeatSources(volumetric=1.0)
    with pytest.raises(RuntimeError, match="no node has a fixed temperature"):
        ThermalComplianceObjective(free)
    with pytest.raises(RuntimeError, match="no node has a fixed temperature"):
        free.pcg_device(free.buildLoadVector_device())
    assert free.fixTemperatureInBox([0, 0.25], [0, 0.75]) == 3 and free.fixedTemperatureMask.sum() == 3
    with pytest.raises(RuntimeError, match="positive definite"):
        free.conductivity = np.array([[1.0, 2.0], [2.0, 1.0]])
    with pytest.raises(RuntimeError, match="solver is"):
        ThermalComplianceObjective(free, solver="multigrid")
    with pytest.raises(TypeError):
        PNormTemperatureObjective(free)


# ---- the closed forms on the device ----

@pytest.mark.parametrize("ne", tc.SLAB_SHAPES, ids=_name)
def test_slab_and_layers_on_the_device(ne):
    N = len(ne)
    h = tc.EDGES[N]
    q, k, rho = 1.3, 0.7, 0.8
    sim = _simulator(ne, h, k, np.full(tc.num_elements(ne), rho), tc.face_mask(ne, 0, 0), volumetric=q)
    T = ThermalComplianceObjective(sim).temperature()
    x = tc.node_coordinates(ne, h)[:, 0]
    exact = q / (tc.kappa(rho) * k) * (ne[0] * h[0] * x - 0.5 * x * x)
    slab, slab_bound = np.abs(T - exact).max() / np.abs(exact).max(), tc.analytic_bound(tc.SLAB_MEASURED[ne], ne)
    # the layers: the restatement's own case (its densities and its face load)
    rng = np.random.default_rng(1800 + tc.num_elements(ne))
    layer = rng.uniform(0.2, 1.0, size=ne[0])
    far = tc.face_mask(ne, 0, 1)
    idx = np.stack(np.meshgrid(*[np.arange(n + 1) for n in ne], indexing="ij"), axis=-1).reshape(-1, N)
    share = np.ones(tc.num_nodes(ne))
    for d in range(1, N):
        share *= np.where((idx[:, d] == 0) | (idx[:, d] == ne[d]), 0.5, 1.0)
    sim = _simulator(ne, h, k, np.repeat(layer, tc.num_elements(ne) // ne[0]), tc.face_mask(ne, 0, 0),
                     nodal=np.where(far, 0.9 * np.prod(h[1:]) * share, 0.0))
    Tf = ThermalComplianceObjective(sim).temperature()[far]
    want = 0.9 * np.sum(h[0] / (tc.kappa(layer) * k))
    assert abs(want - tc.layers_case(ne)[1]) == 0.0
    layers, layers_bound = np.abs(Tf - want).max() / want, tc.analytic_bound(tc.LAYERS_MEASURED[ne], ne)
    print("closed forms on the device %s: slab %.2e (bound %.2e), layers %.2e (bound %.2e)" % (_name(ne), slab, slab_bound, layers, layers_bound))
    assert slab < slab_bound and layers < layers_bound


# ---- the Jacobi-PCG ----

def _pcg_simulator(ne):
    f = tc.pcg_fixture(ne)
    sim = _simulator(ne, f["h"], 1.0, f["rho"], f["fixed"], volumetric=1.0)
    return f, sim


@functools.lru_cache(maxsize=None)
def _pcg_dense(ne):
    f = tc.pcg_fixture(ne)
    return tc.solve(f["A"], f["Q"])


@pytest.mark.parametrize("ne", tc.PCG_SHAPES, ids=_name)
def test_pcg_converges_within_the_restatements_count(ne):
    """measured on an MI355X: 240 and 72 iterations (the restatement stops at the same looks), bounds 248 and 80"""
    f, sim = _pcg_simulator(ne)
    Q = sim.buildLoadVector_device()
    assert np.abs(Q.cpu().numpy() - f["Q"]).max() < 1e-15
    x = sim.pcg_device(Q, tol=1e-8, maxIter=2000)
    its, rel = sim.last_iterations, sim.last_relative_residual
    true = float((Q - sim.applyK_device(x)).norm() / Q.norm())
    T = _pcg_dense(ne)
    sol = np.abs(x.cpu().numpy() - T).max() / np.abs(T).max()
    print("PCG %s: %d iterations (restatement crosses at %d, bound %d), |r|/|b| %.3e, true %.3e, solution %.2e of max |T| (bound %.2e)"
          % (_name(ne), its, tc.PCG_CROSSING[ne], tc.pcg_iteration_bound(ne), rel, true, sol, 10 * tc.PCG_SOLUTION_MEASURED[ne]))
    assert 0 < its <= tc.pcg_iteration_bound(ne) and its % tc.CHECK == 0
    assert rel <= 1e-8 and true <= 1e-8 + 10 * tc.PCG_GAP_MEASURED
    assert sol < 10 * tc.PCG_SOLUTION_MEASURED[ne]
    # the same bits on a second run
    assert torch.equal(x, sim.pcg_device(Q, tol=1e-8, maxIter=2000)) and sim.last_iterations == its
    # the objective warm-starts from its last temperature: a second update at the same densities takes no iteration
    obj = ThermalComplianceObjective(sim, solver="pcg")
    assert obj.iterations == its and torch.equal(obj._u, x)
    u = obj._u
    obj.updateCache(torch.from_numpy(f["rho"]).cuda())
    assert obj.iterations == 0 and obj._u is not u and torch.equal(obj._u, u)
    # both measures follow the temperature: |dJ| <= |Q|_1 max |dT|, and |dJ_P| <= |dT|_P <= nodes^(1/P) max |dT| with J_P >= max |T|
    dT = 10 * tc.PCG_SOLUTION_MEASURED[ne] * np.abs(T).max()
    J = float(f["Q"] @ T)
    assert abs(obj.evaluate() - J) < np.abs(f["Q"]).sum() * dT
    # the peak-temperature measure solves its adjoint through the same PCG
    peak = PNormTemperatureObjective(obj, P=8.0)
    JP = tc.pnorm_temperature(ne, f["h"], 1.0, f["rho"], f["fixed"], 8.0, volumetric=1.0)[0]
    assert abs(peak.evaluate() - JP) < tc.num_nodes(ne) ** (1.0 / 8.0) * dT and obj.iterations > 0
    assert bool(torch.isfinite(peak.gradient_device()).all()) and sim.numDirectFactorizations() == 0


def test_pcg_status_returns():
    """the two failures are status returns of kernels that ran normally: the iteration cap, and a p . Ap that is not positive"""
    f, sim = _pcg_simulator((40, 37))
    Q = sim.buildLoadVector_device()
    with pytest.raises(RuntimeError, match=r"vfem_thermal_pcg: not converged after 8 iterations: \|r\|/\|b\| = \d\.\d+e[-+]\d+ \(tol 1\.000e-08\)"):
        sim.pcg_device(Q, tol=1e-8, maxIter=8)
    assert sim.last_iterations == 8 and 1e-8 < sim.last_relative_residual < 10.0
    with pytest.raises(RuntimeError, match="not converged after 13 iterations"):
        sim.pcg_device(Q, tol=1e-8, maxIter=13)
    assert sim.last_iterations == 13
    # no conductivity at all around the free node (4, 4) of a 7 x 5 grid: its row of A is zero
    ne = (7, 5)
    rho = np.full((7, 5), 0.5)
    rho[3:5, 3:5] = 0.0
    sim = _simulator(ne, (1.0, 1.0), 1.0, rho.reshape(-1), tc.face_mask(ne, 0, 0), volumetric=1.0)
    sim.k_min = 0.0
    assert float(sim.diagonal_device()[4 * 6 + 4]) == 0.0
    with pytest.raises(RuntimeError, match=r"vfem_thermal_pcg: breakdown at iteration 1: p \. Ap = \S+ is not positive \(\|r\|/\|b\| = "):
        sim.pcg_device(sim.buildLoadVector_device(), tol=1e-8, maxIter=100)
    assert sim.last_iterations == 1
    # a zero right-hand side: the zero solution in no iteration
    x = sim.pcg_device(torch.zeros(48, dtype=torch.float64, device="cuda"), x0=torch.ones(48, dtype=torch.float64, device="cuda"))
    assert sim.last_iterations == 0 and float(x.abs().max()) == 0.0


# ---- the design loops ----

def _heated_square(n=16):
    """a uniformly heated unit square with a small sink at the middle of the edge x = 0"""
    sim = HeatConductionSimulator([[0, 0], [1, 1]], [n, n])
    assert sim.fixTemperatureInBox([0.0, 0.4], [0.0, 0.6]) > 0
    sim.setHeatSources(volumetric=1.0)
    return sim


def _restate(sim, x, P=None):
    ne = tuple(int(n) for n in sim.NbElementsPerDimension())
    args = (ne, tuple(sim._h), sim.conductivity, np.asarray(x), sim.fixedTemperatureMask)
    return tc.compliance(*args, volumetric=1.0) if P is None else tc.pnorm_temperature(*args, P, volumetric=1.0)


def test_three_oc_steps_on_the_heated_square():
    sim = _heated_square()
    obj = ThermalComplianceObjective(sim, skipSolve=True)
    smooth = pv.SmoothingFilter()
    smooth.radius = 1
    problem = pv.TopologyOptimizationProblem(sim, obj, [pv.TotalVolumeConstraint(0.4)], [smooth])
    problem.setVars(torch.full((sim.numElements(),), 0.4, dtype=torch.float64, device="cuda"))
    n0 = sim.numDirectFactorizations()
    J = [problem.evaluateObjective()]
    opt = pv.OCOptimizer(problem)
    for _ in range(3):
        opt.step()
        J.append(problem.evaluateObjective())
    want = _restate(sim, sim.getDensities())[0]
    print("three OC steps on the heated square: J %s, restatement at the final densities %.2e" % (" -> ".join("%.6f" % v for v in J), abs(J[-1] - want) / want))
    assert J[3] < J[2] < J[1] < J[0]
    assert abs(J[-1] - want) < TOL_DIRECT * want and abs(sim.getDensities().mean() - 0.4) < 1e-5
    assert sim.numDirectFactorizations() - n0 == 3


def test_three_mma_steps_of_a_cantilever_with_a_temperature_cap():
    n = 16
    heat = _heated_square(n)
    peak = PNormTemperatureObjective(ThermalComplianceObjective(heat, skipSolve=True), P=8.0)
    sim = pv.TensorProductSimulator([1, 1], [np.zeros(2), np.ones(2)], [n, n])
    sim.E_0, sim.E_min, sim.gamma = 1.0, 1e-4, 3.0
    idx = np.stack(np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij"), axis=-1).reshape(-1, 2)
    sim.dirichletMask = np.repeat((idx[:, 0] == 0)[:, None], 2, axis=1)
    load = np.zeros((sim.numNodes(), 2))
    load[(idx[:, 0] == n) & (idx[:, 1] == n // 2), 1] = -1.0
    sim.setLoads_device(torch.from_numpy(load).cuda())
    x0 = torch.full((sim.numElements(),), 0.5, dtype=torch.float64, device="cuda")
    start = peak.evaluate(x0)
    cap = mma.ObjectiveConstraint(peak, 1.1 * start)
    smooth = pv.SmoothingFilter()
    smooth.radius = 1
    problem = pv.TopologyOptimizationProblem(sim, pv.ComplianceObjective(sim), [pv.TotalVolumeConstraint(0.5), cap], [smooth])
    problem.setVars(x0)
    opt = mma.MMAOptimizer(problem, xmin=0.05, xmax=1.0, move=0.1)
    problem.evaluateConstraints()                                           # the cap stands at the start: a step itself solves nothing thermal
    n0 = heat.numDirectFactorizations()
    for step in range(3):
        opt.step()
        values = problem.evaluateConstraints()
        rows = problem.evaluateConstraintsJacobian_device()
        assert heat.numDirectFactorizations() - n0 == step + 1              # one thermal factorisation per step
    xPhys = problem._cached[-1]
    assert torch.equal(heat.getDensities_device(), xPhys) and torch.equal(sim.getDensities_device(), xPhys)
    JP, T, gP, lam = _restate(heat, xPhys.cpu().numpy(), P=8.0)
    got = cap.backprop_dev(xPhys).cpu().numpy()
    errs = abs(values[1] - (1.0 - JP / cap.upperBound)), np.abs(got - (-gP / cap.upperBound)).max() / np.abs(gP / cap.upperBound).max()
    print("three MMA steps with a temperature cap: J_P %.6f -> %.6f under %.6f, constraint %.2e, its gradient %.2e of the largest entry, multipliers %s"
          % (start, peak.evaluate(), cap.upperBound, errs[0], errs[1], opt.lambdas))
    assert errs[0] < TOL_DIRECT and errs[1] < TOL_DIRECT
    assert heat.numDirectFactorizations() - n0 == 3


# ---- the autograd nodes ----

@pytest.mark.parametrize("which", ["compliance", "peak"])
def test_autograd_nodes_return_the_objectives_gradient_bit_for_bit(which):
    f, sim = _direct((16, 6))
    obj = ThermalComplianceObjective(sim, skipSolve=True)
    target, node = (obj, thermal.thermalCompliance) if which == "compliance" else (PNormTemperatureObjective(obj, P=8.0), thermal.pNormTemperature)
    rho = torch.from_numpy(f["rho"]).cuda().requires_grad_(True)
    loss = node(rho, target)
    assert loss.dtype == torch.float64 and float(loss.detach()) == target.evaluate()
    loss.backward()
    assert torch.equal(rho.grad, target.gradient_device())
    # a weight on the loss, float32 densities in another shape
    rho32 = torch.from_numpy(f["rho"]).cuda().to(torch.float32).reshape(16, 6).requires_grad_(True)
    (3.0 * node(rho32, target)).backward()
    assert rho32.grad.dtype == torch.float32 and rho32.grad.shape == (16, 6)
    assert torch.equal(rho32.grad, (3.0 * target.gradient_device()).to(torch.float32).reshape(16, 6))
    # a stale objective raises
    loss = node(rho, target)
    obj.updateCache(torch.from_numpy(0.9 * f["rho"]).cuda())
    with pytest.raises(RuntimeError, match="was updated between forward and backward"):
        loss.backward()
    with pytest.raises(TypeError):
        node(rho, sim)
