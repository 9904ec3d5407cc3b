"""Heat-conduction timing: the element-wise kernels of ndr_amd.thermal on one grid beside two kernels with the same access pattern
and the torch composition a user had before, then the two solvers.  Prints one JSON line per measurement and writes them all to
--out.  The whole run is bounded by --timeout seconds (SIGALRM ends it with exit status 124).

    python tools/thermal_time.py [--grid 256 256 128] [--reps 20] [--warmup 3] [--timeout 500] [--out profiles/thermal_time.json]

Each path is timed through its entry point (HIP events, median of --reps after --warmup calls).  Compulsory HBM traffic, from the
shapes (nodes, elements, N axes, k columns), in bytes:
  thermal apply, k columns     (2 k nodes + elements) 8 + nodes      X and Y, the conductivities, the fixed-node bytes
  thermal source               (2 nodes + elements) 8 + nodes        f_in and f_out, the volumetric source, the fixed-node bytes
  thermal gradient, k pairs    (2 k nodes + 2 elements) 8            A and B, dkappa, g  (k nodes + ... when B is A)
  modal mass apply, 1 column   (2 N nodes + elements) 8 + nodes      the yardstick with the same gather and N components per node
  loads assemble (eigenstrain) (N nodes + elements) 8                the second yardstick
  torch apply                  the same bytes as the thermal apply with one column (what it would have to move, not what it moves)
The fraction is of the 8 TB/s peak.  The solvers are reported without a byte count: the band assembly, the factorisation and one
solve on --band-grids, and one PCG iteration on --grid (the difference of a 16- and an 8-iteration call, over 8).
"""
import argparse
import ctypes
import json
import os
import signal
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12
LINES = []


def _emit(d):
    LINES.append(d)
    print(json.dumps(d), flush=True)


def _expire(signum, frame):
    print(json.dumps({"tool": "thermal_time", "error": "timeout"}), flush=True)
    os._exit(124)


def _time(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def _line(what, grid, ms, nbytes=None, **more):
    med, lo, hi = ms
    out = {"tool": "thermal_time", "path": what, "grid": list(grid), "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
    if nbytes is not None:
        out.update(min_bytes=int(nbytes), TBps=round(nbytes / med * 1e-9, 3), fraction_of_hbm_peak=round(nbytes / (med * 1e-3) / HBM_PEAK, 3))
    out.update(more)
    _emit(out)
    return out


def _torch_apply(Kc0, kappa_grid, fixed_grid, x_grid):
    """A x composed from slice additions over the 2^N x 2^N entries of Kc0: what a user had before the kernel"""
    N = x_grid.dim()
    xm = torch.where(fixed_grid, torch.zeros_like(x_grid), x_grid)
    y = torch.zeros_like(x_grid)
    sl = lambda a: tuple(slice((a >> (N - 1 - d)) & 1, x_grid.shape[d] - 1 + ((a >> (N - 1 - d)) & 1)) for d in range(N))
    for a in range(2 ** N):
        for b in range(2 ** N):
            y[sl(a)] += (kappa_grid * float(Kc0[a, b])) * xm[sl(b)]
    return torch.where(fixed_grid, x_grid, y)


def _kernels(grid, reps, warmup):
    from ndr_amd import _lib, thermal
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    N = len(grid)
    h = np.full(N, 1.0 / max(grid))
    ne = np.asarray(grid, dtype=np.int64)
    head = (N, ne.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    nelem, nnode = int(np.prod(ne)), int(np.prod(ne + 1))
    gen = torch.Generator("cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
    rho = 0.2 + 0.8 * rand(nelem)
    kappa = (1e-3 + rho ** 3.0 * (1.0 - 1e-3)).contiguous()
    dkappa = (3.0 * rho ** 2.0 * (1.0 - 1e-3)).contiguous()
    fixed = (rand(nnode) < 0.05).to(torch.uint8)
    k = np.array([[1.4, 0.3, -0.2], [0.3, 0.8, 0.1], [-0.2, 0.1, 1.1]])[:N, :N]
    Kc0 = np.ascontiguousarray(thermal.conductivityMatrix(k, h))
    X, Y = rand(8, nnode) - 0.5, torch.empty((8, nnode), dtype=torch.float64, device="cuda")
    g = torch.empty(nelem, dtype=torch.float64, device="cuda")
    co = np.ascontiguousarray(np.linspace(1.0, 2.0, 8))
    stream = None
    check = _lib.check

    rows = {}
    for cols in (1, 8):
        rows["apply%d" % cols] = _line("thermal_apply", grid, _time(lambda: check(lib.vfem_thermal_apply(
            *head, dp(Kc0), p(kappa), p(fixed), cols, p(X), p(Y), stream)), reps, warmup), (2 * cols * nnode + nelem) * 8 + nnode, columns=cols)
    rows["source"] = _line("thermal_source", grid, _time(lambda: check(lib.vfem_thermal_source(
        *head, dp(h), p(rho), p(fixed), p(X), p(Y), stream)), reps, warmup), (2 * nnode + nelem) * 8 + nnode)
    for cols in (1, 8):
        rows["gradient%d" % cols] = _line("thermal_gradient", grid, _time(lambda: check(lib.vfem_thermal_gradient(
            *head, cols, dp(Kc0), dp(co), p(dkappa), p(X), p(Y), p(g), stream)), reps, warmup), (2 * cols * nnode + 2 * nelem) * 8, columns=cols)
    _line("thermal_gradient_one_block", grid, _time(lambda: check(lib.vfem_thermal_gradient(
        *head, 1, dp(Kc0), dp(co), p(dkappa), p(X), p(X), p(g), stream)), reps, warmup), (nnode + 2 * nelem) * 8, columns=1)
    flux = torch.empty((nelem, N), dtype=torch.float64, device="cuda")
    _line("thermal_flux", grid, _time(lambda: check(lib.vfem_thermal_flux(
        *head, dp(h), dp(np.ascontiguousarray(k)), p(kappa), p(X), p(flux), stream)), reps, warmup), (nnode + (1 + N) * nelem) * 8)
    del flux

    # the two yardsticks on the same grid
    mhead = head + (dp(h),)
    bits = fixed * (2 ** N - 1)
    XN, YN = rand(nnode, N) - 0.5, torch.empty((nnode, N), dtype=torch.float64, device="cuda")
    rows["mass"] = _line("modal_mass_apply", grid, _time(lambda: check(lib.vfem_modal_mass_apply(
        *mhead, p(rho), p(bits), 1, p(XN), p(YN), stream)), reps, warmup), (2 * N * nnode + nelem) * 8 + nnode, columns=1)
    Lt = np.ascontiguousarray(np.linspace(-1.0, 1.0, N * 2 ** N))
    rows["loads"] = _line("loads_assemble_eigenstrain", grid, _time(lambda: check(lib.vfem_loads_assemble(
        *mhead, None, dp(Lt), None, p(kappa), None, None, p(YN), stream)), reps, warmup), (N * nnode + nelem) * 8)
    del XN, YN

    # what a user had before
    shape_n, shape_e = tuple(int(n) + 1 for n in grid), tuple(int(n) for n in grid)
    before = _line("torch_apply_slices", grid, _time(lambda: _torch_apply(Kc0, kappa.reshape(shape_e), fixed.bool().reshape(shape_n),
                                                                         X[0].reshape(shape_n)), max(3, reps // 4), 1), (2 * nnode + nelem) * 8 + nnode)
    check(lib.vfem_thermal_apply(*head, dp(Kc0), p(kappa), p(fixed), 1, p(X), p(Y), stream))
    ref = _torch_apply(Kc0, kappa.reshape(shape_e), fixed.bool().reshape(shape_n), X[0].reshape(shape_n)).reshape(-1)
    agree = float((Y[0] - ref).abs().max() / ref.abs().max())
    floor = min(rows["mass"]["fraction_of_hbm_peak"], rows["loads"]["fraction_of_hbm_peak"])
    _emit({"tool": "thermal_time", "grid": list(grid), "torch_apply_over_kernel": round(before["ms"] / rows["apply1"]["ms"], 2),
           "kernel_against_torch_apply": agree, "lower_yardstick_fraction": floor,
           "apply1_at_least_the_lower_yardstick": bool(rows["apply1"]["fraction_of_hbm_peak"] >= floor)})

    # one PCG iteration: a sink on the face x = 0, a uniform source
    mask = torch.zeros(shape_n, dtype=torch.uint8, device="cuda")
    mask[0] = 1
    mask = mask.reshape(-1).contiguous()
    b = torch.empty(nnode, dtype=torch.float64, device="cuda")
    check(lib.vfem_thermal_source(*head, dp(h), p(torch.ones_like(rho)), p(mask), None, p(b), stream))
    it, rel = ctypes.c_int(0), ctypes.c_double(0.0)

    def pcg(iters):
        x = torch.zeros_like(b)
        lib.vfem_thermal_pcg(*head, dp(Kc0), p(kappa), p(mask), p(b), p(x), 1e-12, iters, ctypes.byref(it), ctypes.byref(rel), stream)

    t8, t16 = _time(lambda: pcg(8), max(3, reps // 4), 1), _time(lambda: pcg(16), max(3, reps // 4), 1)
    _emit({"tool": "thermal_time", "path": "thermal_pcg_iteration", "grid": list(grid), "ms_8_iterations": round(t8[0], 3),
           "ms_16_iterations": round(t16[0], 3), "ms_per_iteration": round((t16[0] - t8[0]) / 8.0, 4),
           "relative_residual_after_16": rel.value})


def _band(grid, reps):
    from ndr_amd import _lib, thermal
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    N = len(grid)
    sim = thermal.HeatConductionSimulator([np.zeros(N), np.ones(N) * np.asarray(grid) / max(grid)], list(grid))
    gen = torch.Generator("cuda").manual_seed(11)
    sim.setElementDensities(0.2 + 0.8 * torch.rand(sim.numElements(), dtype=torch.float64, device="cuda", generator=gen))
    sim.fixTemperatureInBox(np.zeros(N), [0.0] + [1.0] * (N - 1))
    sim.setHeatSources(volumetric=1.0)
    n, w = sim._band_geometry()
    Q = sim.buildLoadVector_device()
    band = [None]

    def assemble():
        band[0] = None
        band[0] = sim.assembleBand_device()

    ta = _time(assemble, reps, 1)

    def factor():
        assemble()
        _lib.check(lib.vfem_band_spd_factor(n, w, p(band[0]), None))

    tf = _time(factor, reps, 1)
    x = Q.clone()
    ts = _time(lambda: _lib.check(lib.vfem_band_spd_solve(n, w, p(band[0]), p(x), 1, None)), reps, 1)
    T = sim.solve_device(Q)
    res = float((Q - sim.applyK_device(T)).norm() / Q.norm())
    _emit({"tool": "thermal_time", "path": "thermal_band", "grid": list(grid), "n": n, "w": w, "band_MB": round(sim.directBandBytes() / 1e6, 1),
           "assemble_ms": round(ta[0], 3), "assemble_and_factor_ms": round(tf[0], 3), "factor_ms": round(tf[0] - ta[0], 3),
           "solve_ms": round(ts[0], 3), "relative_residual": res})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs="+", default=[256, 256, 128])
    ap.add_argument("--band-grids", type=str, default="250x125,64x32x32")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "thermal_time.json"))
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    _kernels(tuple(a.grid), a.reps, a.warmup)
    for name in [s for s in a.band_grids.split(",") if s]:
        _band(tuple(int(v) for v in name.split("x")), 3)
    with open(a.out, "w") as f:
        json.dump({"tool": "thermal_time", "note": "one run, one box", "measurements": LINES}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
