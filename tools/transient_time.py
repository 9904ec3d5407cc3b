"""Transient heat-conduction timing: the two-term apply beside the one-term apply of the same run, the time-accumulated gradient, one
backward-Euler step by multigrid-PCG beside one steady multigrid-PCG solve, and a whole objective plus gradient.  Prints one JSON line
per measurement and writes them all to --out.  The whole run is bounded by --timeout seconds (SIGALRM ends it with exit status 124).

    python tools/transient_time.py [--grid 256 256 128] [--steps 16] [--reps 20] [--warmup 3] [--timeout 500] [--out profiles/transient_time.json]

Each kernel is timed through its entry point (HIP events, median of --reps after --warmup calls).  Compulsory HBM traffic, from the
shapes (nodes, elements, S steps), in bytes:
  thermal apply, 1 column      (2 nodes + elements) 8 + nodes         X and Y, the conductivities, the fixed-node bytes
  transient apply, k columns   (2 k nodes + 2 elements) 8 + nodes     the same and the capacities  (+ k nodes 8 with b)
  transient gradient, S steps  (2 S + 1) nodes 8 + 3 elements 8       every row of T and Lam once, dkappa, dcap, g
The fraction is of the 8 TB/s peak.  The solves and the objective are wall-clock times of one call each after one warm-up call
(they synchronise themselves).  Nothing here is a threshold: the figures are what one run on one box gave.
"""
import argparse
import ctypes
import json
import os
import signal
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.thermal_time import HBM_PEAK, _time          # noqa: E402

LINES = []


def _emit(d):
    d = dict({"tool": "transient_time"}, **d)
    LINES.append(d)
    print(json.dumps(d), flush=True)


def _expire(signum, frame):
    print(json.dumps({"tool": "transient_time", "error": "timeout"}), flush=True)
    os._exit(124)


def _line(what, grid, ms, nbytes, **more):
    med, lo, hi = ms
    out = {"path": what, "grid": list(grid), "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "min_bytes": int(nbytes),
           "TBps": round(nbytes / med * 1e-9, 3), "fraction_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}
    out.update(more)
    _emit(out)
    return out


def _wall(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _kernels(grid, steps, reps, warmup):
    from ndr_amd import _lib, thermal, transient
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
    cap = (1e-3 + rho * (1.0 - 1e-3)).contiguous()
    fixed = (rand(nnode) < 0.05).to(torch.uint8)
    k = np.array([[1.4, 0.3, -0.2], [0.3, 0.8, 0.1], [-0.2, 0.1, 1.1]])[:N, :N]
    Kc0 = np.ascontiguousarray(thermal.conductivityMatrix(k, h))
    m = transient.capacityEntries(h)
    dt = 0.01
    mb = np.ascontiguousarray(m / dt)
    X, Y = rand(8, nnode) - 0.5, torch.empty((8, nnode), dtype=torch.float64, device="cuda")
    check = _lib.check
    one = _line("thermal_apply", grid, _time(lambda: check(lib.vfem_thermal_apply(*head, dp(Kc0), p(kappa), p(fixed), 1, p(X), p(Y), None)),
                                             reps, warmup), (2 * nnode + nelem) * 8 + nnode, columns=1)
    for cols in (1, 8):
        two = _line("transient_apply", grid, _time(lambda: check(lib.vfem_transient_apply(
            *head, dp(Kc0), dp(mb), p(kappa), p(cap), p(fixed), 1, cols, p(X), None, p(Y), None)), reps, warmup),
            (2 * cols * nnode + 2 * nelem) * 8 + nnode, columns=cols)
        if cols == 1:
            _emit({"grid": list(grid), "two_term_over_one_term_apply": round(two["ms"] / one["ms"], 3)})
    _line("transient_apply_with_b", grid, _time(lambda: check(lib.vfem_transient_apply(
        *head, dp(Kc0), dp(mb), p(kappa), p(cap), p(fixed), 0, 1, p(X), p(X[1]), p(Y), None)), reps, warmup),
        (3 * nnode + 2 * nelem) * 8 + nnode, columns=1)
    del X, Y
    T, Lam = rand(steps + 1, nnode), rand(steps + 1, nnode)
    g = torch.empty(nelem, dtype=torch.float64, device="cuda")
    _line("transient_gradient", grid, _time(lambda: check(lib.vfem_transient_gradient(
        *head, steps, dp(Kc0), dp(m), dt, 1.0, p(kappa), p(cap), p(T), p(Lam), p(g), None)), max(3, reps // 4), 1),
        ((2 * steps + 1) * nnode + 3 * nelem) * 8, steps=steps)


def _solves(grid, steps):
    from ndr_amd import thermal, transient
    N = len(grid)
    heat = thermal.HeatConductionSimulator([np.zeros(N), np.asarray(grid) / max(grid)], list(grid))
    gen = torch.Generator("cuda").manual_seed(11)
    heat.setElementDensities(0.2 + 0.8 * torch.rand(heat.numElements(), dtype=torch.float64, device="cuda", generator=gen))
    heat.fixTemperatureInBox(np.zeros(N), [0.0] + [1.0] * (N - 1))
    heat.setHeatSources(volumetric=1.0)
    Q = heat.buildLoadVector_device()
    ms, _ = _wall(lambda: heat.pcg_device(Q, preconditioner="multigrid"))
    _emit({"path": "steady_multigrid_pcg", "grid": list(grid), "ms": round(ms, 2), "iterations": heat.last_iterations})
    sim = transient.TransientHeatSimulator(heat)
    dt = 0.01
    ms, _ = _wall(lambda: sim.march_device(1, dt, 1.0, solver="pcg", preconditioner="multigrid"))
    _emit({"path": "backward_euler_step_multigrid_pcg", "grid": list(grid), "dt": dt, "ms": round(ms, 2), "iterations": sim.last_iterations,
           "hierarchy_builds": sim.numMultigridBuilds()})
    obj = transient.TransientPNormTemperatureObjective(sim, steps, dt, solver="pcg", preconditioner="multigrid", skipSolve=True)

    def whole():
        obj.updateCache(None)
        return obj.gradient_device()

    ms, _ = _wall(whole)
    _emit({"path": "objective_and_gradient", "grid": list(grid), "steps": steps, "dt": dt, "ms": round(ms, 1), "march_iterations": obj.iterations,
           "adjoint_iterations": sim.last_adjoint_iterations, "trajectory_MB": round((steps + 1) * heat.numNodes() * 8 / 1e6, 1),
           "hierarchy_builds": sim.numMultigridBuilds()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs="+", default=[256, 256, 128])
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "transient_time.json"))
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    _kernels(tuple(a.grid), a.steps, a.reps, a.warmup)
    _solves(tuple(a.grid), a.steps)
    with open(a.out, "w") as f:
        json.dump({"tool": "transient_time", "note": "one run, one box", "measurements": LINES}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
