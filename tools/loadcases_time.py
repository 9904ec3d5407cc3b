"""Load-case timing: the load assembly and the density gradient of ndr_amd.loadcases on one grid, beside the paths that did the same
work before them.  Prints one JSON line per measurement.  The whole run is bounded by --timeout seconds (SIGALRM ends it with exit
status 124).

    python tools/loadcases_time.py [--grid 256 256 128] [--cases 4] [--reps 20] [--warmup 3] [--timeout 300] [--baseline-only]

Each path is timed through its entry point (HIP events, median of --reps).  The assembly is an asynchronous launch; the gradient's
figure includes the upload of K0 and the patterns and a synchronise.  The two comparisons:
  gradient, k fixed-load cases   against k calls of ``sim.complianceGradient_device`` (vfem_sim_compliance_gradient) and the torch
                                 additions that weight and combine them
  assembly of an eigenstrain     against the torch ``pyVoxelFEM._stress_load`` with the same weights E(rho)
``--baseline-only`` measures the comparison paths alone (they need nothing of this module, so they run on a tree without it).
Compulsory HBM traffic, from the shapes, n = dofs of a vector:
  assemble                       ((1 or 2) n + (1 or 2) elements) 8 + nodes bytes    f_in if given, f_out, the multipliers, the mask
  gradient, k cases              (k n + (2 or 3) elements) 8 bytes                   the displacements, dE, dm if given, g
The fraction is of the 8 TB/s peak.
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


def _expire(signum, frame):
    print(json.dumps({"tool": "loadcases_time", "error": "timeout"}), flush=True)
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


def _line(what, grid, ms, nbytes, **more):
    med, lo, hi = ms
    out = {"tool": "loadcases_time", "path": what, "grid": list(grid), "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
           "min_bytes": int(nbytes), "TBps": round(nbytes / med * 1e-9, 3), "fraction_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}
    out.update(more)
    print(json.dumps(out), flush=True)
    return med


def _run(grid, cases, reps, warmup, baseline_only):
    from ndr_amd import _lib
    from ndr_amd import pyVoxelFEM as pv
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    N = len(grid)
    h = np.full(N, 1.0 / max(grid))
    sim = pv.TensorProductSimulator([1] * N, [np.zeros(N), np.asarray(grid) * h], list(grid))
    sim.E_0, sim.E_min, sim.gamma = 1.0, 1e-3, 3.0
    nelem, nnode = sim.numElements(), sim.numNodes()
    n = nnode * N
    gen = torch.Generator("cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
    rho = 0.2 + 0.8 * rand(nelem)
    sim.setElementDensities(rho)
    U = rand(cases, nnode, N) - 0.5
    w = [1.0 + 0.25 * i for i in range(cases)]
    E = (1e-3 + rho ** 3.0 * (1.0 - 1e-3)).contiguous()
    dE = (3.0 * rho ** 2.0 * (1.0 - 1e-3)).contiguous()

    # the paths that were there before
    def separate():
        g = w[0] * sim.complianceGradient_device(U[0])
        for i in range(1, cases):
            g = g + w[i] * sim.complianceGradient_device(U[i])
        return g

    old_g = _line("gradient_separate_calls", grid, _time(separate, reps, warmup), (cases * n + 2 * nelem) * 8, cases=cases)
    eps = 0.01 * np.eye(N)
    sigma = sim.ETensor.doubleContract(eps)
    Egrid = E.reshape(tuple(grid))
    old_a = _line("stress_load_torch", grid, _time(lambda: pv._stress_load(sigma, h, 1, Egrid), reps, warmup), (n + nelem) * 8)
    if baseline_only:
        return

    from ndr_amd import loadcases
    g_ = loadcases._Grid(sim)
    head = g_.head()
    Lb, Lt = g_.patterns(loadcases.LoadCase(loads=0, acceleration=[0.0, -1.0] + [0.0] * (N - 2), eigenstrain=eps))
    f_in, f_out = rand(nnode, N) - 0.5, torch.empty((nnode, N), dtype=torch.float64, device="cuda")
    stream = None
    new_a = _line("assemble_eigenstrain", grid,
                  _time(lambda: _lib.check(lib.vfem_loads_assemble(*head, None, dp(Lt), None, p(E), None, None, p(f_out), stream)), reps, warmup),
                  (n + nelem) * 8)
    _line("assemble_both_masked_added", grid,
          _time(lambda: _lib.check(lib.vfem_loads_assemble(*head, dp(Lb), dp(Lt), p(rho), p(E), p(g_.mask), p(f_in), p(f_out), stream)), reps, warmup),
          (2 * n + 2 * nelem) * 8 + nnode)
    K0 = np.ascontiguousarray(sim.fullDensityElementStiffnessMatrix())
    cK = np.ascontiguousarray(-0.5 * np.asarray(w))
    co = np.ascontiguousarray(np.asarray(w))
    LB, LT = np.ascontiguousarray(np.tile(Lb, (cases, 1))), np.ascontiguousarray(np.tile(Lt, (cases, 1)))
    g = torch.empty(nelem, dtype=torch.float64, device="cuda")
    new_g = _line("gradient_fused_fixed_loads", grid,
                  _time(lambda: _lib.check(lib.vfem_loads_gradient(*head, cases, dp(K0), dp(cK), None, None, None, None, p(dE), None, p(U), p(g),
                                                                   stream)), reps, warmup), (cases * n + 2 * nelem) * 8, cases=cases)
    _line("gradient_fused_with_patterns", grid,
          _time(lambda: _lib.check(lib.vfem_loads_gradient(*head, cases, dp(K0), dp(cK), dp(co), dp(co), dp(LB), dp(LT), p(dE), p(rho), p(U), p(g),
                                                           stream)), reps, warmup), (cases * n + 3 * nelem) * 8, cases=cases)
    _line("gradient_fused_one_case", grid,
          _time(lambda: _lib.check(lib.vfem_loads_gradient(*head, 1, dp(K0), dp(cK), None, None, None, None, p(dE), None, p(U), p(g), stream)),
                reps, warmup), (n + 2 * nelem) * 8, cases=1)
    print(json.dumps({"tool": "loadcases_time", "grid": list(grid), "cases": cases,
                      "gradient_separate_over_fused": round(old_g / new_g, 3), "stress_load_torch_over_assemble": round(old_a / new_a, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs="+", default=[256, 256, 128])
    ap.add_argument("--cases", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--baseline-only", action="store_true")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    _run(tuple(a.grid), a.cases, a.reps, a.warmup, a.baseline_only)


if __name__ == "__main__":
    main()
