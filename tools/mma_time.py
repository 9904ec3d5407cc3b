"""MMA timing: one fused pass over the dual of the subproblem (vfem_mma_dual_eval) on n variables with m constraints, and the
whole subproblem (vfem_mma_subproblem) on the same inputs.  Prints one JSON line per m.  The whole run is bounded by --timeout
seconds (SIGALRM ends it with exit status 124).

    python tools/mma_time.py [--grid 512 256 256] [--m 1 2 3] [--reps 20] [--warmup 3] [--timeout 300]

The pass is timed through the entry point (HIP events, median); that call also allocates its partial sums, copies the finished
sums to the host and synchronises, so the same call on 2 variables is timed as the fixed cost and subtracted.  Compulsory HBM
traffic of one pass: x, L, U, xmin, xmax, g_0 and the m rows of g, (6 + m) * 8 bytes per variable; the fraction is of the 8 TB/s
peak.  The inputs are a design in mid-optimisation: densities in [0, 1], asymptotes half a range away, a negative objective
gradient (compliance), a volume constraint and m - 1 constraints of mixed sign.
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

HBM_PEAK = 8.0e12


def _expire(signum, frame):
    print(json.dumps({"tool": "mma_time", "error": "timeout"}), flush=True)
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
    return float(np.median(ms))


def _inputs(n, m):
    gen = torch.Generator("cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
    x = 0.05 + 0.9 * rand(n)
    g = torch.empty((m, n), dtype=torch.float64, device="cuda")
    g[0] = 1.0 / (0.4 * n)
    if m > 1:
        g[1:] = (rand(m - 1, n) - 0.5) / n
    return dict(x=x, L=x - 0.5, U=x + 0.5, xmin=torch.zeros_like(x), xmax=torch.ones_like(x), g0=-(0.1 + rand(n)), g=g)


def _figures(n, m, reps, warmup):
    from ndr_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    lam, b = np.full(m, 300.0), np.zeros(m)
    W, grad, scale, hess = ctypes.c_double(0.0), np.zeros(m), np.zeros(m), np.zeros((m, m))

    def one_pass(v, count):
        _lib.check(lib.vfem_mma_dual_eval(count, m, p(v["x"]), p(v["L"]), p(v["U"]), p(v["xmin"]), p(v["xmax"]), 0.5, p(v["g0"]),
                                          p(v["g"]), dp(b), 1000.0, dp(lam), ctypes.byref(W), dp(grad), dp(scale), dp(hess), None))

    big, small = _inputs(n, m), _inputs(2, m)
    t_call = _time(lambda: one_pass(big, n), reps, warmup)
    t_fixed = _time(lambda: one_pass(small, 2), reps, warmup)
    kernel_ms = max(t_call - t_fixed, 1e-6)
    nbytes = (6 + m) * 8 * n
    # the whole subproblem: the volume constraint slightly violated, the others met
    f = np.array([0.02] + [-0.1] * (m - 1))
    xnew = torch.empty_like(big["x"])
    lam_out, y_out, its, res = np.zeros(m), np.zeros(m), ctypes.c_int(0), ctypes.c_double(0.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check(lib.vfem_mma_subproblem(n, m, p(big["x"]), p(big["L"]), p(big["U"]), p(big["xmin"]), p(big["xmax"]), 0.5, dp(f),
                                       p(big["g0"]), p(big["g"]), 1000.0, 1e-9, 200, p(xnew), dp(lam_out), dp(y_out), ctypes.byref(its),
                                       ctypes.byref(res), None))
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    return {"tool": "mma_time", "n": n, "m": m, "pass_call_ms": round(t_call, 4), "pass_fixed_cost_ms": round(t_fixed, 4),
            "pass_kernel_ms": round(kernel_ms, 4), "pass_min_bytes": nbytes, "pass_TBps": round(nbytes / kernel_ms * 1e-9, 3),
            "pass_fraction_of_hbm_peak": round(nbytes / (kernel_ms * 1e-3) / HBM_PEAK, 3),
            "subproblem_seconds": round(seconds, 4), "subproblem_newton_iterations": its.value, "subproblem_residual": res.value,
            "lambda": [float(v) for v in lam_out]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs="+", default=[512, 256, 256])
    ap.add_argument("--m", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    n = int(np.prod(a.grid))
    for m in a.m:
        print(json.dumps(_figures(n, m, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
