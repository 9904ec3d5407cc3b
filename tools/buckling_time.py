"""Buckling timing: the geometric stiffness apply, the adjoint load and the density gradient of ndr_amd.buckling on one grid.  Prints
one JSON line per kernel.  The whole run is bounded by --timeout seconds (SIGALRM ends it with exit status 124).

    python tools/buckling_time.py [--grid 256 256 128] [--block 6] [--modes 4] [--reps 20] [--warmup 3] [--timeout 300]

Each kernel is timed through its entry point (HIP events, median of --reps).  The apply and the adjoint load are asynchronous
launches (the table T is on the device after the warm-up calls); the gradient's figure includes the upload of K0 and a synchronise.
Compulsory HBM traffic, from the shapes, n = dofs of a column:
  geometric apply, c columns   ((2 c + 1) n + elements) 8 + nodes bytes    X read once, Y written, u, the multipliers, the mask
  adjoint load, k modes        ((k + 1) n + elements) 8 + nodes bytes      the modes read once, a written
  gradient, k modes            ((k + 2) n + 3 elements) 8 bytes            u, v, the modes, dmG, dE, g
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
    print(json.dumps({"tool": "buckling_time", "error": "timeout"}), flush=True)
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
    out = {"tool": "buckling_time", "kernel": what, "grid": list(grid), "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
           "min_bytes": int(nbytes), "TBps": round(nbytes / med * 1e-9, 3), "fraction_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}
    out.update(more)
    print(json.dumps(out), flush=True)


def _kernels(grid, block, modes, reps, warmup):
    from ndr_amd import _lib
    from ndr_amd.materials import ElasticityTensor
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    N = len(grid)
    ne, h = np.asarray(grid, dtype=np.int64), np.full(N, 1.0 / max(grid))
    D = np.ascontiguousarray(ElasticityTensor(1.0, 0.3, dim=N).D)
    head = (N, ne.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), dp(h), dp(D))
    nelem, nnode = int(np.prod(grid)), int(np.prod([g + 1 for g in grid]))
    n = nnode * N
    gen = torch.Generator("cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
    cols = max(block, modes)
    X, Y = rand(cols, n) - 0.5, torch.empty((cols, n), dtype=torch.float64, device="cuda")
    u, v = rand(n) - 0.5, rand(n) - 0.5
    m = 0.2 + 0.8 * rand(nelem)
    mask = torch.zeros(nnode, dtype=torch.uint8, device="cuda")
    mask[:nnode // (grid[0] + 1)] = 7 if N == 3 else 3
    stream = None
    for c in (1, block):
        ms = _time(lambda: _lib.check(lib.vfem_buckling_geom_apply(*head, p(m), p(u), p(mask), c, p(X), p(Y), stream)), reps, warmup)
        _line("geom_apply", grid, ms, ((2 * c + 1) * n + nelem) * 8 + nnode, columns=c)
    co = np.ones(8)
    a = torch.empty(n, dtype=torch.float64, device="cuda")
    ms = _time(lambda: _lib.check(lib.vfem_buckling_adjoint_load(*head, p(m), p(mask), modes, dp(co), p(X), p(a), stream)), reps, warmup)
    _line("adjoint_load", grid, ms, ((modes + 1) * n + nelem) * 8 + nnode, modes=modes)
    ke = N * 2 ** N
    K0 = np.random.default_rng(4).standard_normal((ke, ke))
    K0 = np.ascontiguousarray(K0 + K0.T)
    g = torch.empty(nelem, dtype=torch.float64, device="cuda")
    ms = _time(lambda: _lib.check(lib.vfem_buckling_gradient(*head, modes, dp(K0), dp(co), dp(co), p(m), p(m), p(u), p(v), p(X), p(g),
                                                             stream)), reps, warmup)
    _line("gradient", grid, ms, ((modes + 2) * n + 3 * nelem) * 8, modes=modes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs="+", default=[256, 256, 128])
    ap.add_argument("--block", type=int, default=6)
    ap.add_argument("--modes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    _kernels(tuple(a.grid), a.block, a.modes, a.reps, a.warmup)


if __name__ == "__main__":
    main()
