"""Natural-frequency timing: the mass operator, the Gram matrix, the linear combination and the density gradient of ndr_amd.modal on
one grid, and one whole eigenmodes() solve on a second, smaller grid.  Prints one JSON line per kernel and one for the solve.  The
whole run is bounded by --timeout seconds (SIGALRM ends it with exit status 124).

    python tools/modal_time.py [--grid 256 256 128] [--block 6] [--solve-grid 64 32 32] [--reps 20] [--warmup 3] [--timeout 300]

Each kernel is timed through its entry point (HIP events, median of --reps; the calls are asynchronous but for the gradient, which
uploads K0 and synchronises).  Compulsory HBM traffic, from the shapes, n = dofs of a column:
  mass apply, c columns      (2 c n + elements) 8 + nodes bytes      X read once, Y written, the multipliers, the mask
  Gram, ka x kb of A, B      (ka + kb) n 8 bytes                      (A = B: ka n 8)
  combine, kin -> kout       (kin + kout) n 8 bytes
  gradient, k modes          (k n + 3 elements) 8 bytes
The Gram kernel as built reads more than that: each of its ceil(ka / 8) ceil(kb / 8) tile rows reads 16 columns.  The fraction is of
the 8 TB/s peak.  The solve runs on random densities in [0.2, 1] with the x = 0 face clamped, preconditioned by one V-cycle.
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
    print(json.dumps({"tool": "modal_time", "error": "timeout"}), flush=True)
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
    out = {"tool": "modal_time", "kernel": what, "grid": list(grid), "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
           "min_bytes": int(nbytes), "TBps": round(nbytes / med * 1e-9, 3), "fraction_of_hbm_peak": round(nbytes / (med * 1e-3) / HBM_PEAK, 3)}
    out.update(more)
    print(json.dumps(out), flush=True)


def _kernels(grid, k, reps, warmup):
    from ndr_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    N = len(grid)
    ne, h = np.asarray(grid, dtype=np.int64), np.full(N, 1.0 / max(grid))
    head = (N, ne.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), dp(h))
    nelem, nnode = int(np.prod(grid)), int(np.prod([g + 1 for g in grid]))
    n = nnode * N
    gen = torch.Generator("cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
    S, KS = rand(3 * k, n) - 0.5, rand(3 * k, n) - 0.5
    out = torch.empty((2 * k, n), dtype=torch.float64, device="cuda")
    m = 0.2 + 0.8 * rand(nelem)
    mask = torch.zeros(nnode, dtype=torch.uint8, device="cuda")
    mask[:nnode // (grid[0] + 1)] = 7 if N == 3 else 3
    stream = None
    for c in (1, k):
        ms = _time(lambda: _lib.check(lib.vfem_modal_mass_apply(*head, p(m), p(mask), c, p(S), p(out), stream)), reps, warmup)
        _line("mass_apply", grid, ms, (2 * c * n + nelem) * 8 + nnode, columns=c)
    G = torch.empty((3 * k, 3 * k), dtype=torch.float64, device="cuda")
    for ka in (k, 3 * k):
        ms = _time(lambda: _lib.check(lib.vfem_block_gram(n, ka, p(S), ka, p(KS), p(G), None, stream)), reps, warmup)
        _line("gram", grid, ms, 2 * ka * n * 8, ka=ka, kb=ka, bytes_read_as_built=(-(-ka // 8)) ** 2 * 16 * n * 8)
    C = np.ascontiguousarray(np.random.default_rng(3).standard_normal((3 * k, 2 * k)))
    ms = _time(lambda: _lib.check(lib.vfem_block_combine(n, 3 * k, 2 * k, p(S), dp(C), p(out), stream)), reps, warmup)
    _line("combine", grid, ms, 5 * k * n * 8, kin=3 * k, kout=2 * k, launches=-(-2 * k // 12))
    modes = min(k, 8)
    ke = N * 2 ** N
    K0 = np.random.default_rng(4).standard_normal((ke, ke))
    K0 = np.ascontiguousarray(K0 + K0.T)
    co = np.ones(8)
    g = torch.empty(nelem, dtype=torch.float64, device="cuda")
    ms = _time(lambda: _lib.check(lib.vfem_modal_gradient(*head, modes, dp(K0), dp(co), dp(co), p(m), p(m), p(S), p(g), stream)), reps, warmup)
    _line("gradient", grid, ms, (modes * n + 3 * nelem) * 8, modes=modes, includes="the upload of K0 and a synchronise")


def _solve(grid, k, tol):
    from ndr_amd import modal
    from ndr_amd import pyVoxelFEM as pv
    N = len(grid)
    sim = pv.TensorProductSimulator([1] * N, [np.zeros(N), np.asarray(grid, dtype=np.float64) / max(grid)], list(grid))
    sim.E_min = 1e-3
    sim.setElementDensities(np.random.default_rng(0).uniform(0.2, 1.0, size=int(np.prod(grid))))
    fixed = np.zeros([g + 1 for g in grid] + [N], dtype=bool)
    fixed[0] = True
    sim.dirichletMask = fixed.reshape(-1, N)
    levels = 0
    e = list(grid)
    while all(v % 2 == 0 and v >= 8 for v in e):
        e = [v // 2 for v in e]
        levels += 1
    mg = sim.multigridSolver(levels)
    for rep in ("cold", "again"):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lam, Phi, info = modal.eigenmodes(sim, k, tol=tol, preconditioner=mg)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        print(json.dumps({"tool": "modal_time", "solve": rep, "grid": list(grid), "modes": k, "block": info["blockSize"], "tol": tol,
                          "levels": levels, "iterations": info["iterations"], "droppedP": info["droppedP"], "seconds": round(seconds, 4),
                          "lambda": [float(v) for v in lam], "residual": float(info["residuals"].max())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs="+", default=[256, 256, 128])
    ap.add_argument("--block", type=int, default=6)
    ap.add_argument("--solve-grid", type=int, nargs="+", default=[64, 32, 32])
    ap.add_argument("--modes", type=int, default=4)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    _kernels(tuple(a.grid), a.block, a.reps, a.warmup)
    _solve(tuple(a.solve_grid), a.modes, a.tol)


if __name__ == "__main__":
    main()
