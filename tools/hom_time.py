"""Periodic homogenisation timing: the batched cell-problem solve of an n^3 cell with a spherical void of radius 0.3 (one size per
run, so that every size runs under a time limit of its own), and the periodic apply alone.  Prints one JSON line.  The whole run
is bounded by --timeout seconds (SIGALRM ends it with exit status 124).

    python tools/hom_time.py --n 64 [--emin 1e-3] [--tol 1e-10] [--reps 20] [--warmup 3] [--timeout 300]
                             [--preconditioner jacobi|multigrid] [--smoothing 1] [--design]

With --preconditioner multigrid the line also holds the level sizes, the time to build the hierarchy (Galerkin products, inverted
diagonal blocks, the dense coarsest inverse; host wall time around a synchronised build, median), the device memory it holds and
the time of one V-cycle on all S columns (HIP events, median).  The whole-solve time includes the build.

With --design the line holds the microstructure-design figures of the same cell instead: the contracted gradient
(vfem_hom_tensor_gradient_contract, a dense and a bulk-modulus weight matrix) against vfem_hom_tensor_gradient followed by the einsum
that does the same contraction, both with the fixed cost of the call on a 2^3 cell alongside (HIP events, medians), the bytes each
writes, and one evaluation of HomogenizedTensorObjective with its gradient as a whole (solve, tensor, contracted gradient; host
wall time around a synchronised call, median of 3).

The apply is timed through vfem_hom_apply (HIP events, median); that call also uploads its element tables and synchronises, so
the same call on a 2^3 cell is timed as the fixed cost and subtracted.  Compulsory HBM traffic of one apply: read W, write W_out
(S x nodes x 3 doubles each) and read the moduli once; the fraction is of the 8 TB/s peak.
"""
import argparse
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
    print(json.dumps({"tool": "hom_time", "error": "timeout"}), flush=True)
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


def _cell(n, emin):
    from ndr_amd import pyVoxelFEM as pv
    sim = pv.TensorProductSimulator([1, 1, 1], [np.zeros(3), np.ones(3)], [n, n, n])
    sim.ETensor = pv.ElasticityTensor(1.0, 0.3, dim=3)
    sim.E_0, sim.E_min, sim.gamma = 1.0, emin, 1.0
    c = (np.arange(n) + 0.5) / n - 0.5
    r2 = c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2
    sim.setElementDensities((r2 > 0.3 ** 2).astype(np.float64).reshape(-1))
    return sim


def _apply_ms(sim, reps, warmup):
    from ndr_amd import _lib
    from ndr_amd import homogenization as hom
    from ndr_amd import pyVoxelFEM as pv
    c = hom._Cell(sim)
    gen = torch.Generator("cuda").manual_seed(1)
    w = torch.randn((c.S, c.pn, c.N), dtype=torch.float64, device="cuda", generator=gen)
    out = torch.empty_like(w)
    lib = _lib.load()
    return _time(lambda: _lib.check(lib.vfem_hom_apply(*c.head(), pv._ptr(w), pv._ptr(out), pv._stream())), reps, warmup), c


def _hierarchy_figures(sim, a):
    from ndr_amd import homogenization as hom
    c = hom._Cell(sim)
    build = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = hom._Hierarchy(c)
        torch.cuda.synchronize()
        build.append(time.perf_counter() - t0)
        h.close()
    h = hom._Hierarchy(c)
    gen = torch.Generator("cuda").manual_seed(2)
    B = torch.randn((c.S, c.pn, c.N), dtype=torch.float64, device="cuda", generator=gen)
    B[:, 0] = 0.0
    vcycle_ms = _time(lambda: h.vcycle(B, a.smoothing), a.reps, a.warmup)
    out = {"smoothing": a.smoothing, "levels": h.dims, "hierarchy_build_seconds": round(float(np.median(build)), 4),
           "hierarchy_bytes": h.bytes, "vcycle_ms": round(vcycle_ms, 4)}
    h.close()
    return out


def _design_figures(sim, a):
    from ndr_amd import homogenization as hom
    from ndr_amd import microstructure as mic

    def gradient_ms(cell_sim):
        c = hom._Cell(cell_sim)
        gen = torch.Generator("cuda").manual_seed(3)
        Wp = torch.randn((c.S, c.pn, c.N), dtype=torch.float64, device="cuda", generator=gen)
        dense = np.random.default_rng(4).standard_normal((c.S, c.S))
        bulk = np.zeros((c.S, c.S))
        bulk[:3, :3] = 1.0
        Cd = torch.from_numpy(dense).cuda()
        full = lambda: hom._gradient_periodic(c, Wp, True)
        return {"contracted_dense_ms": _time(lambda: hom._contracted(c, Wp, dense), a.reps, a.warmup),
                "contracted_bulk_ms": _time(lambda: hom._contracted(c, Wp, bulk), a.reps, a.warmup),
                "blocks_ms": _time(full, a.reps, a.warmup),
                "blocks_then_einsum_ms": _time(lambda: torch.einsum("qr,eqr->e", Cd, full()), a.reps, a.warmup)}, c

    big, c = gradient_ms(sim)
    small, _ = gradient_ms(_cell(2, a.emin))
    obj = mic.HomogenizedTensorObjective(sim, np.pad(np.ones((3, 3)), (0, 3)), tol=a.tol, preconditioner=a.preconditioner,
                                         smoothing=a.smoothing, skipSolve=True)
    whole = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        obj.updateCache(None)
        J = obj.evaluate()
        g = obj.gradient_device()
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    out = {k: round(v, 4) for k, v in big.items()}
    out.update({"fixed_cost_" + k: round(v, 4) for k, v in small.items()})
    out.update({"contracted_bytes_written": 8 * c.pn, "blocks_bytes_written": 8 * c.S * c.S * c.pn,
                "objective_and_gradient_seconds": round(float(np.median(whole)), 4), "iterations": list(hom.last_iterations),
                "J": J, "gradient_max": float(g.abs().max()), "gradient_nowhere_positive": bool((g <= 0).all())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--emin", type=float, default=1e-3)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--preconditioner", choices=["jacobi", "multigrid"], default="jacobi")
    ap.add_argument("--smoothing", type=int, default=1)
    ap.add_argument("--design", action="store_true")
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    from ndr_amd import homogenization as hom
    sim = _cell(a.n, a.emin)
    how = dict(preconditioner=a.preconditioner, smoothing=a.smoothing)
    hom.solveCellProblems_device(_cell(4, a.emin), tol=a.tol, **how)    # library and allocator warm
    if a.design:
        print(json.dumps({"tool": "hom_time", "mode": "design", "n": a.n, "E_min": a.emin, "tol": a.tol, "void_radius": 0.3,
                          "preconditioner": a.preconditioner, **_design_figures(sim, a)}), flush=True)
        return
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    W = hom.solveCellProblems_device(sim, tol=a.tol, **how)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    its = list(hom.last_iterations)
    extra = {}
    if a.preconditioner == "multigrid":
        extra = _hierarchy_figures(sim, a)
    Eh = hom.homogenizedElasticityTensor_device(W, sim).D
    t_apply, c = _apply_ms(sim, a.reps, a.warmup)
    t_fixed, _ = _apply_ms(_cell(2, a.emin), a.reps, a.warmup)
    nbytes = (2 * c.S * c.N + 1) * 8 * c.pn
    kernel_ms = max(t_apply - t_fixed, 1e-6)
    print(json.dumps({
        "tool": "hom_time", "n": a.n, "E_min": a.emin, "tol": a.tol, "void_radius": 0.3, "preconditioner": a.preconditioner, **extra,
        "iterations": its, "relative_residuals": list(hom.last_relative_residuals),
        "solve_seconds_all_cases": round(seconds, 4), "ms_per_iteration": round(1e3 * seconds / max(its), 4),
        "Eh_diag": [round(float(v), 6) for v in np.diag(Eh)],
        "apply_call_ms": round(t_apply, 4), "apply_fixed_cost_ms": round(t_fixed, 4), "apply_kernel_ms": round(kernel_ms, 4),
        "apply_min_bytes": nbytes, "apply_TBps": round(nbytes / kernel_ms * 1e-9, 3),
        "apply_fraction_of_hbm_peak": round(nbytes / (kernel_ms * 1e-3) / HBM_PEAK, 3),
    }), flush=True)


if __name__ == "__main__":
    main()
