"""Heat-conduction solver timing: the multigrid-preconditioned CG of ndr_amd.thermal beside the Jacobi-preconditioned one, on the same
problem in the same run.  Prints one JSON line per measurement and writes them all to --out.  The whole run is bounded by --timeout
seconds (SIGALRM ends it with exit status 124).

    python tools/thermal_mg_time.py [--grids 256x256x128,128x128x64] [--reps 20] [--warmup 3] [--timeout 900] [--out profiles/thermal_mg_time.json]

Two data sets per grid, both with unit voxels, unit conductivity, a unit volumetric source and the sink on the middle third of the
face x = 0 (the problem of tests/thermal_cpu.pcg_fixture):
  random     rho uniform in [0.05, 1], p = 3, k_min = 1e-3
  design     a 0/1 design (uniform noise, two box filters of radius 4, cut at its median), p = 3, k_min = 1e-3: a contrast of 1000
Timed through the entry points with HIP events, median of --reps after --warmup calls: the hierarchy's build, one level-0 sweep, one
apply, one V-cycle, one PCG iteration of either kind (the difference of an 8- and a 4-iteration call, over 4), and both solves to
tol 1e-8 (median of 3 after one warm-up call, with their iteration counts).
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

LINES = []


def _emit(d):
    d = dict(tool="thermal_mg_time", **d)
    LINES.append(d)
    print(json.dumps(d), flush=True)


def _expire(signum, frame):
    print(json.dumps({"tool": "thermal_mg_time", "error": "timeout"}), flush=True)
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
    return round(float(np.median(ms)), 4)


def _densities(grid, data):
    nelem = int(np.prod(grid))
    if data == "random":
        return torch.from_numpy(np.random.default_rng(1600 + nelem).uniform(0.05, 1.0, size=nelem)).cuda()
    gen = torch.Generator("cuda").manual_seed(1600 + nelem)
    f = torch.rand((1, 1) + tuple(grid), dtype=torch.float32, device="cuda", generator=gen)
    pool = torch.nn.functional.avg_pool3d if len(grid) == 3 else torch.nn.functional.avg_pool2d
    for _ in range(2):
        f = pool(f, 9, stride=1, padding=4, count_include_pad=False)
    f = f.reshape(-1)
    return (f > f.median()).to(torch.float64)


def _grid(grid, reps, warmup):
    from ndr_amd import _lib, thermal
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    N = len(grid)
    for data in ("random", "design"):
        sim = thermal.HeatConductionSimulator([np.zeros(N), np.asarray(grid, dtype=np.float64)], list(grid))
        sim.setElementDensities(_densities(grid, data))
        idx = np.stack(np.meshgrid(*[np.arange(n + 1) for n in grid], indexing="ij"), axis=-1).reshape(-1, N)
        mask = idx[:, 0] == 0
        for d in range(1, N):
            mask &= (3 * idx[:, d] >= grid[d]) & (3 * idx[:, d] <= 2 * grid[d])
        del idx
        sim.fixedTemperatureMask = mask
        sim.setHeatSources(volumetric=1.0)
        Q = sim.buildLoadVector_device()
        base = dict(grid=list(grid), data=data, nodes=sim.numNodes())

        def build():
            sim._drop_multigrid()
            sim._multigrid()

        t_build = _time(build, max(3, reps // 4), 1)
        h = sim._multigrid()
        _emit(dict(base, path="hierarchy_build", ms=t_build, levels=sim.multigridLevels(), bytes=sim.multigridBytes()))
        X, Y = torch.zeros_like(Q), torch.empty_like(Q)
        _emit(dict(base, path="level0_sweep", ms=_time(lambda: _lib.check(lib.vfem_thermal_mg_smooth(h, 0, p(X), p(Q), 1, None)), reps, warmup)))
        _emit(dict(base, path="level0_apply", ms=_time(lambda: _lib.check(lib.vfem_thermal_mg_level_apply(h, 0, p(Q), p(Y), None)), reps, warmup)))
        if len(sim.multigridLevels()) > 1:
            n1 = int(np.prod(np.asarray(sim.multigridLevels()[1]) + 1))
            X1, B1 = torch.zeros(n1, dtype=torch.float64, device="cuda"), torch.ones(n1, dtype=torch.float64, device="cuda")
            _emit(dict(base, path="level1_sweep", ms=_time(lambda: _lib.check(lib.vfem_thermal_mg_smooth(h, 1, p(X1), p(B1), 1, None)), reps, warmup)))
        for s in (1, 2):
            _emit(dict(base, path="vcycle", smoothing=s, ms=_time(lambda: _lib.check(lib.vfem_thermal_mg_vcycle(h, p(Q), p(Y), s, None)), reps, warmup)))
        def capped(pre, iters):
            try:
                sim.pcg_device(Q, None, 1e-30, iters, pre)
            except RuntimeError:
                pass                                                    # "not converged after ...": the cap is the point

        for pre in ("multigrid", "jacobi"):
            t4, t8 = _time(lambda: capped(pre, 4), max(3, reps // 4), 1), _time(lambda: capped(pre, 8), max(3, reps // 4), 1)
            _emit(dict(base, path="pcg_iteration", preconditioner=pre, ms_4_iterations=t4, ms_8_iterations=t8, ms_per_iteration=round((t8 - t4) / 4.0, 4)))
        solves = {}
        for pre in ("multigrid", "jacobi"):
            x = [None]

            def solve():
                x[0] = sim.pcg_device(Q, None, 1e-8, 100000, pre)

            ms = _time(solve, 3, 1)
            true = float((Q - sim.applyK_device(x[0])).norm() / Q.norm())
            solves[pre] = dict(ms=ms, iterations=sim.last_iterations, x=x[0])
            _emit(dict(base, path="solve_to_1e-8", preconditioner=pre, ms=ms, iterations=sim.last_iterations,
                       relative_residual=sim.last_relative_residual, true_relative_residual=true))
        agree = float((solves["multigrid"]["x"] - solves["jacobi"]["x"]).abs().max() / solves["jacobi"]["x"].abs().max())
        _emit(dict(base, path="multigrid_against_jacobi", jacobi_over_multigrid_time=round(solves["jacobi"]["ms"] / solves["multigrid"]["ms"], 2),
                   jacobi_over_multigrid_iterations=round(solves["jacobi"]["iterations"] / solves["multigrid"]["iterations"], 1),
                   solutions_differ_by=agree, multigrid_is_faster=bool(solves["multigrid"]["ms"] < solves["jacobi"]["ms"])))
        del solves, sim
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=str, default="256x256x128,128x128x64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "thermal_mg_time.json"))
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    for name in [s for s in a.grids.split(",") if s]:
        _grid(tuple(int(v) for v in name.split("x")), a.reps, a.warmup)
    with open(a.out, "w") as f:
        json.dump({"tool": "thermal_mg_time", "note": "one run, one box", "measurements": LINES}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
