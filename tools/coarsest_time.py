"""Times of the two exact coarsest-level solvers of the tuned hierarchy (MultigridSolver1_1_1.coarsestSolver): the dense inverse
(dense_spd.hip) and the plane-block tridiagonal Cholesky (plane_spd.hip).

  update   setElementDensities + updateElementStiffnessMatrices: the Galerkin operators and the coarsest factorisation, which
           dominates on the grids below (one coarsening level above a small fine grid)
  solve    one coarsestSolve_device on a random right-hand side
  pcg      a whole full-multigrid PCG solve to --tol, operator update included

Device events around the work on the current stream, every shape warmed up once, the median of --reps runs (a run that takes
more than --budget seconds is repeated only twice).  One JSON line per measurement, then the table of DESIGN section 3.2.

  python tools/coarsest_time.py                       all cases: coarsest 17x9x9, 33x17x17, 65x33x33 nodes and PCG on 256x128x128
  python tools/coarsest_time.py --cases 17x9x9,pcg
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ndr_amd import pyVoxelFEM as pv  # noqa: E402

MATERIAL = os.path.join(ROOT, "VoxelFEM", "examples", "materials", "B9Creator.material")
BC = os.path.join(ROOT, "bcs", "3d", "cantilever_flexion.bc")
# coarsest node grid -> (fine elements, coarsening levels, modes)
CASES = {"17x9x9": ((32, 16, 16), 1, ("dense", "planes")),
         "33x17x17": ((64, 32, 32), 1, ("dense", "planes")),
         "65x33x33": ((128, 64, 64), 1, ("planes",))}
PCG_GRID, PCG_LEVELS = (256, 128, 128), 3


def simulator(ne):
    t = pv.TensorProductSimulator([1, 1, 1], [np.zeros(3), np.array([2.0, 1.0, 1.0])], list(ne))
    t.readMaterial(MATERIAL)
    t.applyDisplacementsAndLoadsFromFile(BC)
    t.E_0, t.E_min, t.gamma = 1.0, 1e-4, 3.0
    return t


def timed(fn, reps, budget):
    """median device time of fn() in seconds, and the number of runs behind it"""
    out = []
    while len(out) < reps:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
        if out[-1] > budget and len(out) >= 2:
            break
    return statistics.median(out), len(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(list(CASES) + ["pcg"]))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=5.0)
    ap.add_argument("--tol", type=float, default=1e-8)
    args = ap.parse_args()
    rows = []

    def report(**kw):
        print(json.dumps(kw), flush=True)
        rows.append(kw)

    for name in [c for c in args.cases.split(",") if c in CASES]:
        ne, levels, modes = CASES[name]
        rho = np.random.default_rng(1).uniform(0.1, 1.0, int(np.prod(ne)))
        for mode in modes:
            t = simulator(ne)
            mg = t.multigridSolver(levels)
            mg.coarsestSolver = mode
            n = mg.getSimulator(levels).numNodes() * 3

            def update():
                t.setElementDensities(rho)
                mg.updateElementStiffnessMatrices()

            update()                                                        # warm-up: code objects, workspaces
            t_up, n_up = timed(update, args.reps, args.budget)
            b = torch.from_numpy(np.random.default_rng(2).standard_normal((n // 3, 3))).cuda()
            mg.coarsestSolve_device(b)
            t_so, n_so = timed(lambda: [mg.coarsestSolve_device(b) for _ in range(10)], args.reps, args.budget)
            report(case=name, dofs=n, mode=mode, update_s=t_up, update_runs=n_up, solve_s=t_so / 10, solve_runs=n_so,
                   bytes=mg.coarsestBytes())
            del mg, t
            torch.cuda.empty_cache()
    if "pcg" in args.cases.split(","):
        rho = np.random.default_rng(1).uniform(0.1, 1.0, int(np.prod(PCG_GRID)))
        for mode in ("dense", "planes"):
            t = simulator(PCG_GRID)
            mg = t.multigridSolver(PCG_LEVELS)
            mg.coarsestSolver = mode
            f = t.buildLoadVector_device()
            u0 = torch.zeros_like(f)

            def solve():
                t.setElementDensities(rho)
                mg.preconditionedConjugateGradient_device(u0, f, 200, args.tol, fullMultigrid=True)

            solve()
            t0 = time.perf_counter()
            t_pcg, n_pcg = timed(solve, args.reps, args.budget)
            report(case="pcg %dx%dx%d, %d levels" % (PCG_GRID + (PCG_LEVELS,)), mode=mode, pcg_s=t_pcg, pcg_runs=n_pcg,
                   iterations=mg.last_iterations, relative_residual=mg.last_relative_residual, bytes=mg.coarsestBytes(),
                   wall_s_all_runs=time.perf_counter() - t0)
            del mg, t
            torch.cuda.empty_cache()
    print("\n| case | mode | update | solve | whole PCG | storage |\n|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s | %s | %s | %s | %.2f GB |" % (
            r["case"] + (" (%d dofs)" % r["dofs"] if "dofs" in r else ""), r["mode"],
            "%.1f ms" % (r["update_s"] * 1e3) if "update_s" in r else "",
            "%.3f ms" % (r["solve_s"] * 1e3) if "solve_s" in r else "",
            "%.2f s, %d iterations" % (r["pcg_s"], r["iterations"]) if "pcg_s" in r else "", r["bytes"] / 1e9))


if __name__ == "__main__":
    main()
