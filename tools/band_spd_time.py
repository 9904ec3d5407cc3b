"""Direct-solve timing (band_spd.hip) of TensorProductSimulator.solve_device at 2-D 300x100 (MBB) and 250x125 (bridge), the
reference's --mgl 0 runs, and 3-D 45x21x21 and 64x32x32 (bridge), degree 1, random densities.  The first solve after a density
change assembles, factorises and solves; a repeated solve only solves.  HIP events, median of --reps.  The assembly kernel's own
time comes from a kernel trace of this tool (k_band_assemble).  Prints one JSON line; the run is bounded by --timeout seconds
(SIGALRM ends it with exit status 124).

    python tools/band_spd_time.py [--reps 3] [--timeout 900]
"""
import argparse
import json
import os
import signal
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MATERIAL = os.path.join(ROOT, "VoxelFEM", "examples", "materials", "B9Creator.material")
CASES = [("2d_mbb_300x100", [300, 100], ([0, 0], [3, 1]), "bcs/2d/mbb_beam.bc"),
         ("2d_bridge_250x125", [250, 125], ([0, 0], [2, 1]), "bcs/2d/bridge.bc"),
         ("3d_bridge_45x21x21", [45, 21, 21], ([0, 0, 0], [2, 1, 1]), "bcs/3d/bridge.bc"),
         ("3d_bridge_64x32x32", [64, 32, 32], ([0, 0, 0], [2, 1, 1]), "bcs/3d/bridge.bc")]


def _expire(signum, frame):
    print(json.dumps({"tool": "band_spd_time", "error": "timeout"}), flush=True)
    os._exit(124)


def _time(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    from ndr_amd import band
    from ndr_amd import pyVoxelFEM as pv
    res = {"tool": "band_spd_time", "cases": {}}
    for name, ne, dom, bc in CASES:
        t = pv.TensorProductSimulator([1] * len(ne), dom, ne)
        t.readMaterial(MATERIAL)
        t.applyDisplacementsAndLoadsFromFile(os.path.join(ROOT, bc))
        t.E_0, t.E_min, t.gamma = 1.0, 1e-4, 3.0
        gen = torch.Generator("cuda").manual_seed(1)
        rho = 0.1 + 0.9 * torch.rand(t.numElements(), dtype=torch.float64, device="cuda", generator=gen)
        f = t.buildLoadVector_device()

        def refactor():
            t.setElementDensities(rho)          # a new operator version: the next solve assembles and factorises
            t.solve_device(f)

        full = _time(refactor, a.reps)
        solve = _time(lambda: t.solve_device(f), a.reps)
        n, w, nbytes = band.band_geometry(len(ne), 1, ne)
        nb = -(-n // 64)
        res["cases"][name] = {"n": n, "w": w, "band_bytes": nbytes, "tile_rows": nb,
                              "launches_per_factorisation": 1 + nb + 2 * (nb - 1), "launches_per_solve": 3,
                              "assemble_factor_solve_ms": round(full, 3), "solve_ms": round(solve, 3),
                              "assemble_factor_ms": round(full - solve, 3), "factorisations": t.numDirectFactorizations()}
        del t, rho, f
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
