"""LangelaarFilter timing: apply and backprop (HIP events, median of --reps after --warmup) at 256^3 and 512 x 256 x 256.
Prints one JSON line.  The whole run is bounded by --timeout seconds (SIGALRM ends it with exit status 124).

    python tools/langelaar_time.py [--reps 20] [--warmup 3] [--timeout 300]
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


def _expire(signum, frame):
    print(json.dumps({"tool": "langelaar_time", "error": "timeout"}), flush=True)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    from ndr_amd import pyVoxelFEM as pv
    res = {"tool": "langelaar_time", "layers_per_launch": 8, "grids": {}}
    for dims in ((256, 256, 256), (512, 256, 256)):
        n = int(np.prod(dims))
        gen = torch.Generator("cuda").manual_seed(1)
        x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
        g = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
        f = pv.LangelaarFilter()
        f._set_grid(dims)
        f.apply_dev(x)
        t_apply = _time(lambda: f.apply_dev(x), a.reps, a.warmup)
        t_back = _time(lambda: f.backprop_dev(g, x), a.reps, a.warmup)
        res["grids"]["x".join(map(str, dims))] = {
            "apply_ms": round(t_apply, 4), "backprop_ms": round(t_back, 4), "launches_per_pass": -(-dims[2] // 8),
            # compulsory HBM traffic: apply reads in, writes out + smax; backprop reads g, vars, out, smax, writes grad
            "apply_min_bytes": 3 * 8 * n, "backprop_min_bytes": 5 * 8 * n,
        }
        del x, g, f
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
