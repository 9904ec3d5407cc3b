"""Element-stress kernel timing: the von Mises field (vm only), the adjoint load and the density gradient of the p-norm measure on
one grid (default 512 x 256 x 256), next to their yardsticks on the same machine in the same run: vfem_sim_compliance_gradient (the
same reads of u, one double written per element, far more arithmetic) for the field and gradient kernels, vfem_sim_apply_k
(node-wise, reads u and the moduli, writes a node vector) for the adjoint load.  Prints one JSON line.  The whole run is bounded by
--timeout seconds (SIGALRM ends it with exit status 124).

    python tools/stress_time.py [--n 512 256 256] [--reps 20] [--warmup 3] [--P 8] [--timeout 300]

Every figure is the median of --reps calls timed by HIP events, the five calls taken in turn within each repetition so that drift
hits all alike.  vfem_stress_pnorm_gradient also uploads K0 and synchronises; the same call on a 2 x 2 x 2 grid is timed as its
fixed cost and subtracted.  Compulsory HBM traffic: fields read u and m and write vm; the adjoint load reads u and m, writes and reads its scratch (S doubles per element) and writes a;
the gradient reads u, lambda, m, dm, dE and writes g.  The fraction is of the 8 TB/s peak.
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
    print(json.dumps({"tool": "stress_time", "error": "timeout"}), flush=True)
    os._exit(124)


def _problem(ne, P, seed):
    """a simulator of the grid with random densities, a random displacement and adjoint, and the calls to time"""
    from ndr_amd import _lib
    from ndr_amd import pyVoxelFEM as pv
    from ndr_amd import stress
    lib = _lib.load()
    sim = pv.TensorProductSimulator([1, 1, 1], [np.zeros(3), np.asarray(ne, dtype=np.float64) / max(ne)], list(ne))
    sim.ETensor = pv.ElasticityTensor(1.0, 0.3, dim=3)
    sim.E_0, sim.E_min, sim.gamma = 1.0, 1e-3, 3.0
    gen = torch.Generator("cuda").manual_seed(seed)
    nel, nn = sim.numElements(), sim.numNodes()
    sim.setElementDensities(0.2 + 0.8 * torch.rand(nel, dtype=torch.float64, device="cuda", generator=gen))
    u = torch.randn((nn, 3), dtype=torch.float64, device="cuda", generator=gen)
    lam = torch.randn((nn, 3), dtype=torch.float64, device="cuda", generator=gen)
    g = stress._Grid(sim)
    m, dm = g.multipliers(0.5)
    dE = dm.clone()
    vm = torch.empty(nel, dtype=torch.float64, device="cuda")
    a = torch.empty((nn, 3), dtype=torch.float64, device="cuda")
    work = torch.empty((nel, 6), dtype=torch.float64, device="cuda")
    grad = torch.empty(nel, dtype=torch.float64, device="cuda")
    yard_g = torch.empty(nel, dtype=torch.float64, device="cuda")
    yard_a = torch.empty((nn, 3), dtype=torch.float64, device="cuda")
    K0 = np.ascontiguousarray(sim.fullDensityElementStiffnessMatrix())
    p, st = pv._ptr, pv._stream
    fields = lambda: _lib.check(lib.vfem_stress_fields(*g.head(), p(m), p(u), None, None, p(vm), st()))
    fields()
    J, vmax = stress._pnorm(vm, P)
    calls = {
        "fields_vm": fields,
        "adjoint_load": lambda: _lib.check(lib.vfem_stress_adjoint_load(*g.head(), p(m), p(u), J, P, None, p(work), p(a), st())),
        "gradient": lambda: _lib.check(lib.vfem_stress_pnorm_gradient(*g.head(), K0.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), p(m),
                                                                      p(dm), p(dE), p(u), p(lam), J, P, p(grad), st())),
        "yardstick_compliance_gradient": lambda: _lib.check(lib.vfem_sim_compliance_gradient(sim._h, p(u), p(yard_g), st())),
        "yardstick_apply_k": lambda: _lib.check(lib.vfem_sim_apply_k(sim._h, p(u), p(yard_a), 0, st())),
    }
    keep = (sim, g, u, lam, m, dm, dE, vm, a, work, grad, yard_g, yard_a, K0)
    return calls, keep, dict(J=J, vmax=vmax, nel=nel, nn=nn)


def _time_in_turn(calls, reps, warmup):
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs=3, default=[512, 256, 256])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--P", type=float, default=8.0)
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    small_calls, small_keep, _ = _problem((2, 2, 2), a.P, 1)
    fixed = _time_in_turn({"gradient": small_calls["gradient"]}, a.reps, a.warmup)["gradient"][0]
    calls, keep, info = _problem(tuple(a.n), a.P, 2)
    t = _time_in_turn(calls, a.reps, a.warmup)
    nel, nn = info["nel"], info["nn"]
    nbytes = {"fields_vm": 8 * (3 * nn + 2 * nel), "adjoint_load": 8 * (6 * nn + nel + 12 * nel), "gradient": 8 * (6 * nn + 4 * nel),
              "yardstick_compliance_gradient": 8 * (3 * nn + 2 * nel), "yardstick_apply_k": 8 * (6 * nn + nel)}
    out = {"tool": "stress_time", "n": list(a.n), "P": a.P, "reps": a.reps, "J": info["J"], "vmax": info["vmax"],
           "gradient_fixed_cost_ms": round(fixed, 4)}
    for k, (med, lo, hi) in t.items():
        kernel = max(med - fixed, 1e-6) if k == "gradient" else med
        out[k] = {"ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4), "kernel_ms": round(kernel, 4),
                  "min_bytes": nbytes[k], "TBps": round(nbytes[k] / kernel * 1e-9, 3),
                  "fraction_of_hbm_peak": round(nbytes[k] / (kernel * 1e-3) / HBM_PEAK, 3)}
    out["fields_over_yardstick"] = round(out["fields_vm"]["kernel_ms"] / out["yardstick_compliance_gradient"]["kernel_ms"], 3)
    out["gradient_over_yardstick"] = round(out["gradient"]["kernel_ms"] / out["yardstick_compliance_gradient"]["kernel_ms"], 3)
    out["adjoint_load_over_yardstick"] = round(out["adjoint_load"]["kernel_ms"] / out["yardstick_apply_k"]["kernel_ms"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
