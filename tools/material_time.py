"""Time of the finest-level apply, one level-0 Gauss-Seidel sweep and one multigrid-preconditioned CG solve for an isotropic, an
orthotropic and an anisotropic elasticity tensor:  python tools/material_time.py [nx ny nz]   (default 256 128 128)

Isotropic and orthotropic tensors launch the same kernels (all VFEM_PATH_* flags set), the anisotropic one the general kernels
(k_apply_gather, the coefficient-table row sweeps, level 1 per incident element).  Device events around a synchronised window; every
shape is warmed up; the three materials alternate inside each of three rounds and the median round is reported with the spread
(min .. max), so that a difference between materials can be told from the spread of the box.  Prints one JSON line at the end."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import BC_CANTILEVER  # noqa: E402
from ndr_amd import ElasticityTensor, _lib, pyVoxelFEM as pv  # noqa: E402
from ndr_amd.pyVoxelFEM import _ptr, _stream  # noqa: E402

MATERIALS = os.path.join(ROOT, "tests", "golden", "materials")
ROUNDS, APPLY_REPS, SWEEP_REPS, LEVELS, PCG_TOL, PCG_MAX = 3, 20, 10, 3, 1e-6, 200


def timed(fn, reps):
    """milliseconds per call of fn over `reps` calls, device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ne = tuple(int(a) for a in sys.argv[1:4]) or (256, 128, 128)
    lib = _lib.load()
    tensors = {"isotropic": ElasticityTensor(1.0, 0.3),
               "orthotropic": ElasticityTensor(os.path.join(MATERIALS, "orthotropic_3d.material")),
               "anisotropic": ElasticityTensor(os.path.join(MATERIALS, "anisotropic_3d.material"))}
    sims = {}
    for name, tensor in tensors.items():
        t = pv.TensorProductSimulator([1, 1, 1], [np.zeros(3), np.array([2.0, 1.0, 1.0])], list(ne))
        t.ETensor = tensor
        t.applyDisplacementsAndLoadsFromFile(BC_CANTILEVER)
        t.E_0, t.E_min, t.gamma = 1.0, 1e-4, 3.0
        g = torch.Generator(device="cuda").manual_seed(88)
        t.setElementDensities(torch.rand(t.numElements(), dtype=torch.float64, device="cuda", generator=g))
        mg = t.multigridSolver(LEVELS)
        mg.updateElementStiffnessMatrices()
        u = torch.randn((t.numNodes(), 3), dtype=torch.float64, device="cuda", generator=g)
        b = torch.randn((t.numNodes(), 3), dtype=torch.float64, device="cuda", generator=g)
        sims[name] = (t, mg, u, b, torch.empty_like(u), t.buildLoadVector_device())

    def apply(name):
        t, mg, u, b, out, f = sims[name]
        return lambda: _lib.check(lib.vfem_sim_apply_k(t._h, _ptr(u), _ptr(out), 0, _stream()))

    def sweep(name):
        t, mg, u, b, out, f = sims[name]
        x = u.clone()
        return lambda: _lib.check(lib.vfem_mg_smooth_sweeps(mg._h, 0, _ptr(x), _ptr(b), 1, 1, _stream()))

    def pcg(name):
        t, mg, u, b, out, f = sims[name]
        return lambda: mg.preconditionedConjugateGradient_device(torch.zeros_like(f), f, PCG_MAX, PCG_TOL, None, 1, 2, True)

    res = {name: {"paths": int(lib.vfem_mg_tensor_paths(sims[name][1]._h)), "apply_ms": [], "sweep_ms": [], "pcg_ms": [],
                  "pcg_iterations": 0} for name in sims}
    for name in sims:                         # warm-up of every shape and kernel the timed windows use
        timed(apply(name), 2)
        timed(sweep(name), 2)
        timed(pcg(name), 1)
    for _ in range(ROUNDS):
        for name in sims:                     # the materials alternate inside a round
            res[name]["apply_ms"].append(timed(apply(name), APPLY_REPS))
            res[name]["sweep_ms"].append(timed(sweep(name), SWEEP_REPS))
            res[name]["pcg_ms"].append(timed(pcg(name), 1))
            res[name]["pcg_iterations"] = sims[name][1].last_iterations
    print("grid %dx%dx%d, %d coarsening levels, PCG to %g" % (ne + (LEVELS, PCG_TOL)))
    for name, r in res.items():
        line = "%-12s paths %2d" % (name, r["paths"])
        for key in ("apply_ms", "sweep_ms", "pcg_ms"):
            v = sorted(r[key])
            line += "   %s %9.3f (%.3f .. %.3f)" % (key[:-3], v[len(v) // 2], v[0], v[-1])
        print(line + "   %d iterations, %.2f ms each" % (r["pcg_iterations"], sorted(r["pcg_ms"])[ROUNDS // 2] / max(r["pcg_iterations"], 1)))
    print(json.dumps({"grid": list(ne), "levels": LEVELS, "pcg_tol": PCG_TOL, "materials": res}))


if __name__ == "__main__":
    main()
