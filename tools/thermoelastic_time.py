"""Thermo-elastic timing: the three coupling entry points of ndr_amd.thermoelastic and one whole coupled gradient on one grid, beside a
torch composition of the same sums.  Prints one JSON line per measurement and writes them all to --out (default
profiles/thermoelastic_time.json).  The whole run is bounded by --timeout seconds (SIGALRM ends it with exit status 124).

    python tools/thermoelastic_time.py [--grid 256 256 128] [--cases 4] [--reps 20] [--warmup 3] [--timeout 600] [--out FILE]

Each path is timed through its entry point (HIP events, median of --reps after --warmup calls), random data.  The load is an
asynchronous launch; the figures of the adjoint source and of the gradient include the upload of the coupling matrices and a
synchronise.  "Before" is what one would write without the kernels: the same sums as 2^N x 2^N torch slice additions over the node
and element grids (``torch_load``, ``torch_adjoint_source``, ``torch_gradient`` below), timed in the same run.  It is not the code
under test; the tool checks once that both agree to 1e-12 of the largest entry.

The whole coupled gradient is ``LoadCaseComplianceObjective._weighted_gradient`` on a state of random displacements and a solved
temperature: ``vfem_loads_gradient``, ``vfem_thermoelastic_gradient``, ``vfem_thermoelastic_adjoint_source``, one thermal adjoint solve
(multigrid-preconditioned CG to 1e-8, whose iteration count is reported) and ``vfem_thermal_gradient``.

Compulsory HBM traffic, from the shapes, n = dofs of a displacement vector, k = cases:
  load                  (nodes + elements + n) 8 bytes                 T, E, f_out       (+ n 8 + nodes with f_in and the mask)
  adjoint source        (k n + elements + nodes) 8 bytes               U, E, q           (+ nodes with the fixed mask)
  gradient              (k n + nodes + 2 elements) 8 bytes             U, T, dE, g_out   (+ elements 8 with g_in)
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
LINES = []


def _emit(line):
    LINES.append(line)
    print(json.dumps(line), flush=True)


def _expire(signum, frame):
    print(json.dumps({"tool": "thermoelastic_time", "error": "timeout"}), flush=True)
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


def _line(what, grid, ms, nbytes=None, **more):
    med, lo, hi = ms
    out = {"tool": "thermoelastic_time", "path": what, "grid": list(grid), "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)}
    if nbytes is not None:
        out.update(min_bytes=int(nbytes), TBps=round(nbytes / med * 1e-9, 3), fraction_of_hbm_peak=round(nbytes / (med * 1e-3) / HBM_PEAK, 3))
    out.update(more)
    _emit(out)
    return med


def _slices(N):
    """the slice of the node grid that local node n of every element occupies, axis 0 the most significant bit"""
    return [tuple(slice(1, None) if (n >> (N - 1 - d)) & 1 else slice(0, -1) for d in range(N)) for n in range(2 ** N)]


def torch_load(G, tref, E, T, grid):
    """sum_e E_e G (T_e - T_ref) as 2^N x 2^N slice additions; G a device tensor [ke, npe]"""
    N, sl = len(grid), _slices(len(grid))
    nn = tuple(g + 1 for g in grid)
    theta, Eg = (T - tref).reshape(nn), E.reshape(grid)
    f = torch.zeros(nn + (N,), dtype=torch.float64, device=T.device)
    for n in range(2 ** N):
        for m in range(2 ** N):
            f[sl[n]] += (Eg * theta[sl[m]]).unsqueeze(-1) * G[n * N:(n + 1) * N, m]
    return f.reshape(-1, N)


def torch_adjoint_source(a, G, E, U, grid):
    """sum_i a_i sum_e E_e G_i^T u_ie; G [cases, ke, npe], U [cases, nodes, N]"""
    N, sl = len(grid), _slices(len(grid))
    nn = tuple(g + 1 for g in grid)
    Eg = E.reshape(grid)
    q = torch.zeros(nn, dtype=torch.float64, device=E.device)
    for i in range(U.shape[0]):
        Ug = U[i].reshape(nn + (N,))
        for m in range(2 ** N):
            for n in range(2 ** N):
                q[sl[m]] += a[i] * Eg * (Ug[sl[n]] * G[i, n * N:(n + 1) * N, m]).sum(-1)
    return q.reshape(-1)


def torch_gradient(a, G, tref, dE, T, U, grid):
    """dE_e sum_i a_i u_ie^T G_i (T_e - T_ref,i)"""
    N, sl = len(grid), _slices(len(grid))
    nn = tuple(g + 1 for g in grid)
    s = torch.zeros(grid, dtype=torch.float64, device=T.device)
    for i in range(U.shape[0]):
        Ug, theta = U[i].reshape(nn + (N,)), (T - tref[i]).reshape(nn)
        for n in range(2 ** N):
            for m in range(2 ** N):
                s += a[i] * (Ug[sl[n]] * G[i, n * N:(n + 1) * N, m]).sum(-1) * theta[sl[m]]
    return dE * s.reshape(-1)


def _run(grid, cases, reps, warmup):
    from ndr_amd import _lib, loadcases, thermal, thermoelastic
    from ndr_amd import pyVoxelFEM as pv
    N = len(grid)
    h = np.full(N, 1.0 / max(grid))
    box = [np.zeros(N), np.asarray(grid) * h]
    sim = pv.TensorProductSimulator([1] * N, box, list(grid))
    sim.E_0, sim.E_min, sim.gamma = 1.0, 1e-3, 3.0
    nelem, nnode = sim.numElements(), sim.numNodes()
    n = nnode * N
    gen = torch.Generator("cuda").manual_seed(7)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device="cuda", generator=gen)
    rho = 0.2 + 0.8 * rand(nelem)
    sim.setElementDensities(rho)
    U, T = rand(cases, nnode, N) - 0.5, rand(nnode)
    a = np.ascontiguousarray([1.0 + 0.25 * i for i in range(cases)], dtype=np.float64)
    tref = np.ascontiguousarray([0.1 * i for i in range(cases)], dtype=np.float64)
    E = (1e-3 + rho ** 3.0 * (1.0 - 1e-3)).contiguous()
    dE = (3.0 * rho ** 2.0 * (1.0 - 1e-3)).contiguous()
    G = np.ascontiguousarray(np.stack([thermoelastic.couplingMatrix(sim, 0.01 * (1.0 + 0.1 * i)) for i in range(cases)]))
    Gd = torch.from_numpy(G).cuda()
    mask = loadcases._Grid(sim).mask
    f_in, f_out = rand(nnode, N) - 0.5, torch.empty((nnode, N), dtype=torch.float64, device="cuda")
    q, g_in, g_out = torch.empty(nnode, dtype=torch.float64, device="cuda"), rand(nelem), torch.empty(nelem, dtype=torch.float64, device="cuda")

    # the two agree (once, before anything is timed)
    agree = lambda got, want: float((got - want).abs().max() / want.abs().max())
    checks = {"load": agree(thermoelastic.thermalLoad_device(sim, G[0], T, tref[0], E=E, masked=False), torch_load(Gd[0], tref[0], E, T, grid)),
              "adjoint_source": agree(thermoelastic.adjointSource_device(sim, a, G, U, E=E), torch_adjoint_source(a, Gd, E, U, grid)),
              "gradient": agree(thermoelastic.couplingGradient_device(sim, a, G, tref, dE, T, U), torch_gradient(a, Gd, tref, dE, T, U, grid))}
    _emit({"tool": "thermoelastic_time", "grid": list(grid), "kernels_against_torch": checks})
    if max(checks.values()) > 1e-12:
        raise RuntimeError("the kernels and the torch composition disagree: %r" % (checks,))

    old_l = _line("torch_load", grid, _time(lambda: torch_load(Gd[0], tref[0], E, T, grid), reps, warmup), (nnode + nelem + n) * 8)
    old_q = _line("torch_adjoint_source", grid, _time(lambda: torch_adjoint_source(a, Gd, E, U, grid), reps, warmup),
                  (cases * n + nelem + nnode) * 8, cases=cases)
    old_g = _line("torch_gradient", grid, _time(lambda: torch_gradient(a, Gd, tref, dE, T, U, grid), reps, warmup),
                  (cases * n + nnode + 2 * nelem) * 8, cases=cases)

    # the entry points themselves (the Python wrappers build a grid object per call, which is host time between the two events)
    lib, head = _lib.load(), loadcases._Grid(sim).head()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    dp = lambda v: v.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    G1, a1, t1 = np.ascontiguousarray(G[0]), np.ascontiguousarray(a[:1]), np.ascontiguousarray(tref[:1])
    stream = None
    new_l = _line("load", grid, _time(lambda: _lib.check(lib.vfem_thermoelastic_load(*head, dp(G1), float(tref[0]), p(E), p(T), None, None, p(f_out),
                                                                                      stream)), reps, warmup), (nnode + nelem + n) * 8)
    f_io = f_in.clone()
    _line("load_masked_added_in_place", grid,
          _time(lambda: _lib.check(lib.vfem_thermoelastic_load(*head, dp(G1), float(tref[0]), p(E), p(T), p(mask), p(f_io), p(f_io), stream)),
                reps, warmup), (nnode + nelem + 2 * n) * 8 + nnode)
    new_q = _line("adjoint_source", grid,
                  _time(lambda: _lib.check(lib.vfem_thermoelastic_adjoint_source(*head, cases, dp(a), dp(G), p(E), p(U), None, p(q), stream)),
                        reps, warmup), (cases * n + nelem + nnode) * 8, cases=cases)
    _line("adjoint_source_one_case", grid,
          _time(lambda: _lib.check(lib.vfem_thermoelastic_adjoint_source(*head, 1, dp(a1), dp(G1), p(E), p(U), None, p(q), stream)), reps, warmup),
          (n + nelem + nnode) * 8, cases=1)
    new_g = _line("gradient", grid,
                  _time(lambda: _lib.check(lib.vfem_thermoelastic_gradient(*head, cases, dp(a), dp(G), dp(tref), p(dE), p(T), p(U), None, p(g_out),
                                                                           stream)), reps, warmup), (cases * n + nnode + 2 * nelem) * 8, cases=cases)
    _line("gradient_added", grid,
          _time(lambda: _lib.check(lib.vfem_thermoelastic_gradient(*head, cases, dp(a), dp(G), dp(tref), p(dE), p(T), p(U), p(g_in), p(g_out),
                                                                   stream)), reps, warmup), (cases * n + nnode + 3 * nelem) * 8, cases=cases)
    _line("gradient_one_case", grid,
          _time(lambda: _lib.check(lib.vfem_thermoelastic_gradient(*head, 1, dp(a1), dp(G1), dp(t1), p(dE), p(T), p(U), None, p(g_out), stream)),
                reps, warmup), (n + nnode + 2 * nelem) * 8, cases=1)
    _emit({"tool": "thermoelastic_time", "grid": list(grid), "cases": cases, "torch_load_over_load": round(old_l / new_l, 3),
           "torch_adjoint_source_over_adjoint_source": round(old_q / new_q, 3), "torch_gradient_over_gradient": round(old_g / new_g, 3)})

    # one whole coupled gradient: the objective's own code on a state of random displacements and a solved temperature
    heat = thermal.HeatConductionSimulator(box, list(grid))
    fixed = np.zeros(tuple(g + 1 for g in grid), dtype=bool)
    fixed[0] = True
    heat.fixedTemperatureMask = fixed.reshape(-1)
    heat.setHeatSources(volumetric=1.0)
    heat.setElementDensities(rho)
    th = thermal.ThermalComplianceObjective(heat, solver="pcg", preconditioner="multigrid", skipSolve=True)
    th.updateCache(None)
    first = th.iterations
    hot = [loadcases.LoadCase(loads=0, temperature=thermoelastic.TemperatureLoad(th, 0.01 * (1.0 + 0.1 * i), tref[i])) for i in range(cases)]
    obj = loadcases.LoadCaseComplianceObjective(sim, hot, skipSolve=True)
    grid_ = loadcases._Grid(sim)
    obj._state = dict(grid=grid_, U=U, us=[U[i] for i in range(cases)], dE=dE, dm=None, E=E, T=th._u, a=a, grad=None)
    _line("coupled_gradient_whole", grid, _time(lambda: obj._weighted_gradient(a), max(3, reps // 4), 1), None, cases=cases,
          heat_pcg_iterations_primal=first, heat_pcg_iterations_adjoint=th.iterations, heat_levels=len(heat.multigridLevels()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs="+", default=[256, 256, 128])
    ap.add_argument("--cases", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thermoelastic_time.json"))
    a = ap.parse_args()
    signal.signal(signal.SIGALRM, _expire)
    signal.alarm(a.timeout)
    try:
        _run(tuple(a.grid), a.cases, a.reps, a.warmup)
    finally:
        with open(a.out, "w") as fh:
            json.dump(LINES, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
