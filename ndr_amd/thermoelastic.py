"""Thermo-elastic coupling on the device: the temperature field of a heat-conduction solve as the thermal load of a load case, with
the coupled density gradient.

    heat = thermal.HeatConductionSimulator(bbox, ne)                     # the same grid and box as the elastic simulator
    heat.fixTemperatureInBox(...); heat.setHeatSources(volumetric=1.0)
    solve = thermal.ThermalComplianceObjective(heat, solver="direct", skipSolve=True)
    hot = loadcases.LoadCase(loads=F, temperature=TemperatureLoad(solve, expansion=1.2e-5, referenceTemperature=0.0))
    obj = loadcases.LoadCaseComplianceObjective(sim, [hot])              # J, dJ/drho with one thermal adjoint solve
    cap = mma.ObjectiveConstraint(thermal.PNormTemperatureObjective(solve), bound)     # shares the heat solve

for a degree-1 simulator in 2-D or 3-D, whole grids.  The numerics run in ``libvfem.so`` (``vfem_thermoelastic_*``, include/vfem.h);
DESIGN 3.17 has the formulas.  With theta = T - T_ref at the nodes (T the heat simulator's solution, its fixed nodes at 0),
beta = C : alpha and the consistent coupling matrix of a full-density voxel

    G[(n, a)][m] = int beta_aq dN_n/dx_q N_m dV = sum_q beta[a][q] s_nq (vol / h_q) 1/2 prod_{d != q} w(n_d, m_d),

w = 1/3 where the two nodes are on the same side of axis d and 1/6 otherwise (the temperature is interpolated inside the element,
not averaged over it; the row sums of G are the eigenstrain pattern Lt of eps* = alpha), a heated case has the load

    f_i = P (F_i + [self-weight, constant eigenstrain] + sum_e E_e G_i theta_e),      c_i = 1/2 f_i . u_i

and with the aggregate coefficients a_i = dJ/dc_i and design-independent heat sources

    q = P_T sum_i a_i sum_e E_e G_i^T u_ie,      A(rho) mu = q      (one thermal adjoint solve for all cases)
    dJ/drho_e = [the load-case gradient] + dE_e sum_i a_i u_ie^T G_i theta_e - kappa'_e mu_e^T Kc0 T_e.

There is no elastic adjoint solve.
"""
import numpy as np
import torch

from . import _lib, loadcases
from ._grid import _dp
from .pyVoxelFEM import _dev, _ptr, _stream, _to_dev
from .thermal import ThermalComplianceObjective

__all__ = ["couplingMatrix", "TemperatureLoad", "thermalLoad_device", "adjointSource_device", "couplingGradient_device", "MAX_CASES"]

MAX_CASES = 8


def _expansion_tensor(expansion, N, who):
    """alpha as a symmetric N x N matrix: a scalar means alpha I"""
    al = np.asarray(expansion, dtype=np.float64)
    if al.ndim == 0:
        al = np.diag(np.full(N, float(al)))
    if al.shape != (N, N) or not np.isfinite(al).all() or np.abs(al - al.T).max() > 1e-12 * max(np.abs(al).max(), 1e-300):
        raise RuntimeError("%s: expansion must be a finite scalar or a finite symmetric %d x %d matrix" % (who, N, N))
    return 0.5 * (al + al.T)


def couplingMatrix(sim, expansion):
    """G [ke = N 2^N, 2^N] of a full-density voxel of ``sim`` for the expansion ``expansion`` (a scalar alpha, meaning alpha I, or a
    symmetric N x N tensor): G[(n, a)][m] = int (C : alpha)_aq dN_n/dx_q N_m dV in the local node order of K0"""
    g = loadcases._Grid(sim)
    N, npe = g.N, 2 ** g.N
    al = _expansion_tensor(expansion, N, "couplingMatrix")
    beta = np.asarray(sim.ETensor.doubleContract(al), dtype=np.float64).reshape(N, N)
    bits = np.array([[(n >> (N - 1 - d)) & 1 for d in range(N)] for n in range(npe)])
    G = np.zeros((g.ke, npe))
    for n in range(npe):
        for m in range(npe):
            w = np.where(bits[n] == bits[m], 1.0 / 3.0, 1.0 / 6.0)
            for q in range(N):
                s = 1.0 if bits[n, q] else -1.0
                G[n * N:(n + 1) * N, m] += beta[:, q] * (s * g.vol / g.h[q] * 0.5 * np.prod(np.delete(w, q)))
    if not np.isfinite(G).all():
        raise RuntimeError("couplingMatrix: the coupling matrix is not finite")
    return np.ascontiguousarray(G)


class TemperatureLoad:
    """The temperature of a heat-conduction solve as the thermal load of a ``loadcases.LoadCase(temperature=...)``.

    ``thermal``: the ``ThermalComplianceObjective`` that solves the heat problem; it brings its simulator, its solver choice and the
    solve the coupled adjoint goes through (as ``PNormTemperatureObjective`` takes it).  Its simulator must have the grid and the
    bounding box of the elastic simulator (checked when the case is handed to an objective).  ``expansion``: a scalar alpha or a
    symmetric N x N tensor.  ``referenceTemperature``: T_ref, the temperature at which the body is stress-free; the load is that
    of theta = T - T_ref."""

    def __init__(self, thermal, expansion, referenceTemperature=0.0):
        if not isinstance(thermal, ThermalComplianceObjective):
            raise TypeError("TemperatureLoad takes a ThermalComplianceObjective (got %r)" % (type(thermal).__name__,))
        self.thermal = thermal
        self.expansion = _expansion_tensor(expansion, int(thermal._sim.N), "TemperatureLoad")
        self.referenceTemperature = float(referenceTemperature)
        if not np.isfinite(self.referenceTemperature):
            raise RuntimeError("TemperatureLoad: referenceTemperature must be finite (got %r)" % (referenceTemperature,))

    def check(self, sim):
        """refuse a heat simulator that does not stand on the elastic simulator's grid"""
        heat = self.thermal._sim
        ne = [int(n) for n in sim.NbElementsPerDimension()]
        if heat.N != sim.N or [int(n) for n in heat.NbElementsPerDimension()] != ne:
            raise RuntimeError("TemperatureLoad: the heat simulator's grid %s is not the elastic simulator's %s"
                               % ([int(n) for n in heat.NbElementsPerDimension()], ne))
        lo, hi = np.asarray(sim._bbmin, dtype=np.float64), np.asarray(sim._bbmax, dtype=np.float64)
        tol = 1e-12 * float(np.abs(hi - lo).max())
        if np.abs(heat._bbmin - lo).max() > tol or np.abs(heat._bbmax - hi).max() > tol:
            raise RuntimeError("TemperatureLoad: the heat simulator's bounding box is not the elastic simulator's")

    def couplingMatrix(self, sim):
        return couplingMatrix(sim, self.expansion)


# ---- the three calls, for tests and tools ----

def _matrices(g, G, count=None):
    G = np.ascontiguousarray(np.asarray(G, dtype=np.float64))
    per = g.ke * 2 ** g.N
    k = 1 if count is None else int(count)
    if G.size != k * per:
        raise RuntimeError("Invalid input size: expected %d coupling matrices of %d x %d values, got %d values" % (k, g.ke, 2 ** g.N, G.size))
    return G


def _host(values, k, what):
    v = np.ascontiguousarray(np.asarray(values, dtype=np.float64).reshape(-1))
    if v.size != k:
        raise RuntimeError("Invalid input size: expected %d %s, got %d" % (k, what, v.size))
    return v


def _columns(g, U):
    U = _to_dev(U)
    if U.numel() % g.n:
        raise RuntimeError("Invalid input size: expected columns of %d x %d values, got %d values" % (g.nnode, g.N, U.numel()))
    return U.reshape(-1, g.nnode, g.N)


def thermalLoad_device(sim, G, T, referenceTemperature=0.0, E=None, f_in=None, masked=True, out=None):
    """P (f_in + sum_e E_e G (T_e - T_ref)) [numNodes, N]: ``E`` defaults to the simulator's moduli at its present densities,
    ``masked=False`` leaves the Dirichlet components in, ``out`` (default: a new tensor) may be ``f_in``"""
    g = loadcases._Grid(sim)
    G = _matrices(g, G)
    T = _to_dev(T, (g.nnode,))
    E = g.stiffness_multipliers(sim.getDensities_device()[:g.nelem])[0] if E is None else _to_dev(E, (g.nelem,))
    f_in = None if f_in is None else _to_dev(f_in, (g.nnode, g.N))
    if out is None:
        out = torch.empty((g.nnode, g.N), dtype=torch.float64, device=_dev())
    _lib.check(_lib.load().vfem_thermoelastic_load(*g.head(), _dp(G), float(referenceTemperature), _ptr(E), _ptr(T),
                                                   _ptr(g.mask) if masked else None, None if f_in is None else _ptr(f_in), _ptr(out),
                                                   _stream()))
    return out


def adjointSource_device(sim, coefficients, G, U, E=None, fixed=None, out=None):
    """q [numNodes] = P_T sum_i a_i sum_e E_e G_i^T u_ie over the columns of ``U`` [cases, numNodes, N]; ``G`` [cases, ke, 2^N];
    ``fixed``: one byte per node on the device (nonzero: q is 0 there), or None"""
    g = loadcases._Grid(sim)
    U = _columns(g, U)
    k = U.shape[0]
    a, G = _host(coefficients, k, "coefficients"), _matrices(g, G, k)
    E = g.stiffness_multipliers(sim.getDensities_device()[:g.nelem])[0] if E is None else _to_dev(E, (g.nelem,))
    if out is None:
        out = torch.empty(g.nnode, dtype=torch.float64, device=_dev())
    _lib.check(_lib.load().vfem_thermoelastic_adjoint_source(*g.head(), k, _dp(a), _dp(G), _ptr(E), _ptr(U),
                                                             None if fixed is None else _ptr(fixed), _ptr(out), _stream()))
    return out


def couplingGradient_device(sim, coefficients, G, referenceTemperatures, dE, T, U, g_in=None, out=None):
    """g_in + dE_e sum_i a_i u_ie^T G_i (T_e - T_ref,i) [numElements]; ``out`` (default: a new tensor) may be ``g_in``"""
    g = loadcases._Grid(sim)
    U = _columns(g, U)
    k = U.shape[0]
    a, tref, G = _host(coefficients, k, "coefficients"), _host(referenceTemperatures, k, "reference temperatures"), _matrices(g, G, k)
    dE, T = _to_dev(dE, (g.nelem,)), _to_dev(T, (g.nnode,))
    g_in = None if g_in is None else _to_dev(g_in, (g.nelem,))
    if out is None:
        out = torch.empty(g.nelem, dtype=torch.float64, device=_dev())
    _lib.check(_lib.load().vfem_thermoelastic_gradient(*g.head(), k, _dp(a), _dp(G), _dp(tref), _ptr(dE), _ptr(T), _ptr(U),
                                                       None if g_in is None else _ptr(g_in), _ptr(out), _stream()))
    return out
