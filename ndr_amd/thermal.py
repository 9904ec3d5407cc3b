"""Steady heat conduction on the device: the scalar operator of a degree-1 voxel grid, its two solvers, the thermal compliance and
the peak-temperature measure with their density gradients, and the flux field.

    heat = HeatConductionSimulator([[0, 0], [1, 1]], [64, 64])
    heat.fixTemperatureInBox([0, 0.45], [0, 0.55])                       # the sink, at the reference temperature
    heat.setHeatSources(volumetric=1.0)                                  # a uniformly heated plate
    obj = ThermalComplianceObjective(heat, solver="direct")
    problem = pyVoxelFEM.TopologyOptimizationProblem(heat, obj, [pyVoxelFEM.TotalVolumeConstraint(0.4)], [smooth])
    problem.setVars(x0); oc = pyVoxelFEM.OCOptimizer(problem); oc.step()
    cap = mma.ObjectiveConstraint(PNormTemperatureObjective(ThermalComplianceObjective(heat, skipSolve=True), P=8.0), bound)
    loss = thermalCompliance(densities, obj)                             # the same as an autograd node

for whole grids in 2-D and 3-D.  The numerics run in ``libvfem.so`` (``vfem_thermal_*``, include/vfem.h); DESIGN 3.16 has the
formulas.  T is one temperature per node, in the node order of the simulators.  With the element conductivity
kappa_e = k_min + rho_e^p (1 - k_min) and the conductivity matrix Kc0 of a full-density voxel,

    A(kappa) = P (sum_e kappa_e Kc0) P + (I - P),      Q = P (Q_nodal + sum_e q_e vol / 2^N),      A T = Q,

P zeroing the nodes of the fixed-temperature mask (fixed temperatures are zero: the sink defines the reference temperature).

    thermal compliance   J = Q . T                                dJ/drho_e   = -kappa'_e T_e^T Kc0 T_e
    peak temperature     J_P = (sum_n |T_n|^P)^(1/P) >= max |T|,  dJ_P/drho_e = -kappa'_e lambda_e^T Kc0 T_e,  A lambda = P dJ_P/dT

The compliance gradient is nowhere positive for the design-independent sources taken here, so ``OCOptimizer`` works; the
peak-temperature measure is a constraint for ``ndr_amd.mma.MMAOptimizer`` (``mma.ObjectiveConstraint``).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._grid import ObjectiveFunction, _dp
from .pyVoxelFEM import _dev, _ptr, _stream, _to_dev, _to_np

__all__ = ["HeatConductionSimulator", "ThermalComplianceObjective", "PNormTemperatureObjective", "ThermalComplianceFunction",
           "PNormTemperatureFunction", "thermalCompliance", "pNormTemperature", "conductivityMatrix", "MAX_COLUMNS"]

MAX_COLUMNS = 8
_TILE = 64


def conductivityMatrix(k, h):
    """Kc0[a][b] = int grad N_a^T k grad N_b dV of a voxel with the edge lengths ``h`` and the N x N conductivity tensor ``k``, by two
    Gauss points per axis (exact); local node a has axis 0 as its most significant bit"""
    h = np.asarray(h, dtype=np.float64)
    N, npe = h.size, 2 ** h.size
    k = np.asarray(k, dtype=np.float64).reshape(N, N)
    bits = np.array([[(a >> (N - 1 - d)) & 1 for d in range(N)] for a in range(npe)])
    gp = 0.5 + np.array([-0.5, 0.5]) / np.sqrt(3.0)
    K = np.zeros((npe, npe))
    for idx in np.ndindex(*([2] * N)):
        xi = gp[list(idx)]
        shape = np.where(bits == 1, xi, 1.0 - xi)                           # [node][axis]: the 1-D factor of N_a along each axis
        grad = np.empty((npe, N))
        for d in range(N):
            others = np.prod(np.delete(shape, d, axis=1), axis=1)
            grad[:, d] = np.where(bits[:, d] == 1, 1.0, -1.0) / h[d] * others
        K += grad @ k @ grad.T * (np.prod(h) / npe)
    return K


def _check_solver(who, solver, preconditioner):
    """the three refusals of every call that takes ``solver`` and ``preconditioner``"""
    if solver not in ("direct", "pcg"):
        raise RuntimeError("%s: solver is \"direct\" or \"pcg\" (got %r)" % (who, solver))
    if preconditioner not in ("jacobi", "multigrid"):
        raise RuntimeError("%s: preconditioner is \"jacobi\" or \"multigrid\" (got %r)" % (who, preconditioner))
    if preconditioner != "jacobi" and solver != "pcg":
        raise RuntimeError("%s: a preconditioner goes with solver=\"pcg\" (got solver %r)" % (who, solver))


def _set_densities(sim, xPhys):
    """the densities of a design update (None: as they are): set only if they differ, since setting them again would drop the kept
    factor; returns whether they were set"""
    if xPhys is None:
        return False
    x = _to_dev(xPhys).reshape(-1)
    if x.shape == sim._rho.shape and torch.equal(sim._rho, x):
        return False
    sim.setElementDensities(x)
    return True


class _KeptSolvers:
    """The band factor and the multigrid hierarchy of one operator, for ``HeatConductionSimulator`` and
    ``ndr_amd.transient.TransientHeatSimulator``: each is built on first use, counted, and kept until ``drop()``; the hierarchy's
    handle is destroyed there, or with the holder."""

    def __init__(self):
        self.band = self.mg = None          # mg: (handle, the arrays it reads: kept alive)
        self.factorizations = self.builds = 0

    def factor(self, assemble, n, w):
        if self.band is None:
            band = assemble()
            _lib.check(_lib.load().vfem_band_spd_factor(n, w, _ptr(band), _stream()))
            self.band = band
            self.factorizations += 1
        return self.band

    def multigrid(self, create, operator):
        """the handle of ``create(&handle, *args, all coarsenings, stream)``, with ``operator()`` = (args, the arrays that the handle
        goes on reading: kept alive with it)"""
        if self.mg is None:
            args, alive = operator()
            handle = ctypes.c_void_p()
            _lib.check(create(ctypes.byref(handle), *args, -1, _stream()))
            self.mg = (handle, alive)
            self.builds += 1
        return self.mg[0]

    def drop_multigrid(self):
        if getattr(self, "mg", None) is not None:
            handle, self.mg = self.mg[0], None
            _lib.load().vfem_thermal_mg_destroy(handle)

    def drop(self):
        self.band = None
        self.drop_multigrid()

    def __del__(self):
        try:
            self.drop_multigrid()
        except Exception:
            pass


class HeatConductionSimulator:
    """Steady heat conduction -div(kappa k grad T) = q on a grid of ``elementsPerDimension`` voxels (2 or 3 axes) over
    ``domainBBox`` = [lower corner, upper corner].  It has what the design problem and the filters read from a simulator
    (``numElements``, ``numNodes``, ``NbElementsPerDimension``, the density accessors) and is otherwise a class of its own.

    ``conductivity``: a positive scalar or a symmetric positive definite N x N tensor (default 1).  ``k_min`` (default 1e-3) and
    ``exponent`` (default 3): kappa_e = k_min + rho_e^exponent (1 - k_min) multiplies the full-density element matrix.
    ``fixedTemperatureMask``: bool [numNodes], the nodes held at the reference temperature 0 (assign a whole array, or use
    ``fixTemperatureInBox``).  ``setHeatSources(nodal, volumetric)``: a nodal source [numNodes] and a volumetric source per
    element ([numElements] or a scalar).

    ``solve_device(Q)`` factorises the band of A on the device (``vfem_thermal_band_assemble`` + ``vfem_band_spd_factor``) and keeps
    the factor until the densities, the material or the mask change; ``pcg_device`` is the conjugate-gradient solver, with the
    Jacobi preconditioner or (``preconditioner="multigrid"``) a geometric multigrid V-cycle whose hierarchy (``vfem_thermal_mg_*``)
    is kept as long as the factor is: ``numMultigridBuilds()``, ``multigridLevels()``, ``multigridBytes()``."""

    def __init__(self, domainBBox, elementsPerDimension):
        _lib.require_gpu()
        ne = np.array([int(n) for n in elementsPerDimension], dtype=np.int64)
        if ne.size not in (2, 3) or np.any(ne < 1):
            raise RuntimeError("HeatConductionSimulator: 2 or 3 axes of at least 1 element each (got %r)" % (list(elementsPerDimension),))
        lo, hi = (np.asarray(c, dtype=np.float64).reshape(-1) for c in domainBBox)
        if lo.size != ne.size or hi.size != ne.size or not np.all(hi > lo) or not (np.isfinite(lo).all() and np.isfinite(hi).all()):
            raise RuntimeError("HeatConductionSimulator: the bounding box must have %d finite coordinates per corner, upper > lower" % ne.size)
        self.N = int(ne.size)
        self._version = 0                   # counts the changes of the operator (what ndr_amd.transient keeps its own factor by)
        self._ne, self._nn = ne, ne + 1
        self._bbmin, self._bbmax = lo, hi
        self._h = (hi - lo) / ne
        self._rho = torch.ones(self.numElements(), dtype=torch.float64, device=_dev())
        self._k = np.eye(self.N)
        self._k_min, self._exponent = 1e-3, 3.0
        self._mask = np.zeros(self.numNodes(), dtype=bool)
        self._mask_dev = torch.zeros(self.numNodes(), dtype=torch.uint8, device=_dev())
        self._Qn = self._qv = None
        self._Kc0 = None
        self._kept = _KeptSolvers()         # the band factor and the multigrid hierarchy of the present operator
        self.last_iterations = 0
        self.last_relative_residual = 0.0

    # ---- sizes / geometry ----
    def numNodes(self):
        return int(np.prod(self._nn))

    def numElements(self):
        return int(np.prod(self._ne))

    def NbElementsPerDimension(self):
        return self._ne.copy()

    def nodePositions(self):
        """[numNodes, N] on the host"""
        axes = [self._bbmin[d] + np.arange(self._nn[d]) * self._h[d] for d in range(self.N)]
        return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, self.N)

    def _head(self):
        return self.N, self._ne.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))

    def _changed(self):
        """the operator changed: the kept factor and the kept hierarchy no longer stand for it"""
        self._version += 1
        self._kept.drop()

    def _drop_multigrid(self):
        self._kept.drop_multigrid()

    # ---- material ----
    def _get_conductivity(self):
        return self._k.copy()

    def _set_conductivity(self, k):
        k = np.asarray(k, dtype=np.float64)
        if k.ndim == 0:
            k = float(k) * np.eye(self.N)
        if k.shape != (self.N, self.N) or not np.isfinite(k).all() or np.abs(k - k.T).max() > 1e-12 * np.abs(k).max():
            raise RuntimeError("HeatConductionSimulator: conductivity is a positive scalar or a symmetric %d x %d tensor" % (self.N, self.N))
        if not np.linalg.eigvalsh(k).min() > 0.0:
            raise RuntimeError("HeatConductionSimulator: the conductivity tensor is not positive definite")
        self._k, self._Kc0 = 0.5 * (k + k.T), None
        self._changed()

    conductivity = property(_get_conductivity, _set_conductivity)

    def _set_k_min(self, v):
        v = float(v)
        if not np.isfinite(v) or v < 0.0 or v >= 1.0:
            raise RuntimeError("HeatConductionSimulator: k_min must be in [0, 1) (got %r)" % (v,))
        self._k_min = v
        self._changed()

    def _set_exponent(self, v):
        v = float(v)
        if not np.isfinite(v) or v < 1.0:
            raise RuntimeError("HeatConductionSimulator: exponent must be finite and at least 1 (got %r)" % (v,))
        self._exponent = v
        self._changed()

    k_min = property(lambda s: s._k_min, _set_k_min)
    exponent = property(lambda s: s._exponent, _set_exponent)

    def fullDensityElementConductivityMatrix(self):
        if self._Kc0 is None:
            self._Kc0 = np.ascontiguousarray(conductivityMatrix(self._k, self._h))
        return self._Kc0.copy()

    def _K(self):
        self.fullDensityElementConductivityMatrix()
        return self._Kc0

    def elementConductivities_device(self):
        """(kappa, dkappa/drho) [numElements] at the present densities"""
        p, span = self._exponent, 1.0 - self._k_min
        return (self._k_min + self._rho ** p * span).contiguous(), (p * self._rho ** (p - 1.0) * span).contiguous()

    # ---- densities ----
    def setUniformDensities(self, density):
        if density > 1.0 or density < 0:
            raise RuntimeError("Density value (%f) has to be in between 0 and 1" % density)
        self._rho = torch.full((self.numElements(),), float(density), dtype=torch.float64, device=_dev())
        self._changed()

    def setElementDensities(self, rho):
        self._rho = _to_dev(rho, (self.numElements(),)).clone()
        self._changed()

    def getDensities_device(self):
        return self._rho.clone()

    def getDensities(self):
        return _to_np(self._rho)

    # ---- boundary conditions and sources ----
    def _get_mask(self):
        return self._mask.copy()

    def _set_mask(self, mask):
        mask = np.asarray(mask)
        if mask.dtype != bool or mask.size != self.numNodes():
            raise RuntimeError("fixedTemperatureMask is a bool array of numNodes = %d values" % self.numNodes())
        self._mask = mask.reshape(-1).copy()
        self._mask_dev = torch.from_numpy(self._mask.astype(np.uint8)).to(_dev())
        self._changed()

    fixedTemperatureMask = property(_get_mask, _set_mask)

    def fixTemperatureInBox(self, lower, upper, value=0.0):
        """fix the nodes inside the box [lower, upper] (its faces included, to 1e-9 of an edge length) at the reference
        temperature; returns how many nodes the box holds"""
        if float(value) != 0.0:
            raise RuntimeError("Nonzero fixed temperatures currently unsupported (the sink is at the reference temperature 0)")
        lo, hi = (np.asarray(c, dtype=np.float64).reshape(-1) for c in (lower, upper))
        if lo.size != self.N or hi.size != self.N:
            raise RuntimeError("fixTemperatureInBox: the corners have %d coordinates" % self.N)
        eps = 1e-9 * self._h
        inside = np.all((self.nodePositions() >= lo - eps) & (self.nodePositions() <= hi + eps), axis=1)
        self.fixedTemperatureMask = self._mask | inside
        return int(inside.sum())

    def setHeatSources(self, nodal=None, volumetric=None):
        """``nodal``: [numNodes] (numpy or device); ``volumetric``: [numElements] or a scalar, per unit volume.  ``None``: none."""
        if nodal is not None:
            nodal = _to_dev(nodal, (self.numNodes(),)).clone()
            if not bool(torch.isfinite(nodal).all()):
                raise RuntimeError("setHeatSources: the nodal source is not finite")
        if volumetric is not None:
            if not isinstance(volumetric, torch.Tensor) and np.ndim(volumetric) == 0:
                volumetric = torch.full((self.numElements(),), float(volumetric), dtype=torch.float64, device=_dev())
            else:
                volumetric = _to_dev(volumetric, (self.numElements(),)).clone()
            if not bool(torch.isfinite(volumetric).all()):
                raise RuntimeError("setHeatSources: the volumetric source is not finite")
        self._Qn, self._qv = nodal, volumetric

    def _fixed(self):
        return _ptr(self._mask_dev) if self._mask.any() else None

    def _need_sink(self, what):
        if not self._mask.any():
            raise RuntimeError("%s: no node has a fixed temperature, the conduction operator is singular (fix a sink first)" % what)

    def buildLoadVector_device(self):
        """Q = P (Q_nodal + sum_e q_e vol / 2^N) [numNodes]"""
        out = torch.zeros(self.numNodes(), dtype=torch.float64, device=_dev())
        if self._Qn is None and self._qv is None:
            return out
        h = np.ascontiguousarray(self._h)
        _lib.check(_lib.load().vfem_thermal_source(*self._head(), _dp(h), None if self._qv is None else _ptr(self._qv), self._fixed(),
                                                   None if self._Qn is None else _ptr(self._Qn), _ptr(out), _stream()))
        return out

    def buildLoadVector(self):
        return _to_np(self.buildLoadVector_device())

    # ---- operator ----
    def applyK_device(self, T):
        """A T for one field [numNodes] or a block [columns <= 8, numNodes]"""
        T = _to_dev(T)
        cols = 1 if T.dim() == 1 else T.shape[0]
        if T.numel() != cols * self.numNodes():
            raise RuntimeError("Invalid input size")
        kappa = self.elementConductivities_device()[0]
        out = torch.empty_like(T)
        _lib.check(_lib.load().vfem_thermal_apply(*self._head(), _dp(self._K()), _ptr(kappa), self._fixed(), cols, _ptr(T), _ptr(out),
                                                  _stream()))
        return out

    def applyK(self, T):
        return _to_np(self.applyK_device(T))

    def diagonal_device(self):
        kappa = self.elementConductivities_device()[0]
        out = torch.empty(self.numNodes(), dtype=torch.float64, device=_dev())
        _lib.check(_lib.load().vfem_thermal_diagonal(*self._head(), _dp(self._K()), _ptr(kappa), self._fixed(), _ptr(out), _stream()))
        return out

    # ---- direct solver ----
    def _band_geometry(self):
        n, w = 1, 0
        for a in range(self.N - 1, -1, -1):
            w += n
            n *= int(self._nn[a])
        return n, w

    def directBandBytes(self):
        n, w = self._band_geometry()
        return (n + _TILE - 1) // _TILE * ((w + _TILE - 1) // _TILE + 2) * _TILE * _TILE * 8

    def numDirectFactorizations(self):
        return self._kept.factorizations

    def assembleBand_device(self):
        """the lower band of A in the tile layout of ``vfem_band_spd_factor`` (a new buffer; the factor slots are zero)"""
        kappa = self.elementConductivities_device()[0]
        band = torch.zeros(self.directBandBytes() // 8, dtype=torch.float64, device=_dev())
        _lib.check(_lib.load().vfem_thermal_band_assemble(*self._head(), _dp(self._K()), _ptr(kappa), self._fixed(), _ptr(band), _stream()))
        return band

    def solve_device(self, Q):
        """T = A^-1 Q on the free nodes, 0 on the fixed ones (Q is ignored there); one field [numNodes] or a block"""
        self._need_sink("solve_device")
        Q = _to_dev(Q)
        cols = 1 if Q.dim() == 1 else Q.shape[0]
        if Q.numel() != cols * self.numNodes():
            raise RuntimeError("Invalid input size")
        n, w = self._band_geometry()
        band = self._kept.factor(self.assembleBand_device, n, w)
        T = Q.clone()
        T.reshape(cols, n)[:, self._mask_dev.bool()] = 0.0
        _lib.check(_lib.load().vfem_band_spd_solve(n, w, _ptr(band), _ptr(T), cols, _stream()))
        return T

    def solve(self, Q):
        return _to_np(self.solve_device(Q))

    # ---- iterative solver ----
    def _multigrid(self):
        """the hierarchy of the present operator (``vfem_thermal_mg_create``), built on first use and kept until the densities, the
        material or the mask change: the events that drop the band factor"""
        def operator():
            kappa, mask, Kc0 = self.elementConductivities_device()[0], self._mask_dev, self._K()
            return (*self._head(), _dp(Kc0), _ptr(kappa), self._fixed()), (kappa, mask, Kc0)
        return self._kept.multigrid(_lib.load().vfem_thermal_mg_create, operator)

    def numMultigridBuilds(self):
        return self._kept.builds

    def multigridLevels(self):
        """the elements per axis of every level of the hierarchy (built if need be)"""
        lib, h = _lib.load(), self._multigrid()
        out = []
        for l in range(lib.vfem_thermal_mg_num_levels(h)):
            n = np.zeros(self.N, dtype=np.int64)
            _lib.check(lib.vfem_thermal_mg_level_dims(h, l, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            out.append([int(v) for v in n])
        return out

    def multigridBytes(self):
        """device memory the hierarchy holds (built if need be)"""
        return int(_lib.load().vfem_thermal_mg_bytes(self._multigrid()))

    def pcg_device(self, Q, x0=None, tol=1e-8, maxIter=2000, preconditioner="jacobi", smoothing=1):
        """conjugate gradients on A T = Q from ``x0`` (default 0) until |r| / |Q| <= tol, with the Jacobi preconditioner or
        (``preconditioner="multigrid"``) one V-cycle of ``smoothing`` sweeps before and after the coarse correction;
        ``last_iterations`` and ``last_relative_residual`` are those of this solve.  Raises when ``maxIter`` is reached or the
        operator is singular."""
        _check_solver("pcg_device", "pcg", preconditioner)
        self._need_sink("pcg_device")
        Q = _to_dev(Q, (self.numNodes(),))
        x = torch.zeros_like(Q) if x0 is None else _to_dev(x0, (self.numNodes(),)).clone()
        it, rel = ctypes.c_int(0), ctypes.c_double(0.0)
        if preconditioner == "multigrid":
            status = _lib.load().vfem_thermal_mg_pcg(self._multigrid(), _ptr(Q), _ptr(x), float(tol), int(maxIter), int(smoothing),
                                                     ctypes.byref(it), ctypes.byref(rel), _stream())
        else:
            kappa = self.elementConductivities_device()[0]
            status = _lib.load().vfem_thermal_pcg(*self._head(), _dp(self._K()), _ptr(kappa), self._fixed(), _ptr(Q), _ptr(x), float(tol),
                                                  int(maxIter), ctypes.byref(it), ctypes.byref(rel), _stream())
        self.last_iterations, self.last_relative_residual = int(it.value), float(rel.value)
        _lib.check(status)
        return x

    def pcg(self, Q, x0=None, tol=1e-8, maxIter=2000, preconditioner="jacobi", smoothing=1):
        return _to_np(self.pcg_device(Q, x0, tol, maxIter, preconditioner, smoothing))

    # ---- fields ----
    def flux_device(self, T):
        """q_e = -kappa_e k grad T at the element centres, [numElements, N]"""
        T = _to_dev(T, (self.numNodes(),))
        kappa = self.elementConductivities_device()[0]
        out = torch.empty((self.numElements(), self.N), dtype=torch.float64, device=_dev())
        h, k = np.ascontiguousarray(self._h), np.ascontiguousarray(self._k)
        _lib.check(_lib.load().vfem_thermal_flux(*self._head(), _dp(h), _dp(k), _ptr(kappa), _ptr(T), _ptr(out), _stream()))
        return out

    def flux(self, T):
        return _to_np(self.flux_device(T))

    def bilinearGradient_device(self, coefficients, A, B=None):
        """g[e] = kappa'_e sum_i c_i a_ie^T Kc0 b_ie over 1 to 8 column pairs of the blocks ``A`` and ``B`` (default: ``A``)"""
        c = np.ascontiguousarray(np.asarray(coefficients, dtype=np.float64).reshape(-1))
        A = _to_dev(A, (c.size, self.numNodes()))
        B = A if B is None else _to_dev(B, (c.size, self.numNodes()))
        dkappa = self.elementConductivities_device()[1]
        out = torch.empty(self.numElements(), dtype=torch.float64, device=_dev())
        _lib.check(_lib.load().vfem_thermal_gradient(*self._head(), int(c.size), _dp(self._K()), _dp(c), _ptr(dkappa), _ptr(A), _ptr(B),
                                                     _ptr(out), _stream()))
        return out


class ThermalComplianceObjective:
    """J(rho) = Q . T with A(rho) T = Q: the thermal compliance of a ``HeatConductionSimulator``, and dJ/drho_e = -kappa'_e T_e^T Kc0
    T_e (self-adjoint: no adjoint solve; nowhere positive, so ``OCOptimizer`` applies).

    ``solver``: "direct" (``heat.solve_device``: one factorisation per design), "pcg" (``heat.pcg_device`` with the attributes
    ``tol`` = 1e-8 and ``maxIter`` = 2000, warm-started from the last temperature; ``iterations`` is the count of the last
    solve).  ``preconditioner`` (with "pcg"): "jacobi", or "multigrid" with the attribute ``smoothing`` = 1: one hierarchy per design,
    which the adjoint solves of the measures built on this objective reuse.  (``solver`` itself keeps its two values: "multigrid"
    as a solver name stays refused, as it was.)  The sources are read from the simulator at every update.  The constructor solves
    once unless ``skipSolve``.

    The objective protocol of the design loop: ``updateCache(xPhys)``, ``evaluate()``, ``gradient_device()``, ``gradient()``.
    ``_sim`` is the simulator and ``_u`` the temperature, a new tensor with every solve (what ``mma.ObjectiveConstraint``
    follows)."""

    def __init__(self, heat, solver="direct", skipSolve=False, preconditioner="jacobi"):
        if not isinstance(heat, HeatConductionSimulator):
            raise TypeError("ThermalComplianceObjective takes a HeatConductionSimulator (got %r)" % (type(heat).__name__,))
        _check_solver("ThermalComplianceObjective", solver, preconditioner)
        self._sim, self.solver, self.preconditioner = heat, solver, preconditioner
        self.tol, self.maxIter, self.smoothing = 1e-8, 2000, 1
        self.iterations = 0
        self._u = self._f = None
        self._J = self._grad = None
        if not skipSolve:
            self.updateCache(None)

    def _solve(self, Q, last=None):
        """A^-1 Q through the objective's solver (the adjoint solves of the measures built on it come here too)"""
        if self.solver == "direct":
            return self._sim.solve_device(Q)
        x = self._sim.pcg_device(Q, last, self.tol, self.maxIter, self.preconditioner, self.smoothing)
        self.iterations = self._sim.last_iterations
        return x

    def updateCache(self, xPhys):
        sim = self._sim
        _set_densities(sim, xPhys)
        Q = sim.buildLoadVector_device()
        T = self._solve(Q, self._u)
        J = float(torch.dot(Q, T))
        if not np.isfinite(J):
            raise RuntimeError("ThermalComplianceObjective: the compliance is not finite (%r)" % (J,))
        self._f, self._u, self._J, self._grad = Q, T, J, None

    def _need(self):
        if self._u is None:
            raise RuntimeError("ThermalComplianceObjective: updateCache(xPhys) has not been called")

    def evaluate(self, xPhys=None):
        if xPhys is not None:
            self.updateCache(xPhys)
        self._need()
        return self._J

    compliance = evaluate

    def gradient_device(self):
        self._need()
        if self._grad is None:
            self._grad = self._sim.bilinearGradient_device([-1.0], self._u.unsqueeze(0))
        return self._grad.clone()

    def gradient(self):
        return _to_np(self.gradient_device())

    def temperature_device(self):
        self._need()
        return self._u

    def temperature(self):
        return _to_np(self.temperature_device())


class PNormTemperatureObjective:
    """J_P(rho) = (sum_n |T_n|^P)^(1/P), a smooth upper bound of the peak temperature (max |T| <= J_P <= numNodes^(1/P) max |T|), of
    the problem a ``ThermalComplianceObjective`` solves.  ``solved`` points at that objective: its temperature is shared, and
    this measure adds one adjoint solve A lambda = P dJ_P/dT through the same factor or PCG, so an update at densities the shared
    objective already stands at factorises nothing.  The measure is evaluated scaled by max |T| (``vfem_stress_pnorm``) and cannot
    overflow."""

    def __init__(self, thermalCompliance, P=8.0):
        if not isinstance(thermalCompliance, ThermalComplianceObjective):
            raise TypeError("PNormTemperatureObjective takes a ThermalComplianceObjective (got %r)" % (type(thermalCompliance).__name__,))
        P = float(P)
        if not np.isfinite(P) or P < 1.0:
            raise RuntimeError("PNormTemperatureObjective: P must be finite and at least 1 (got %r)" % (P,))
        self.solved, self.P = thermalCompliance, P
        self._sim = thermalCompliance._sim
        self._state = None

    _u = property(lambda s: s.solved._u)

    def updateCache(self, xPhys):
        sim, so = self._sim, self.solved
        if _set_densities(sim, xPhys) or so._u is None:
            so.updateCache(None)
        self._measure()

    def _measure(self):
        """the measure and its adjoint at the temperature the shared objective holds"""
        sim, so = self._sim, self.solved
        T = so._u
        if T is None:
            raise RuntimeError("PNormTemperatureObjective: updateCache(xPhys) has not been called")
        if self._state is not None and self._state["T"] is T:
            return self._state
        absT = T.abs().contiguous()
        J, top = ctypes.c_double(0.0), ctypes.c_double(0.0)
        _lib.check(_lib.load().vfem_stress_pnorm(absT.numel(), _ptr(absT), self.P, ctypes.byref(J), ctypes.byref(top), _stream()))
        J, top = J.value, top.value
        if not np.isfinite(J):
            raise RuntimeError("PNormTemperatureObjective: the measure is not finite (%r)" % (J,))
        if J > 0.0:
            a = (absT / J) ** (self.P - 1.0) * torch.sign(T)
            a[sim._mask_dev.bool()] = 0.0
            last = None if self._state is None else self._state["lam"]
            lam = so._solve(a.contiguous(), last)
        else:
            lam = torch.zeros_like(T)
        self._state = dict(T=T, J=J, top=top, lam=lam, grad=None)
        return self._state

    def evaluate(self, xPhys=None):
        if xPhys is not None:
            self.updateCache(xPhys)
        return self._measure()["J"]

    def maxTemperature(self):
        """max |T| of the same field"""
        return self._measure()["top"]

    def adjoint_device(self):
        return self._measure()["lam"]

    def gradient_device(self):
        st = self._measure()
        if st["grad"] is None:
            st["grad"] = self._sim.bilinearGradient_device([-1.0], st["lam"].unsqueeze(0), st["T"].unsqueeze(0))
        return st["grad"].clone()

    def gradient(self):
        return _to_np(self.gradient_device())


# the two objectives as autograd nodes, the counterparts of ``loadcases.AggregateComplianceFunction``
class ThermalComplianceFunction(ObjectiveFunction):
    NAME = "thermalCompliance"


class PNormTemperatureFunction(ObjectiveFunction):
    NAME = "pNormTemperature"


def thermalCompliance(densities, objective):
    """J of ``objective`` (a ``ThermalComplianceObjective``) at the element densities ``densities`` (a device tensor of numElements
    values, float32 or float64) as a differentiable float64 scalar: backward is grad_output x ``objective.gradient_device()`` in the
    densities' dtype and shape.  The simulator is left holding these densities."""
    if not isinstance(objective, ThermalComplianceObjective):
        raise TypeError("thermalCompliance takes a ThermalComplianceObjective (got %r)" % (type(objective).__name__,))
    return ThermalComplianceFunction.apply(densities, objective)


def pNormTemperature(densities, objective):
    """J_P of ``objective`` (a ``PNormTemperatureObjective``) as a differentiable float64 scalar, as ``thermalCompliance``"""
    if not isinstance(objective, PNormTemperatureObjective):
        raise TypeError("pNormTemperature takes a PNormTemperatureObjective (got %r)" % (type(objective).__name__,))
    return PNormTemperatureFunction.apply(densities, objective)
