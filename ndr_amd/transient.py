"""Transient heat conduction on the device: the capacity operator of a ``HeatConductionSimulator``, the theta-scheme march, its
discrete adjoint, the time-accumulated density gradient and two objectives over the whole history.

    heat = HeatConductionSimulator([[0, 0], [1, 1]], [64, 64])
    heat.fixTemperatureInBox([0, 0.45], [0, 0.55])
    heat.setHeatSources(volumetric=1.0)
    pulse = np.where(np.arange(17) <= 8, 1.0, 0.0)                       # the source is on for the first half of 16 steps
    tr = TransientHeatSimulator(heat, capacity=1.0)
    work = TransientComplianceObjective(tr, steps=16, dt=0.01, sourceScale=pulse)
    peak = TransientPNormTemperatureObjective(tr, steps=16, dt=0.01, sourceScale=pulse, P=8.0)
    problem = pyVoxelFEM.TopologyOptimizationProblem(heat, work, [pyVoxelFEM.TotalVolumeConstraint(0.4),
                                                                  mma.ObjectiveConstraint(peak, bound)], [smooth])
    mma.MMAOptimizer(problem).step()

The numerics run in ``libvfem.so`` (``vfem_transient_*``, include/vfem.h); DESIGN 3.18 has the formulas.  With the element capacity
c_e = c_min + rho_e^q (1 - c_min), the capacity matrix Mc0 of a full voxel (consistent, row-sum lumped, or a blend) and the
conduction operator of the wrapped simulator,

    C = sum_e c_e Mc0,    A = P (C / dt + theta K) P + (I - P),    B = P (C / dt - (1 - theta) K) P,
    T^0 = P T_init,       A T^n = B T^(n-1) + (theta s_n + (1 - theta) s_(n-1)) P Q,        n = 1 .. steps,
    A lam^S = P dj_S/dT,  A lam^n = P (dj_n/dT + B lam^(n+1)),
    dJ/drho_e = -sum_n (c'_e / dt lam_e^n . Mc0 (T_e^n - T_e^(n-1)) + kappa'_e lam_e^n . Kc0 (theta T_e^n + (1 - theta) T_e^(n-1))).

A is the same for every step of a design and of its adjoint, so one band factorisation or one multigrid hierarchy serves
2 x steps solves; it is positive definite without a sink.  A trajectory is a tensor [steps + 1, numNodes]: (steps + 1) x numNodes x 8
bytes, kept whole (no checkpointing).

Both objectives have gradients of either sign: they are objectives and constraints for ``ndr_amd.mma.MMAOptimizer`` or a torch
optimiser, not for ``OCOptimizer``.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._grid import ObjectiveFunction, _dp
from .pyVoxelFEM import _dev, _ptr, _stream, _to_dev, _to_np
from .thermal import HeatConductionSimulator, _check_solver, _KeptSolvers, _set_densities

__all__ = ["TransientHeatSimulator", "TransientComplianceObjective", "TransientPNormTemperatureObjective", "TransientComplianceFunction",
           "TransientPNormTemperatureFunction", "transientCompliance", "transientPNormTemperature", "capacityEntries"]


def capacityEntries(h, capacity=1.0, lumping=0.0):
    """m[d], d = 0 .. N: the entry of the capacity matrix of a voxel with the edge lengths ``h`` for two local nodes that differ along d
    axes, m[d] = capacity ((1 - lumping) vol 2^(N - d) / 6^N + lumping [d = 0] vol / 2^N)"""
    h = np.asarray(h, dtype=np.float64)
    N, vol = h.size, float(np.prod(h))
    m = np.array([(1.0 - lumping) * vol * 2.0 ** (N - d) / 6.0 ** N for d in range(N + 1)])
    m[0] += lumping * vol / 2.0 ** N
    return np.ascontiguousarray(capacity * m)


def _scheme(who, dt, theta):
    dt, theta = float(dt), float(theta)
    if not np.isfinite(dt) or not dt > 0.0:
        raise RuntimeError("%s: dt must be positive and finite (got %r)" % (who, dt))
    if not 0.5 <= theta <= 1.0:
        raise RuntimeError("%s: theta must be in [0.5, 1] (got %r)" % (who, theta))
    return dt, theta


class TransientHeatSimulator:
    """The heat capacity and the time march of a ``HeatConductionSimulator``, whose densities, mask, conductivity and sources it
    shares.  ``capacity`` (per unit volume, positive), ``capacityExponent`` q >= 1 and ``c_min`` in [0, 1): c_e = c_min + rho_e^q
    (1 - c_min) multiplies the capacity matrix of a full voxel; ``lumping`` in [0, 1] blends the consistent matrix (0) with the
    row-sum lumped one (1).

    ``march_device`` factorises the band of A = C / dt + theta K once (``solver="direct"``) or builds one multigrid hierarchy
    (``solver="pcg", preconditioner="multigrid"``) and keeps it for the adjoint march and for later marches, until the wrapped
    simulator's densities, material or mask change (the events that drop its own factor), or dt, theta or a capacity parameter
    does.  A sink is not required."""

    def __init__(self, heat, capacity=1.0, capacityExponent=1.0, c_min=1e-3, lumping=0.0):
        if not isinstance(heat, HeatConductionSimulator):
            raise TypeError("TransientHeatSimulator takes a HeatConductionSimulator (got %r)" % (type(heat).__name__,))
        self.heat = heat
        self._capacity, self._q, self._c_min, self._lumping = 1.0, 1.0, 1e-3, 0.0
        self._kept = _KeptSolvers()         # the band factor and the multigrid hierarchy of A,
        self._kept_at = None                #   and what they stand for: (heat's version, dt, theta)
        self._march = None                  # the scheme and the solver of the last march, for the adjoint
        self.last_iterations = []
        self.capacity, self.capacityExponent, self.c_min, self.lumping = capacity, capacityExponent, c_min, lumping

    # ---- parameters ----
    def _param(name, test, rule):
        attr = "_" + {"capacity": "capacity", "capacityExponent": "q", "c_min": "c_min", "lumping": "lumping"}[name]

        def setter(self, v):
            v = float(v)
            if not np.isfinite(v) or not test(v):
                raise RuntimeError("TransientHeatSimulator: %s must be %s (got %r)" % (name, rule, v))
            setattr(self, attr, v)
            self._drop()
        return property(lambda self: getattr(self, attr), setter)

    capacity = _param("capacity", lambda v: v > 0.0, "positive and finite")
    capacityExponent = _param("capacityExponent", lambda v: v >= 1.0, "finite and at least 1")
    c_min = _param("c_min", lambda v: 0.0 <= v < 1.0, "in [0, 1)")
    lumping = _param("lumping", lambda v: 0.0 <= v <= 1.0, "in [0, 1]")
    del _param

    def _drop(self):
        self._kept_at = None
        self._kept.drop()

    def numDirectFactorizations(self):
        return self._kept.factorizations

    def numMultigridBuilds(self):
        return self._kept.builds

    def numNodes(self):
        return self.heat.numNodes()

    def numElements(self):
        return self.heat.numElements()

    def capacityEntries(self):
        return capacityEntries(self.heat._h, self._capacity, self._lumping)

    def elementCapacities_device(self):
        """(c, dc/drho) [numElements] at the present densities"""
        rho, q, span = self.heat._rho, self._q, 1.0 - self._c_min
        return (self._c_min + rho ** q * span).contiguous(), (q * rho ** (q - 1.0) * span).contiguous()

    def elementCapacities(self):
        return tuple(_to_np(t) for t in self.elementCapacities_device())

    # ---- operators ----
    def _operator(self, a, b):
        """the host arrays and element fields of A(a Kc0, b m)"""
        Ka = np.ascontiguousarray(float(a) * self.heat._K())
        mb = np.ascontiguousarray(float(b) * self.capacityEntries())
        return Ka, mb, self.heat.elementConductivities_device()[0], self.elementCapacities_device()[0]

    def applyOperator_device(self, a, b, X, identity=True, add=None):
        """A(a Kc0, b m) X (+ P add) for one field [numNodes] or a block [columns <= 8, numNodes]; ``identity``: a fixed node keeps
        its own value (otherwise 0)"""
        X = _to_dev(X)
        cols = 1 if X.dim() == 1 else X.shape[0]
        if X.numel() != cols * self.numNodes():
            raise RuntimeError("Invalid input size")
        if add is not None:
            add = _to_dev(add)
            if add.shape != X.shape:
                raise RuntimeError("Invalid input size")
        Ka, mb, kappa, cap = self._operator(a, b)
        out = torch.empty_like(X)
        _lib.check(_lib.load().vfem_transient_apply(*self.heat._head(), _dp(Ka), _dp(mb), _ptr(kappa), _ptr(cap), self.heat._fixed(),
                                                    1 if identity else 0, cols, _ptr(X), None if add is None else _ptr(add), _ptr(out),
                                                    _stream()))
        return out

    def applyOperator(self, a, b, X, identity=True, add=None):
        return _to_np(self.applyOperator_device(a, b, X, identity, add))

    def applyC_device(self, X):
        """P C P X"""
        return self.applyOperator_device(0.0, 1.0, X, identity=False)

    def applyC(self, X):
        return _to_np(self.applyC_device(X))

    def diagonal_device(self, dt, theta=1.0):
        dt, theta = _scheme("diagonal_device", dt, theta)
        Ka, mb, kappa, cap = self._operator(theta, 1.0 / dt)
        out = torch.empty(self.numNodes(), dtype=torch.float64, device=_dev())
        _lib.check(_lib.load().vfem_transient_diagonal(*self.heat._head(), _dp(Ka), _dp(mb), _ptr(kappa), _ptr(cap), self.heat._fixed(),
                                                       _ptr(out), _stream()))
        return out

    def assembleBand_device(self, dt, theta=1.0):
        """the lower band of A = P (C / dt + theta K) P + (I - P) in the tile layout of ``vfem_band_spd_factor`` (a new buffer)"""
        dt, theta = _scheme("assembleBand_device", dt, theta)
        Ka, mb, kappa, cap = self._operator(theta, 1.0 / dt)
        band = torch.zeros(self.heat.directBandBytes() // 8, dtype=torch.float64, device=_dev())
        _lib.check(_lib.load().vfem_transient_band_assemble(*self.heat._head(), _dp(Ka), _dp(mb), _ptr(kappa), _ptr(cap),
                                                            self.heat._fixed(), _ptr(band), _stream()))
        return band

    # ---- the kept factor or hierarchy ----
    def _stand_at(self, dt, theta):
        key = (self.heat._version, dt, theta)
        if self._kept_at != key:
            self._drop()
            self._kept_at = key

    def _factor(self, dt, theta):
        self._stand_at(dt, theta)
        return self._kept.factor(lambda: self.assembleBand_device(dt, theta), *self.heat._band_geometry())

    def _multigrid(self, dt, theta):
        self._stand_at(dt, theta)

        def operator():
            Ka, mb, kappa, cap = self._operator(theta, 1.0 / dt)
            return ((*self.heat._head(), _dp(Ka), _dp(mb), _ptr(kappa), _ptr(cap), self.heat._fixed()),
                    (kappa, cap, self.heat._mask_dev, Ka, mb))
        return self._kept.multigrid(_lib.load().vfem_transient_mg_create, operator)

    def _solve(self, m, rhs, x0):
        """A^-1 rhs (rhs is zero at the fixed nodes) through the solver of the march ``m``; returns (x, iterations)"""
        lib = _lib.load()
        if m["solver"] == "direct":
            band = self._factor(m["dt"], m["theta"])
            n, w = self.heat._band_geometry()
            x = rhs.clone()
            _lib.check(lib.vfem_band_spd_solve(n, w, _ptr(band), _ptr(x), 1, _stream()))
            return x, 0
        x = torch.zeros_like(rhs) if x0 is None else x0.clone()
        it, rel = ctypes.c_int(0), ctypes.c_double(0.0)
        if m["preconditioner"] == "multigrid":
            status = lib.vfem_thermal_mg_pcg(self._multigrid(m["dt"], m["theta"]), _ptr(rhs), _ptr(x), m["tol"], m["maxIter"],
                                             m["smoothing"], ctypes.byref(it), ctypes.byref(rel), _stream())
        else:
            Ka, mb, kappa, cap = self._operator(m["theta"], 1.0 / m["dt"])
            status = lib.vfem_transient_pcg(*self.heat._head(), _dp(Ka), _dp(mb), _ptr(kappa), _ptr(cap), self.heat._fixed(), _ptr(rhs),
                                            _ptr(x), m["tol"], m["maxIter"], ctypes.byref(it), ctypes.byref(rel), _stream())
        _lib.check(status)
        return x, int(it.value)

    # ---- the march and its adjoint ----
    def march_device(self, steps, dt, theta=1.0, T0=None, sourceScale=None, solver="direct", preconditioner="jacobi", tol=1e-8,
                     maxIter=2000, smoothing=1):
        """the trajectory [steps + 1, numNodes] from ``T0`` (default 0; projected) under the simulator's load vector scaled by
        ``sourceScale`` [steps + 1] (default 1).  ``solver``: "direct" or "pcg" (warm-started from the step before, with the
        ``preconditioner`` "jacobi" or "multigrid"); ``last_iterations`` lists the PCG count of every step."""
        steps = int(steps)
        if steps < 1:
            raise RuntimeError("march_device: steps must be at least 1 (got %r)" % (steps,))
        dt, theta = _scheme("march_device", dt, theta)
        _check_solver("march_device", solver, preconditioner)
        s =np.ones(steps + 1) if sourceScale is None else np.asarray(sourceScale, dtype=np.float64).reshape(-1)
        if s.size != steps + 1 or not np.isfinite(s).all():
            raise RuntimeError("march_device: sourceScale holds steps + 1 = %d finite values" % (steps + 1))
        n = self.numNodes()
        m = dict(steps=steps, dt=dt, theta=theta, s=s, solver=solver, preconditioner=preconditioner, tol=float(tol), maxIter=int(maxIter),
                 smoothing=int(smoothing), version=self.heat._version)
        T = torch.zeros((steps + 1, n), dtype=torch.float64, device=_dev())
        if T0 is not None:
            T[0] = _to_dev(T0, (n,))
            T[0, self.heat._mask_dev.bool()] = 0.0
        Q = self.heat.buildLoadVector_device()
        self.last_iterations = []
        for k in range(1, steps + 1):
            rhs = self.applyOperator_device(-(1.0 - theta), 1.0 / dt, T[k - 1], identity=False,
                                            add=(theta * s[k] + (1.0 - theta) * s[k - 1]) * Q)
            T[k], it = self._solve(m, rhs, T[k - 1])
            self.last_iterations.append(it)
        self._march = m
        return T

    def march(self, *args, **kwargs):
        return _to_np(self.march_device(*args, **kwargs))

    def adjointMarch_device(self, dJdT, march=None):
        """Lam [steps + 1, numNodes] (row 0 zero) of J = sum_{n >= 1} j_n(T^n) from ``dJdT`` [steps + 1, numNodes] (row 0 ignored), with
        the scheme and through the factor or hierarchy of the last march (or of ``march``, what ``lastMarch()`` returned after one)"""
        m = self._march if march is None else march
        if m is None:
            raise RuntimeError("adjointMarch_device: march_device has not been called")
        if m["version"] != self.heat._version:
            raise RuntimeError("adjointMarch_device: the simulator changed since the march")
        steps, dt, theta = m["steps"], m["dt"], m["theta"]
        dJdT = _to_dev(dJdT, (steps + 1, self.numNodes()))
        fixed = self.heat._mask_dev.bool()
        Lam = torch.zeros_like(dJdT)
        iterations = []
        for k in range(steps, 0, -1):
            if k == steps:
                rhs = dJdT[k].clone()
                rhs[fixed] = 0.0
            else:
                rhs = self.applyOperator_device(-(1.0 - theta), 1.0 / dt, Lam[k + 1], identity=False, add=dJdT[k])
            Lam[k], it = self._solve(m, rhs, None if k == steps else Lam[k + 1])
            iterations.append(it)
        self.last_adjoint_iterations = iterations
        return Lam

    def adjointMarch(self, dJdT, march=None):
        return _to_np(self.adjointMarch_device(dJdT, march))

    def lastMarch(self):
        """the scheme and the solver settings of the last march, for ``adjointMarch_device`` after another march has run"""
        return self._march

    def gradient_device(self, T, Lam, dt=None, theta=None):
        """dJ/drho [numElements] from a trajectory and its adjoint (``vfem_transient_gradient``); dt and theta default to those of the
        last march"""
        m = self._march
        if (dt is None or theta is None) and m is None:
            raise RuntimeError("gradient_device: march_device has not been called")
        dt, theta = _scheme("gradient_device", m["dt"] if dt is None else dt, m["theta"] if theta is None else theta)
        T = _to_dev(T)
        if T.dim() != 2 or T.shape[0] < 2 or T.shape[1] != self.numNodes():
            raise RuntimeError("gradient_device: the trajectory is [steps + 1, numNodes]")
        Lam = _to_dev(Lam, tuple(T.shape))
        dkappa, dcap = self.heat.elementConductivities_device()[1], self.elementCapacities_device()[1]
        Kc0, mc = self.heat._K(), self.capacityEntries()
        out = torch.empty(self.numElements(), dtype=torch.float64, device=_dev())
        _lib.check(_lib.load().vfem_transient_gradient(*self.heat._head(), T.shape[0] - 1, _dp(Kc0), _dp(mc), dt, theta, _ptr(dkappa),
                                                       _ptr(dcap), _ptr(T), _ptr(Lam), _ptr(out), _stream()))
        return out

    def gradient(self, T, Lam, dt=None, theta=None):
        return _to_np(self.gradient_device(T, Lam, dt, theta))


class _TransientObjective:
    """what the two objectives share: the march at every update, the adjoint march and the gradient on demand.  The objective protocol
    of the design loop: ``updateCache(xPhys)``, ``evaluate()``, ``gradient_device()``, ``gradient()``; ``_sim`` is the wrapped
    ``HeatConductionSimulator`` (what the design problem sets densities on) and ``_u`` the trajectory, a new tensor with every
    march."""

    def __init__(self, transient, steps, dt, theta=1.0, T0=None, sourceScale=None, solver="direct", preconditioner="jacobi", skipSolve=False):
        name = type(self).__name__
        if not isinstance(transient, TransientHeatSimulator):
            raise TypeError("%s takes a TransientHeatSimulator (got %r)" % (name, type(transient).__name__))
        self.transient, self._sim = transient, transient.heat
        self.steps = int(steps)
        if self.steps < 1:
            raise RuntimeError("%s: steps must be at least 1 (got %r)" % (name, steps))
        self.dt, self.theta = _scheme(name, dt, theta)
        _check_solver(name, solver, preconditioner)
        self.solver, self.preconditioner = solver, preconditioner
        self.tol, self.maxIter, self.smoothing = 1e-8, 2000, 1
        self.T0 = None if T0 is None else _to_dev(T0, (self._sim.numNodes(),)).clone()
        self.s = np.ones(self.steps + 1) if sourceScale is None else np.asarray(sourceScale, dtype=np.float64).reshape(-1).copy()
        if self.s.size != self.steps + 1 or not np.isfinite(self.s).all():
            raise RuntimeError("%s: sourceScale holds steps + 1 = %d finite values" % (name, self.steps + 1))
        self.iterations = []
        self._u = self._Q = self._J = self._lam = self._grad = None
        if not skipSolve:
            self.updateCache(None)

    def updateCache(self, xPhys):
        sim = self._sim
        _set_densities(sim, xPhys)
        T =self.transient.march_device(self.steps, self.dt, self.theta, self.T0, self.s, self.solver, self.preconditioner, self.tol,
                                        self.maxIter, self.smoothing)
        self.iterations = list(self.transient.last_iterations)
        self._marched = self.transient.lastMarch()
        self._Q = sim.buildLoadVector_device()
        self._u, self._lam, self._grad = T, None, None
        self._J = self._measure(T)
        if not np.isfinite(self._J):
            raise RuntimeError("%s: the objective is not finite (%r)" % (type(self).__name__, self._J))

    def _need(self):
        if self._u is None:
            raise RuntimeError("%s: updateCache(xPhys) has not been called" % type(self).__name__)

    def evaluate(self, xPhys=None):
        if xPhys is not None:
            self.updateCache(xPhys)
        self._need()
        return self._J

    def adjoint_device(self):
        self._need()
        if self._lam is None:
            self._lam = self.transient.adjointMarch_device(self._dJdT(self._u), self._marched)
        return self._lam

    def gradient_device(self):
        self._need()
        if self._grad is None:
            self._grad = self.transient.gradient_device(self._u, self.adjoint_device(), self.dt, self.theta)
        return self._grad.clone()

    def gradient(self):
        return _to_np(self.gradient_device())

    def trajectory_device(self):
        self._need()
        return self._u

    def trajectory(self):
        return _to_np(self.trajectory_device())


class TransientComplianceObjective(_TransientObjective):
    """J(rho) = dt sum_{n >= 1} s_n Q . T^n: the work of the sources over the history of a ``TransientHeatSimulator``'s march
    (``steps, dt, theta, T0, sourceScale, solver, preconditioner`` as ``march_device`` takes them; attributes ``tol``, ``maxIter``,
    ``smoothing``).  The sources are read from the simulator at every update; they do not depend on the design."""

    def _measure(self, T):
        w = torch.from_numpy(self.dt * self.s[1:]).to(T.device)
        return float(torch.dot(w, T[1:] @ self._Q))

    def _dJdT(self, T):
        w = torch.from_numpy(self.dt * self.s).to(T.device)
        return w[:, None] * self._Q[None, :]


class TransientPNormTemperatureObjective(_TransientObjective):
    """J_P(rho) = (sum_{n >= 1} sum_i |T_i^n|^P)^(1/P): a smooth upper bound of the peak temperature over the whole history, evaluated
    scaled by the peak as ``PNormTemperatureObjective`` is (``vfem_stress_pnorm``).  ``maxTemperature()`` returns the peak and the
    step at which it is reached."""

    def __init__(self, transient, steps, dt, theta=1.0, T0=None, sourceScale=None, solver="direct", preconditioner="jacobi", P=8.0,
                 skipSolve=False):
        P = float(P)
        if not np.isfinite(P) or P < 1.0:
            raise RuntimeError("TransientPNormTemperatureObjective: P must be finite and at least 1 (got %r)" % (P,))
        self.P = P
        super().__init__(transient, steps, dt, theta, T0, sourceScale, solver, preconditioner, skipSolve)

    def _measure(self, T):
        absT = T[1:].abs().contiguous()
        J, top = ctypes.c_double(0.0), ctypes.c_double(0.0)
        _lib.check(_lib.load().vfem_stress_pnorm(absT.numel(), _ptr(absT), self.P, ctypes.byref(J), ctypes.byref(top), _stream()))
        self._top = top.value
        return J.value

    def _dJdT(self, T):
        out = torch.zeros_like(T)
        if self._J > 0.0:
            out[1:] = (T[1:].abs() / self._J) ** (self.P - 1.0) * torch.sign(T[1:])
        return out

    def maxTemperature(self):
        """(max |T_i^n| over n >= 1, the step n at which it is reached)"""
        self._need()
        step = 1 + int(torch.argmax(self._u[1:].abs().max(dim=1).values))
        return self._top, step


# the two objectives as autograd nodes, the counterparts of ``thermal.ThermalComplianceFunction``
class TransientComplianceFunction(ObjectiveFunction):
    NAME = "transientCompliance"


class TransientPNormTemperatureFunction(ObjectiveFunction):
    NAME = "transientPNormTemperature"


def transientCompliance(densities, objective):
    """J of ``objective`` (a ``TransientComplianceObjective``) at the element densities ``densities`` as a differentiable float64
    scalar: backward is grad_output x ``objective.gradient_device()`` in the densities' dtype and shape"""
    if not isinstance(objective, TransientComplianceObjective):
        raise TypeError("transientCompliance takes a TransientComplianceObjective (got %r)" % (type(objective).__name__,))
    return TransientComplianceFunction.apply(densities, objective)


def transientPNormTemperature(densities, objective):
    """J_P of ``objective`` (a ``TransientPNormTemperatureObjective``), as ``transientCompliance``"""
    if not isinstance(objective, TransientPNormTemperatureObjective):
        raise TypeError("transientPNormTemperature takes a TransientPNormTemperatureObjective (got %r)" % (type(objective).__name__,))
    return TransientPNormTemperatureFunction.apply(densities, objective)
