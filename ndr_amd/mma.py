"""Method of Moving Asymptotes on the device: the optimiser of the design loop for objectives whose gradient has either sign and
for up to eight inequality constraints (Svanberg 1987 / 2007 with a_i = 0, d_i = 1, c_i = c).

    compliance = pyVoxelFEM.ComplianceObjective(sim)
    stress = ObjectiveConstraint(PNormStressObjective(compliance), upperBound=limit)
    problem = pyVoxelFEM.TopologyOptimizationProblem(sim, compliance, [pyVoxelFEM.TotalVolumeConstraint(0.4), stress], [smooth])
    problem.setVars(x0); mma = MMAOptimizer(problem, xmin=xmin, xmax=xmax)
    for _ in range(60): change = mma.step()

The problem's constraints follow the project's convention (c_i(x) >= 0 is feasible), so MMA's f_i = -c_i.  One step takes the
gradients from the problem (already chained through its filters), moves the asymptotes, solves the convex separable subproblem
through its dual and hands the new variables to the problem: one ``setVars``, so one primal solve, per step.  The design vector,
the asymptotes and the gradients stay on the device; every n-sized operation is a kernel of ``libvfem.so`` (``vfem_mma_*``,
include/vfem.h), the m x m Newton iteration on the multipliers runs on the host inside ``vfem_mma_subproblem``.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._grid import _dp
from .pyVoxelFEM import _dev, _ptr, _stream, _to_dev, _to_np

__all__ = ["MMAOptimizer", "ObjectiveConstraint", "VolumeObjective", "MAX_CONSTRAINTS"]

MAX_CONSTRAINTS = 8


class VolumeObjective:
    """J = mean(xPhys), the volume fraction: the objective of "the lightest design subject to ..." """

    def __init__(self):
        self._x = None

    def updateCache(self, xPhys):
        if xPhys is not None:
            self._x = _to_dev(xPhys).reshape(-1)

    def _need(self):
        if self._x is None:
            raise RuntimeError("VolumeObjective: updateCache(xPhys) has not been called")
        return self._x

    def evaluate(self, xPhys=None):
        if xPhys is not None:
            self.updateCache(xPhys)
        x, m = self._need(), ctypes.c_double(0.0)
        _lib.check(_lib.load().vfem_mean(x.numel(), _ptr(x), ctypes.byref(m), _stream()))
        return m.value

    def gradient_device(self):
        n = self._need().numel()
        return torch.full((n,), 1.0 / n, dtype=torch.float64, device=_dev())

    def gradient(self):
        return _to_np(self.gradient_device())


class ObjectiveConstraint:
    """Any objective of the project as the constraint  1 - J / upperBound >= 0.

    ``evaluate_dev(xPhys)`` calls ``objective.updateCache(xPhys)`` only when ``xPhys`` differs from the densities the objective
    stands at.  For an objective that reads a simulator (``objective._sim``: the compliance objectives and
    ``PNormStressObjective``, which solve inside ``updateCache`` right after setting the densities) it stands at ``xPhys`` when
    the simulator holds exactly ``xPhys`` (compared bit for bit on the device) and a solve has happened since the densities
    changed: the displacement of the solver it shares (``solved._u``, a new tensor with every solve) is not the one seen at
    this constraint's last call with other densities.  Densities set on the simulator without a solve are therefore solved for
    here.  (An objective that shares no solver with another one -- it has no ``solved`` -- is updated at its first use whatever
    its simulator holds: it may have been built with ``skipSolve``.)  For any other objective the densities it stands at are the
    ones this constraint handed to it last.  So a ``PNormStressObjective(compliance)`` beside the problem's own ``compliance``
    finds the densities ``problem.setVars`` has just set and solved for and adds only its adjoint solve: one primal and one
    adjoint solve per step, one factorisation.  An objective with a simulator of its own sees other densities there and solves."""

    def __init__(self, objective, upperBound):
        upperBound = float(upperBound)
        if not np.isfinite(upperBound) or not upperBound > 0.0:
            raise RuntimeError("ObjectiveConstraint: upperBound must be positive and finite (got %r)" % (upperBound,))
        for name in ("updateCache", "evaluate", "gradient_device"):
            if not hasattr(objective, name):
                raise TypeError("ObjectiveConstraint takes an objective with updateCache / evaluate / gradient_device")
        self.objective, self.upperBound = objective, upperBound
        self._seen = self._seen_u = None            # the densities of the last call and the solver's displacement then

    def _displacement(self):
        o = self.objective
        while hasattr(o, "solved"):
            o = o.solved
        return getattr(o, "_u", None)

    def _stands_at(self, x):
        same = lambda t: t is not None and t.shape == x.shape and torch.equal(t, x)
        sim = getattr(self.objective, "_sim", None)
        if sim is None:
            return same(self._seen)
        if self._seen is None and not hasattr(self.objective, "solved"):
            return False                            # nobody else updates it, and it may have been built with skipSolve
        if not same(sim.getDensities_device()):
            return False
        return self._seen is None or same(self._seen) or self._displacement() is not self._seen_u

    def _update(self, xPhys):
        x = _to_dev(xPhys).reshape(-1)
        if not self._stands_at(x):
            self.objective.updateCache(x)
        if not (self._seen is not None and self._seen.shape == x.shape and torch.equal(self._seen, x)):
            self._seen = x.clone()
        self._seen_u = self._displacement()

    def evaluate_dev(self, xPhys):
        self._update(xPhys)
        return 1.0 - float(self.objective.evaluate()) / self.upperBound

    def evaluate(self, xPhys):
        return self.evaluate_dev(xPhys)

    def backprop_dev(self, xPhys):
        self._update(xPhys)
        return self.objective.gradient_device().reshape(-1) * (-1.0 / self.upperBound)

    def backprop(self, xPhys):
        return _to_np(self.backprop_dev(xPhys))


class MMAOptimizer:
    """``step()`` moves the problem's variables by one MMA step and returns the largest |x_new - x|.

    ``problem`` is a ``TopologyOptimizationProblem`` (any filters) or anything with its ``numVars``, ``getVars_device``, ``setVars``,
    ``evaluateObjectiveGradient_device``, ``evaluateConstraints`` and ``evaluateConstraintsJacobian_device``; it holds 1 to 8
    constraints of any class with ``evaluate_dev`` / ``backprop_dev``.  ``xmin`` / ``xmax`` are scalars or arrays of ``numVars``
    (numpy or device); ``xmin == xmax`` freezes a variable (passive regions, cut-outs).  The variables must lie within them.
    ``c`` is the price of violating a constraint of the subproblem (its y_i), ``move`` the largest step as a fraction of
    xmax - xmin, ``asyinit`` / ``asyincr`` / ``asydecr`` the asymptote rule, ``tol`` / ``maxDualIterations`` the dual's stopping
    rule (relative to the scale of each constraint's sums) and its cap: reaching the cap raises, the variables stay."""

    def __init__(self, problem, xmin=0.0, xmax=1.0, move=0.5, c=1000.0, asyinit=0.5, asyincr=1.2, asydecr=0.7, tol=1e-9,
                 maxDualIterations=200):
        self._p = problem
        self._n = int(problem.numVars())
        self._xmin, self._xmax = self._bound(xmin, "xmin"), self._bound(xmax, "xmax")
        if bool((self._xmin > self._xmax).any()):
            raise RuntimeError("MMAOptimizer: xmin exceeds xmax")
        self.move, self.c, self.tol = float(move), float(c), float(tol)
        self.asyinit, self.asyincr, self.asydecr = float(asyinit), float(asyincr), float(asydecr)
        self.maxDualIterations = int(maxDualIterations)
        self.reset()

    def _bound(self, v, name):
        if np.ndim(v) == 0 and not isinstance(v, torch.Tensor):
            return torch.full((self._n,), float(v), dtype=torch.float64, device=_dev())
        t = _to_dev(v).reshape(-1)
        if t.numel() == 1:
            t = t.expand(self._n)
        if t.numel() != self._n:
            raise RuntimeError("MMAOptimizer: %s has %d entries, the problem %d variables" % (name, t.numel(), self._n))
        return t.clone().contiguous()

    def reset(self):
        """forget the history: the next step starts the asymptotes afresh"""
        self._it = 0
        self._xold1 = self._xold2 = None
        self._L = torch.empty(self._n, dtype=torch.float64, device=_dev())
        self._U = torch.empty(self._n, dtype=torch.float64, device=_dev())
        self._lambdas = None
        self._dual_iterations = 0

    iteration = property(lambda s: s._it, doc="steps taken since the last reset")
    lambdas = property(lambda s: None if s._lambdas is None else s._lambdas.copy(), doc="multipliers of the last subproblem")
    dualIterations = property(lambda s: s._dual_iterations, doc="Newton iterations of the last dual solve")

    def asymptotes_device(self):
        """(L, U) of the last step"""
        if self._it == 0:
            raise RuntimeError("MMAOptimizer: no step taken yet")
        return self._L, self._U

    def step(self):
        p, n, lib = self._p, self._n, _lib.load()
        x = p.getVars_device().reshape(-1).contiguous().clone()
        if bool(((x < self._xmin) | (x > self._xmax)).any()):
            raise RuntimeError("MMAOptimizer: the problem's variables leave [xmin, xmax]; set them inside first")
        g0 = p.evaluateObjectiveGradient_device().reshape(-1).contiguous()
        values = np.asarray(p.evaluateConstraints(), dtype=np.float64).reshape(-1)
        rows = p.evaluateConstraintsJacobian_device()
        m = len(rows)
        if m < 1 or m > MAX_CONSTRAINTS or values.size != m:
            raise RuntimeError("MMAOptimizer takes 1 to %d constraints (the problem has %d)" % (MAX_CONSTRAINTS, m))
        if g0.numel() != n or any(r.numel() != n for r in rows):
            raise RuntimeError("MMAOptimizer: a gradient's size differs from numVars")
        g = -torch.stack([r.reshape(-1) for r in rows]).contiguous()        # f_i = -c_i
        f = np.ascontiguousarray(-values)
        it = self._it + 1
        old = lambda t: None if t is None else _ptr(t)
        L, U = self._L.clone(), self._U.clone()             # a step that raises leaves the optimiser as it was
        _lib.check(lib.vfem_mma_asymptotes(n, it, _ptr(x), old(self._xold1), old(self._xold2), _ptr(self._xmin), _ptr(self._xmax),
                                           self.asyinit, self.asyincr, self.asydecr, _ptr(L), _ptr(U), _stream()))
        xnew = torch.empty_like(x)
        lam, its = np.zeros(m), ctypes.c_int(0)
        _lib.check(lib.vfem_mma_subproblem(n, m, _ptr(x), _ptr(L), _ptr(U), _ptr(self._xmin), _ptr(self._xmax), self.move,
                                           _dp(f), _ptr(g0), _ptr(g), self.c, self.tol, self.maxDualIterations, _ptr(xnew),
                                           _dp(lam), None, ctypes.byref(its), None, _stream()))
        self._it, self._xold2, self._xold1, self._L, self._U = it, self._xold1, x, L, U
        self._lambdas, self._dual_iterations = lam, its.value
        p.setVars(xnew)
        return float((xnew - x).abs().max())
