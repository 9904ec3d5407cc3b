"""Load cases on the device: several loads per design, self-weight and thermal (eigenstrain) loads, and the compliance objective
over them with its density gradient.

    cases = [LoadCase(loads=loadsFromFile(sim, "left.bc")), LoadCase(loads=loadsFromFile(sim, "right.bc")),
             LoadCase(loads=0, acceleration=[0, -9.81], weight=0.5), LoadCase(loads=0, eigenstrain=thermalStrain(1.2e-5, 40.0, 2))]
    obj = LoadCaseComplianceObjective(sim, cases, aggregate="pnorm", P=8.0, mass=dict(massDensity=7.8))
    J, dJ = obj.evaluate(), obj.gradient_device()
    caps = [mma.ObjectiveConstraint(obj.case(i), bound) for i in range(len(cases))]       # the bound formulation of min-max
    loss = aggregateCompliance(densities, obj)                                            # the same as an autograd node

for a degree-1 simulator in 2-D (plane stress) or 3-D holding any material, whole grids, zero Dirichlet values.  The numerics run in
``libvfem.so`` (``vfem_loads_*``, include/vfem.h); DESIGN 3.15 has the formulas.  Case i has the load

    f_i(rho) = P (F_i + sum_e m(rho_e) Lb_i + sum_e E(rho_e) Lt_i),
    Lb_i[(n, a)] = vol / 2^N g_i[a],   Lt_i[(n, a)] = sum_q sigma*_i[a][q] s_nq vol / (2^(N-1) h_q),   sigma*_i = C : eps*_i,

P zeroing the Dirichlet components, F_i a fixed nodal load, m the mass law of ``modal.massMultipliers``, E = E_min + rho^gamma (E_0 -
E_min) the modulus of K, s_nq = +1 / -1 on the upper / lower face of axis q.  With K u_i = f_i:

    c_i = 1/2 f_i . u_i,    dc_i/drho_e = -1/2 dE_e u_ie^T K0 u_ie + dm_e Lb_i . u_ie + dE_e Lt_i . u_ie

(compliance stays self-adjoint with a design-dependent load: no adjoint solve), and with the case weights w_i

    "sum":   J = sum_i w_i c_i                      dJ/drho = sum_i w_i dc_i/drho
    "pnorm": J = (sum_i (w_i c_i)^P)^(1/P)          dJ/drho = sum_i w_i (w_i c_i / J)^(P-1) dc_i/drho.

With fixed loads only the gradient is nowhere positive and ``OCOptimizer`` works.  With self-weight or an eigenstrain it has both
signs (material added above a span weighs on it; on a 16 x 6 arch under its own weight tests/test_loadcases_cpu.py pins the
counts): use ``ndr_amd.mma.MMAOptimizer`` or ``aggregateCompliance`` with a torch optimiser.

A case may also carry the solved temperature field of a heat-conduction problem (``LoadCase(temperature=TemperatureLoad(...))``,
``ndr_amd.thermoelastic``): its load gains sum_e E(rho_e) G_i (T_e - T_ref), the objective solves the heat problem once per
design before it assembles, and the gradient gains dE_e u_ie^T G_i theta_e and the term of one thermal adjoint solve.
"""
import numpy as np
import torch

from . import _lib, modal
from ._grid import ObjectiveFunction, _dp, simp_multipliers
from .pyVoxelFEM import _dev, _matched_regions, _ptr, _stream, _to_dev, _to_np, _write_force_region, _MultigridSolver

__all__ = ["LoadCase", "thermalStrain", "loadsFromFile", "assembleLoad", "assembleLoad_device", "LoadCaseComplianceObjective",
           "AggregateComplianceFunction", "aggregateCompliance", "MAX_CASES"]

MAX_CASES = 8


def _opt(t):
    return None if t is None else _ptr(t)


def thermalStrain(alpha, deltaT, N):
    """the eigenstrain alpha deltaT I of a uniform temperature change ``deltaT`` at the expansion coefficient ``alpha``"""
    if int(N) not in (2, 3):
        raise RuntimeError("thermalStrain: N must be 2 or 3 (got %r)" % (N,))
    return float(alpha) * float(deltaT) * np.eye(int(N))


def loadsFromFile(sim, bcPath):
    """[numNodes, N] on the device: the nodal load of the ``force`` regions of a boundary-condition file, each split evenly over the
    nodes its box holds, as ``sim.applyDisplacementsAndLoadsFromFile`` writes them; the simulator is only read (its Dirichlet
    regions are ignored here)"""
    N = sim.N
    loads = torch.zeros(tuple(int(n) for n in sim._nn) + (N,), dtype=torch.float64, device=_dev())
    for kind, comps, value, sel, count in _matched_regions(sim, bcPath):
        if kind == "force":
            _write_force_region(loads, sel, value, count)
    return loads.reshape(-1, N)


class LoadCase:
    """One load case.  ``loads``: the fixed nodal load [numNodes, N] (numpy or device), ``None`` for the simulator's own
    ``buildLoadVector_device()`` (read when the case is handed to an objective or assembled), ``0`` for none.  ``acceleration``:
    N values g; the body force m(rho) g.  ``eigenstrain``: a symmetric N x N strain eps* the material would take on unloaded
    (``thermalStrain``); the load int B^T E(rho) C : eps*.  ``temperature``: a ``thermoelastic.TemperatureLoad``, the solved
    temperature field of a heat-conduction problem as a thermal load.  ``weight``: w_i > 0 in the aggregate."""

    def __init__(self, loads=None, acceleration=None, eigenstrain=None, weight=1.0, temperature=None):
        self.loads = loads
        self.acceleration = None if acceleration is None else np.array(acceleration, dtype=np.float64).reshape(-1)
        self.eigenstrain = None if eigenstrain is None else np.array(eigenstrain, dtype=np.float64)
        self.weight = float(weight)
        if not np.isfinite(self.weight) or not self.weight > 0.0:
            raise RuntimeError("LoadCase: weight must be positive and finite (got %r)" % (weight,))
        if self.acceleration is not None and not np.isfinite(self.acceleration).all():
            raise RuntimeError("LoadCase: the acceleration is not finite")
        if self.eigenstrain is not None:
            e = self.eigenstrain
            if e.ndim != 2 or e.shape[0] != e.shape[1] or not np.isfinite(e).all() or np.abs(e - e.T).max() > 1e-12 * max(np.abs(e).max(), 1e-300):
                raise RuntimeError("LoadCase: eigenstrain must be a finite symmetric N x N matrix")
        self.temperature = temperature
        if temperature is not None:
            from . import thermoelastic
            if not isinstance(temperature, thermoelastic.TemperatureLoad):
                raise TypeError("LoadCase: temperature is a thermoelastic.TemperatureLoad (got %r)" % (type(temperature).__name__,))

    @property
    def designDependent(self):
        return self.acceleration is not None or self.eigenstrain is not None or self.temperature is not None

    def _has_fixed(self):
        return not (self.loads is not None and not isinstance(self.loads, torch.Tensor) and np.ndim(self.loads) == 0
                    and float(self.loads) == 0.0)


class _Grid(modal._Grid):
    """what every ``vfem_loads_*`` call starts with (``modal._Grid``: the grid, the edge lengths, the node mask), refusing what the
    kernels do not take, and the element patterns and multipliers of a case"""

    def __init__(self, sim):
        super().__init__(sim, "load cases need")
        if np.any(sim._dvals[sim._mask] != 0):
            raise RuntimeError("load cases: nonzero Dirichlet values are not supported (the loads are those of the clamped body)")
        self.vol = float(np.prod(self.h))
        self.ke = self.N * 2 ** self.N

    def patterns(self, case):
        """(Lb, Lt) of a case: numpy [ke] each, or None"""
        N, npe = self.N, 2 ** self.N
        Lb = Lt = None
        if case.acceleration is not None:
            if case.acceleration.size != N:
                raise RuntimeError("LoadCase: acceleration has %d values, the simulator %d dimensions" % (case.acceleration.size, N))
            Lb = np.tile(self.vol / npe * case.acceleration, npe)
        if case.eigenstrain is not None:
            if case.eigenstrain.shape != (N, N):
                raise RuntimeError("LoadCase: eigenstrain is %s, the simulator has %d dimensions" % (case.eigenstrain.shape, N))
            sigma = np.asarray(self.sim.ETensor.doubleContract(case.eigenstrain), dtype=np.float64).reshape(N, N)
            Lt = np.empty(self.ke)
            for n in range(npe):
                s = np.array([1.0 if (n >> (N - 1 - q)) & 1 else -1.0 for q in range(N)])
                Lt[n * N:(n + 1) * N] = sigma @ (s * self.vol / (2.0 ** (N - 1) * self.h))
        for L in (Lb, Lt):
            if L is not None and not np.isfinite(L).all():
                raise RuntimeError("LoadCase: the element load pattern is not finite")
        return Lb, Lt

    def fixed_load(self, case):
        """the case's fixed nodal load as a device tensor [numNodes, N], or None"""
        if not case._has_fixed():
            return None
        if case.loads is None:
            return self.sim.buildLoadVector_device()
        n = case.loads.numel() if isinstance(case.loads, torch.Tensor) else np.asarray(case.loads).size
        if n != self.n:
            raise RuntimeError("Invalid input size: expected %d x %d load values, got %d" % (self.nnode, self.N, n))
        return _to_dev(case.loads, (self.nnode, self.N)).clone()

    def stiffness_multipliers(self, rho):
        return simp_multipliers(self.sim, rho)

    def assemble(self, F, Lb, Lt, m, E):
        """P (F + sum_e m Lb + sum_e E Lt) as a new device tensor; F may be None"""
        out = torch.empty((self.nnode, self.N), dtype=torch.float64, device=_dev())
        if Lb is None and Lt is None:               # a fixed load only: nothing to gather
            out.copy_(F)
            self.project(out.unsqueeze(0))
            return out
        _lib.check(_lib.load().vfem_loads_assemble(*self.head(), _dp(Lb), _dp(Lt), _ptr(m) if Lb is not None else None,
                                                   _ptr(E) if Lt is not None else None, _ptr(self.mask), _opt(F), _ptr(out), _stream()))
        return out


def _mass_law_args(mass):
    """the keywords of ``modal.massMultipliers`` with its defaults, as ``modal._mass_law`` takes them"""
    return dict(dict(massDensity=1.0, massExponent=1.0, lowDensityCut=None), **modal._mass_args(mass))


def _check_case(case):
    if not isinstance(case, LoadCase):
        raise TypeError("a load case is a LoadCase (got %r)" % (type(case).__name__,))
    return case


def assembleLoad_device(sim, case, mass=None):
    """f(rho) [numNodes, N] of ``case`` at the simulator's present densities, zero at the Dirichlet components.  ``mass``: the keywords
    of ``modal.massMultipliers`` as a dict."""
    g = _Grid(sim)
    case = _check_case(case)
    Lb, Lt = g.patterns(case)
    F = g.fixed_load(case)
    if case.temperature is not None:
        raise RuntimeError("assembleLoad: a case with a temperature field is assembled by LoadCaseComplianceObjective (its load "
                           "follows a heat solve)")
    if F is None and Lb is None and Lt is None:
        return torch.zeros((g.nnode, g.N), dtype=torch.float64, device=_dev())
    rho = sim.getDensities_device()[:g.nelem]
    m = modal._mass_law(rho, **_mass_law_args(mass))[0] if Lb is not None else None
    E = g.stiffness_multipliers(rho)[0] if Lt is not None else None
    return g.assemble(F, Lb, Lt, m, E)


def assembleLoad(sim, case, mass=None):
    return _to_np(assembleLoad_device(sim, case, mass))


class _CaseView:
    """Case ``i`` of a ``LoadCaseComplianceObjective`` as a solved compliance objective: ``_sim``, ``_u``, ``_f``, ``updateCache``
    (the parent's: all cases are solved together), ``compliance()``, ``evaluate()`` = c_i and ``gradient_device()`` = dc_i/drho.
    Over a multigrid solver it also has ``_mg`` and the PCG attributes of the parent.  ``designDependentLoad`` says whether the
    case has a self-weight or eigenstrain part: measures whose adjoint gradient lacks the lambda^T df/drho term refuse it then."""

    _PARENT = ("_mg", "cgIter", "tol", "mgIterations", "mgSmoothingIterations", "fullMultigrid", "zeroInit")

    def __init__(self, parent, i):
        self._parent, self._i = parent, i
        self._sim = parent._sim
        self.designDependentLoad = parent._cases[i].designDependent
        self._grad_u = self._grad = None

    def __getattr__(self, name):                # (only reached for names that are neither set on the instance nor defined by the class)
        if name in _CaseView._PARENT and self.__dict__["_parent"]._mg is not None:
            return getattr(self.__dict__["_parent"], name)
        raise AttributeError(name)

    solved = property(lambda s: s._parent, doc="the objective that solves this case (what `mma.ObjectiveConstraint` follows)")
    # (None before the first solve, as an attribute that exists: `mma.ObjectiveConstraint` compares it by identity)
    _u = property(lambda s: None if s._parent._state is None else s._parent._state["us"][s._i])
    _f = property(lambda s: None if s._parent._state is None else s._parent._state["fs"][s._i])

    def updateCache(self, xPhys):
        self._parent.updateCache(xPhys)

    def compliance(self):
        return float(self._parent.compliances()[self._i])

    def evaluate(self, xPhys=None):
        if xPhys is not None:
            self.updateCache(xPhys)
        return self.compliance()

    def gradient_device(self):
        u = self._u
        if self._grad is None or self._grad_u is not u:
            a = np.zeros(len(self._parent._cases))
            a[self._i] = 1.0
            self._grad, self._grad_u = self._parent._weighted_gradient(a, [self._i]), u
        return self._grad.clone()

    def gradient(self):
        return _to_np(self.gradient_device())

    def u(self):
        return _to_np(self._u)

    def f(self):
        return _to_np(self._f)


class LoadCaseComplianceObjective:
    """J(rho) = the weighted sum, or the weighted p-norm, of the compliances c_i = 1/2 f_i(rho) . u_i of 1 to 8 load cases
    (``LoadCase``), with its density gradient (the module's docstring has the formulas).

    ``solver`` is a simulator: every case is solved by ``sim.solve_device``, one factorisation per design for all cases (the band
    factor is kept until the operator changes).  Or it is a ``MultigridSolver`` of the simulator: every case is solved by its PCG
    with the attributes ``cgIter``, ``tol``, ``mgIterations``, ``mgSmoothingIterations``, ``fullMultigrid``, ``zeroInit`` (defaults
    those of ``MultigridComplianceObjective``), each case warm-started from its own last displacement; the hierarchy follows the
    densities once per design (a solve on unchanged moduli keeps it).  ``aggregate`` is "sum" or "pnorm" (``P`` >= 1; a smooth upper
    bound of the worst weighted case, max <= J <= k^(1/P) max).  ``mass``: the keywords of ``modal.massMultipliers`` for the
    self-weight.  The fixed loads are read at construction.  The constructor solves once unless ``skipSolve``.  Heated cases
    (``LoadCase(temperature=...)``) share one ``ThermalComplianceObjective``: every update solves it first, at the same densities, and
    every gradient adds one thermal adjoint solve through it (``ndr_amd.thermoelastic``).

    The objective protocol of the design loop: ``updateCache(xPhys)``, ``evaluate()``, ``gradient_device()``, ``gradient()``;
    also ``compliances()`` (host, [k]), ``displacements_device()`` ([k, numNodes, N]), ``loads_device()``; ``_u`` is case 0's
    displacement, a new tensor with every solve.  ``case(i)`` is a view of one case with what a solved compliance objective has:
    ``mma.ObjectiveConstraint(obj.case(i), bound)`` per case is the bound formulation of min-max compliance, and
    ``stress.PNormStressObjective(obj.case(i))`` / ``buckling.BucklingObjective(obj.case(i))`` cap the stress or the buckling load
    of a chosen (fixed-load) case with no further primal solve.

    With fixed loads only the gradient is nowhere positive and ``OCOptimizer`` works.  With self-weight or an eigenstrain it has
    both signs: use ``ndr_amd.mma.MMAOptimizer``, or ``aggregateCompliance`` with a torch optimiser."""

    def __init__(self, solver, cases, aggregate="sum", P=8.0, mass=None, skipSolve=False):
        if isinstance(solver, _MultigridSolver):
            self._mg, self._sim = solver, solver.getSimulator(0)
            self.cgIter, self.tol, self.mgIterations, self.mgSmoothingIterations = 100, 1e-5, 1, 2
            self.fullMultigrid, self.zeroInit = True, False
        else:
            self._mg, self._sim = None, solver
        g = _Grid(self._sim)                                  # refuses what the kernels do not take
        cases = list(cases)
        if len(cases) < 1 or len(cases) > MAX_CASES:
            raise RuntimeError("LoadCaseComplianceObjective takes 1 to %d load cases (got %d)" % (MAX_CASES, len(cases)))
        self._cases = [_check_case(c) for c in cases]
        for c in self._cases:
            if not np.isfinite(c.weight) or not c.weight > 0.0:
                raise RuntimeError("LoadCaseComplianceObjective: every weight must be positive and finite (got %r)" % (c.weight,))
        if aggregate not in ("sum", "pnorm"):
            raise RuntimeError("LoadCaseComplianceObjective: aggregate is \"sum\" or \"pnorm\" (got %r)" % (aggregate,))
        P = float(P)
        if not np.isfinite(P) or P < 1.0:
            raise RuntimeError("LoadCaseComplianceObjective: P must be finite and at least 1 (got %r)" % (P,))
        self.aggregate, self.P = aggregate, P
        self.mass = _mass_law_args(mass)
        modal._mass_law(torch.ones(1, dtype=torch.float64, device=_dev()), **self.mass)          # (refuses a bad law now)
        self._weights = np.array([c.weight for c in self._cases])
        self._fixed = [g.fixed_load(c) for c in self._cases]
        self._patterns = [g.patterns(c) for c in self._cases]
        k = len(self._cases)
        stack = lambda j: None if all(p[j] is None for p in self._patterns) else \
            np.ascontiguousarray(np.stack([np.zeros(g.ke) if p[j] is None else p[j] for p in self._patterns]))
        self._Lb, self._Lt = stack(0), stack(1)
        # the heated cases: one heat solve for all of them, a coupling matrix and a reference temperature each
        heated = [c.temperature for c in self._cases if c.temperature is not None]
        self._thermal = heated[0].thermal if heated else None
        for t in heated:
            if t.thermal is not self._thermal:
                raise RuntimeError("LoadCaseComplianceObjective: the heated cases of one objective share one ThermalComplianceObjective "
                                   "(several temperature fields are not supported)")
            t.check(self._sim)
        self._G = [None if c.temperature is None else c.temperature.couplingMatrix(self._sim) for c in self._cases]
        self._tref = [0.0 if c.temperature is None else c.temperature.referenceTemperature for c in self._cases]
        self._views = [_CaseView(self, i) for i in range(k)]
        self._state = None
        if not skipSolve:
            self.updateCache(None)

    numCases = property(lambda s: len(s._cases))
    weights = property(lambda s: s._weights.copy())
    # the objective has what a solved compliance objective has (`_sim`, `_u`, `_f`, `updateCache`) and stands for its case 0 there:
    # a measure built on it refuses it as it refuses that case's view
    designDependentLoad = property(lambda s: s._cases[0].designDependent)

    def case(self, i):
        i = int(i)
        if i < 0 or i >= len(self._cases):
            raise IndexError("LoadCaseComplianceObjective: case %d of %d" % (i, len(self._cases)))
        return self._views[i]

    def _solve(self, f, last):
        if self._mg is None:
            return self._sim.solve_device(f)
        x0 = torch.zeros_like(f) if last is None or self.zeroInit else last
        return self._mg.preconditionedConjugateGradient_device(x0, f, int(self.cgIter), float(self.tol), None, int(self.mgIterations),
                                                               int(self.mgSmoothingIterations), bool(self.fullMultigrid))

    def updateCache(self, xPhys):
        sim = self._sim
        if xPhys is not None:
            x = _to_dev(xPhys).reshape(-1)
            if not torch.equal(sim.getDensities_device()[:x.numel()], x):        # (setting them again would drop the band factor)
                sim.setElementDensities(x)
        g = _Grid(sim)
        rho = sim.getDensities_device()[:g.nelem]
        m = dm = None
        if self._Lb is not None:
            m, dm = modal._mass_law(rho, **self.mass)
        E, dE = g.stiffness_multipliers(rho)
        T = None
        if self._thermal is not None:               # the heat problem at the same densities, solved once for all heated cases
            self._thermal.updateCache(rho)
            T = self._thermal._u
        last = None if self._state is None else self._state["us"]
        k = len(self._cases)
        U = torch.empty((k, g.nnode, g.N), dtype=torch.float64, device=_dev())
        fs, iterations = [], []
        for i in range(k):
            Lb, Lt = self._patterns[i]
            F = self._fixed[i]
            if F is None and Lb is None and Lt is None:
                f = torch.zeros((g.nnode, g.N), dtype=torch.float64, device=_dev())
            else:
                f = g.assemble(F, Lb, Lt, m, E)
            if self._G[i] is not None:
                _lib.check(_lib.load().vfem_thermoelastic_load(*g.head(), _dp(self._G[i]), self._tref[i], _ptr(E), _ptr(T),
                                                               _ptr(g.mask), _ptr(f), _ptr(f), _stream()))
            fs.append(f)
            U[i].copy_(self._solve(f, None if last is None else last[i]))
            if self._mg is not None:
                iterations.append(int(self._mg.last_iterations))
        us = [U[i] for i in range(k)]
        c = np.array([sim._compliance(fs[i], us[i]) for i in range(k)])
        if not np.isfinite(c).all():
            raise RuntimeError("LoadCaseComplianceObjective: a compliance is not finite (%s)" % " ".join("%.3e" % v for v in c))
        wc = self._weights * c
        if self.aggregate == "sum":
            J, a = float(np.sum(wc)), self._weights.copy()
        else:
            top = float(wc.max())
            if top > 0.0:
                J = top * float(np.sum((wc / top) ** self.P)) ** (1.0 / self.P)
                a = self._weights * (wc / J) ** (self.P - 1.0)
            else:
                J, a = 0.0, np.zeros(k)
        self._state = dict(grid=g, U=U, us=us, fs=fs, c=c, J=J, a=a, dE=dE, dm=dm, iterations=iterations, grad=None,
                           E=E, T=T)

    def _need(self):
        if self._state is None:
            raise RuntimeError("LoadCaseComplianceObjective: updateCache(xPhys) has not been called")
        return self._state

    _u = property(lambda s: None if s._state is None else s._state["us"][0])
    _f = property(lambda s: None if s._state is None else s._state["fs"][0])

    def evaluate(self, xPhys=None):
        if xPhys is not None:
            self.updateCache(xPhys)
        return self._need()["J"]

    def compliances(self):
        return self._need()["c"].copy()

    def caseCoefficients(self):
        """a_i = dJ/dc_i [k]: w_i for the sum, w_i (w_i c_i / J)^(P-1) for the p-norm"""
        return self._need()["a"].copy()

    def displacements_device(self):
        return self._need()["U"]

    def loads_device(self):
        return torch.stack(self._need()["fs"])

    def iterations(self):
        """PCG iterations of the last update per case (multigrid solver only)"""
        return list(self._need()["iterations"])

    def _weighted_gradient(self, a, which=None):
        """sum_i a_i dc_i/drho over the cases ``which`` (default: all) in one kernel pass"""
        st = self._need()
        g, sim = st["grid"], self._sim
        idx = list(range(len(self._cases))) if which is None else list(which)
        a = np.asarray(a, dtype=np.float64)[idx]
        if which is None:
            U = st["U"]
        elif len(idx) == 1:
            U = st["us"][idx[0]]
        else:
            U = st["U"][idx].contiguous()
        Lb = None if self._Lb is None else np.ascontiguousarray(self._Lb[idx])
        Lt = None if self._Lt is None else np.ascontiguousarray(self._Lt[idx])
        if Lb is not None and not Lb.any():
            Lb = None
        if Lt is not None and not Lt.any():
            Lt = None
        K0 = np.ascontiguousarray(sim.fullDensityElementStiffnessMatrix())
        cK, cB, cT = np.ascontiguousarray(-0.5 * a), np.ascontiguousarray(a) if Lb is not None else None, \
            np.ascontiguousarray(a) if Lt is not None else None
        out = torch.empty(g.nelem, dtype=torch.float64, device=_dev())
        _lib.check(_lib.load().vfem_loads_gradient(*g.head(), len(idx), _dp(K0), _dp(cK), _dp(cB), _dp(cT), _dp(Lb), _dp(Lt),
                                                   _ptr(st["dE"]), _ptr(st["dm"]) if Lb is not None else None, _ptr(U), _ptr(out),
                                                   _stream()))
        hot = [j for j in idx if self._G[j] is not None]
        if hot:
            self._add_coupled_terms(st, a[[idx.index(j) for j in hot]], hot, out)
        return out

    def _add_coupled_terms(self, st, a, hot, out):
        """onto ``out``: dE_e sum_i a_i u_ie^T G_i theta_e - kappa'_e mu_e^T Kc0 T_e over the heated cases ``hot``, A mu = P_T sum_i
        a_i sum_e E_e G_i^T u_ie: one thermal adjoint solve through the thermal objective's own solver"""
        g, heat, lib = st["grid"], self._thermal._sim, _lib.load()
        a = np.ascontiguousarray(a)
        G = np.ascontiguousarray(np.stack([self._G[j] for j in hot]))
        tref = np.ascontiguousarray(np.array([self._tref[j] for j in hot], dtype=np.float64))
        U = st["us"][hot[0]] if len(hot) == 1 else (st["U"] if len(hot) == len(self._cases) else st["U"][hot].contiguous())
        _lib.check(lib.vfem_thermoelastic_gradient(*g.head(), len(hot), _dp(a), _dp(G), _dp(tref), _ptr(st["dE"]), _ptr(st["T"]),
                                                   _ptr(U), _ptr(out), _ptr(out), _stream()))
        q = torch.empty(g.nnode, dtype=torch.float64, device=_dev())
        _lib.check(lib.vfem_thermoelastic_adjoint_source(*g.head(), len(hot), _dp(a), _dp(G), _ptr(st["E"]), _ptr(U), heat._fixed(),
                                                         _ptr(q), _stream()))
        mu = self._thermal._solve(q)
        out += heat.bilinearGradient_device([-1.0], mu.unsqueeze(0), st["T"].unsqueeze(0))

    def gradient_device(self):
        st = self._need()
        if st["grad"] is None:
            st["grad"] = self._weighted_gradient(st["a"])
        return st["grad"].clone()

    def gradient(self):
        return _to_np(self.gradient_device())


class AggregateComplianceFunction(ObjectiveFunction):
    """J of the predicted densities as an autograd node, the counterpart of ``modal.MeanEigenvalueFunction``: forward sets the
    densities and solves every case; backward is ``gradient_device()`` weighted by the incoming gradient."""

    NAME = "aggregateCompliance"


def aggregateCompliance(densities, objective):
    """J of ``objective`` (a ``LoadCaseComplianceObjective``) at the element densities ``densities`` (a device tensor of numElements
    values, float32 or float64) as a differentiable float64 scalar: backward is grad_output x ``objective.gradient_device()`` in the
    densities' dtype and shape.  The simulator is left holding these densities."""
    return AggregateComplianceFunction.apply(densities, objective)
