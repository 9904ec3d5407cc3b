"""Von Mises stress of a solved design on the device: the element fields, a p-norm measure of the peak stress, and that measure's
gradient with respect to the densities by one adjoint solve.

    u   = objective._u                                  # or sim.solve_device(f)
    vm  = vonMises_device(sim, u)                       # [numElements]: where does it yield?
    obj = PNormStressObjective(pyVoxelFEM.ComplianceObjective(sim)); J, dJ = obj.evaluate(), obj.gradient_device()
    loss = pNormStress(densities, obj)                  # the same as an autograd node

for a degree-1 simulator in 2-D (plane stress) or 3-D holding any material.  The numerics run in ``libvfem.so`` (``vfem_stress_*``,
include/vfem.h); DESIGN 3.11 has the formulas.  Element e with nodal displacements u_e:

    eps_e   = the element's mean strain (``TensorProductSimulator::elementStrain`` of the reference; the strain at the centroid)
    sigma_e = m(rho_e) C : eps_e,   m(rho) = E_min + rho^q (E_0 - E_min),   q = ``stressExponent`` (None: q = gamma, the stress the
              SIMP material carries; q < gamma relaxes it so that low-density elements cannot hide their stress)
    vm_e    = von Mises stress of sigma_e,    J = (sum_e vm_e^P)^(1/P)

Strains and stresses hold TENSOR components in the order of ``ndr_amd.materials``: xx yy xy / xx yy zz yz xz xy.  The simulator is
only read by the field functions.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._grid import Grid, ObjectiveFunction, _dp, simp_multipliers
from .pyVoxelFEM import _dev, _ptr, _stream, _to_dev, _to_np

__all__ = ["elementStrains", "elementStrains_device", "elementStresses", "elementStresses_device", "vonMises", "vonMises_device",
           "PNormStressObjective", "PNormStressFunction", "pNormStress", "complianceAndPNormStress"]


def _exponent(sim, stressExponent):
    q = float(sim.gamma if stressExponent is None else stressExponent)
    if not q > 0.0:
        raise RuntimeError("stressExponent must be positive (got %r)" % (stressExponent,))
    return q


class _Grid(Grid):
    """what every ``vfem_stress_*`` grid call starts with, taken from a simulator: the grid, the voxel's edge lengths, the tensor"""

    def __init__(self, sim):
        super().__init__(sim, "element stresses need")
        self.S = 3 if self.N == 2 else 6
        self.D = np.ascontiguousarray(sim.ETensor.D)

    def head(self):
        return super().head(_dp(self.h), _dp(self.D))

    def displacement(self, u):
        """``u`` as a device tensor [numNodes, N] (a contiguous float64 device tensor is taken as it is)"""
        n = u.numel() if isinstance(u, torch.Tensor) else np.asarray(u).size
        if n != self.nnode * self.N:
            raise RuntimeError("Invalid input size: expected %d x %d displacement values, got %d" % (self.nnode, self.N, n))
        return _to_dev(u, (self.nnode, self.N))

    def multipliers(self, stressExponent):
        """(m, dm/drho) of the simulator's densities: m = E_min + rho^q (E_0 - E_min)"""
        sim = self.sim
        return simp_multipliers(sim, sim.getDensities_device()[:self.nelem], _exponent(sim, stressExponent))

    def fields(self, u, m, strain=False, stress=False, vm=False):
        new = lambda want, *shape: torch.empty(shape, dtype=torch.float64, device=_dev()) if want else None
        out = new(strain, self.nelem, self.S), new(stress, self.nelem, self.S), new(vm, self.nelem)
        opt = lambda t: None if t is None else _ptr(t)
        _lib.check(_lib.load().vfem_stress_fields(*self.head(), opt(m), _ptr(u), opt(out[0]), opt(out[1]), opt(out[2]), _stream()))
        return out


def elementStrains_device(sim, u):
    """[numElements, S]: every element's mean strain  eps_e = sum_j sym(g_j (x) u_j),  g_j = the mean of grad(phi_j)"""
    g = _Grid(sim)
    return g.fields(g.displacement(u), None, strain=True)[0]


def elementStresses_device(sim, u, stressExponent=None):
    """[numElements, S]: sigma_e = m(rho_e) C : eps_e with the simulator's tensor and densities"""
    g = _Grid(sim)
    u = g.displacement(u)
    return g.fields(u, g.multipliers(stressExponent)[0], stress=True)[1]


def vonMises_device(sim, u, stressExponent=None):
    """[numElements]: 3-D sqrt(((sxx - syy)^2 + (syy - szz)^2 + (szz - sxx)^2) / 2 + 3 (syz^2 + sxz^2 + sxy^2)), 2-D (plane stress)
    sqrt(sxx^2 - sxx syy + syy^2 + 3 sxy^2)"""
    g = _Grid(sim)
    u = g.displacement(u)
    return g.fields(u, g.multipliers(stressExponent)[0], vm=True)[2]


def elementStrains(sim, u):
    return _to_np(elementStrains_device(sim, u))


def elementStresses(sim, u, stressExponent=None):
    return _to_np(elementStresses_device(sim, u, stressExponent))


def vonMises(sim, u, stressExponent=None):
    return _to_np(vonMises_device(sim, u, stressExponent))


def _pnorm(vm, P):
    """(J, vmax) of a device array of von Mises stresses"""
    J, vmax = ctypes.c_double(0.0), ctypes.c_double(0.0)
    _lib.check(_lib.load().vfem_stress_pnorm(vm.numel(), _ptr(vm), float(P), ctypes.byref(J), ctypes.byref(vmax), _stream()))
    return J.value, vmax.value


class PNormStressObjective:
    """J(rho) = (sum_e vm_e^P)^(1/P), a smooth stand-in for the largest von Mises stress (``maxVonMises() <= J <= n^(1/P)
    maxVonMises()``), of the problem a compliance objective solves.  ``solved`` is a ``ComplianceObjective`` or a
    ``MultigridComplianceObjective``: this objective shares its simulator, load, solver settings and displacement.
    ``updateCache(xPhys)`` updates ``solved`` (one primal solve); ``gradient_device()`` adds one adjoint solve  K lambda = dJ/du
    through the same path (``sim.solve_device``, whose band factor is reused, or the multigrid objective's PCG from zero with its
    ``cgIter``, ``tol``, ``mgIterations``, ``mgSmoothingIterations``, ``fullMultigrid``; the hierarchy is not rebuilt), then

        dJ/drho_e = w_e q rho_e^(q-1) (E_0 - E_min) vm_e / m_e - gamma rho_e^(gamma-1) (E_0 - E_min) lambda_e^T K0 u_e,
        w_e = (vm_e / J)^(P-1).

    ``stressExponent`` defaults to 0.5 (None: gamma).  With q < 1 the first term is unbounded at rho = 0: keep the densities positive.

    Not an objective for ``OCOptimizer``: the optimality-criterion step takes sqrt(-dJ/drho) and so needs a gradient that is
    nowhere positive, which compliance has and this measure has not: adding material lowers the stress here and raises it there
    (the second term has either sign).  On a 6 x 4 cantilever with random densities 8 entries are positive and 16 negative
    (tests/test_stress_cpu.py).
    Minimise it, or cap it, with ``ndr_amd.mma.MMAOptimizer``, which takes gradients of either sign (as a constraint:
    ``mma.ObjectiveConstraint(objective, upperBound)``), or use ``pNormStress`` / ``complianceAndPNormStress`` with a torch optimiser
    or the MLP density field."""

    def __init__(self, solved, P=8.0, stressExponent=0.5):
        P = float(P)
        if not np.isfinite(P) or P < 1.0:
            raise RuntimeError("PNormStressObjective: P must be finite and at least 1 (got %r)" % (P,))
        if not (hasattr(solved, "_sim") and hasattr(solved, "_u") and hasattr(solved, "updateCache")):
            raise TypeError("PNormStressObjective takes a ComplianceObjective or a MultigridComplianceObjective")
        if getattr(solved, "designDependentLoad", False):
            raise RuntimeError("PNormStressObjective: the load of this case depends on the design (self-weight or eigenstrain): the "
                               "adjoint gradient lacks the lambda^T df/drho term")
        _Grid(solved._sim)                                   # refuses what the kernels do not take
        if stressExponent is not None and not float(stressExponent) > 0.0:
            raise RuntimeError("stressExponent must be positive (got %r)" % (stressExponent,))
        self._solved, self._sim = solved, solved._sim
        self.P, self.stressExponent = P, stressExponent
        self._state = None

    @property
    def solved(self):
        return self._solved

    def updateCache(self, xPhys):
        self._state = None
        self._solved.updateCache(xPhys)

    def _need(self):
        """the fields of the displacement ``solved`` holds now; computed once per displacement"""
        u = self._solved._u
        st = self._state
        if st is None or st["u"] is not u:
            g = _Grid(self._sim)
            m, dm = g.multipliers(self.stressExponent)
            vm = g.fields(u, m, vm=True)[2]
            J, vmax = _pnorm(vm, self.P)
            st = self._state = dict(u=u, grid=g, m=m, dm=dm, vm=vm, J=J, vmax=vmax, a=None, lam=None, grad=None)
        return st

    def evaluate(self, xPhys=None):
        if xPhys is not None:
            self.updateCache(xPhys)
        return self._need()["J"]

    def vonMises_device(self):
        return self._need()["vm"]

    def maxVonMises(self):
        return self._need()["vmax"]

    def adjointLoad_device(self):
        """dJ/du at fixed densities, [numNodes, N], zero at the Dirichlet components"""
        st = self._need()
        if st["a"] is None:
            g = st["grid"]
            a = torch.empty((g.nnode, g.N), dtype=torch.float64, device=_dev())
            work = torch.empty((g.nelem, g.S), dtype=torch.float64, device=_dev())          # scratch of the call
            _lib.check(_lib.load().vfem_stress_adjoint_load(*g.head(), _ptr(st["m"]), _ptr(st["u"]), st["J"], self.P, _ptr(g.mask),
                                                            _ptr(work), _ptr(a), _stream()))
            st["a"] = a
        return st["a"]

    def adjoint_device(self):
        """lambda = K^-1 dJ/du by the solver that produced u; the operator has not changed, so nothing is factorised or rebuilt"""
        st = self._need()
        if st["lam"] is None:
            a, s = self.adjointLoad_device(), self._solved
            mg = getattr(s, "_mg", None)
            if st["J"] == 0.0:
                st["lam"] = torch.zeros_like(a)              # no stress anywhere: a = 0, nothing to solve
            elif mg is None:
                st["lam"] = self._sim.solve_device(a)
            else:
                st["lam"] = mg.preconditionedConjugateGradient_device(torch.zeros_like(a), a, int(s.cgIter), float(s.tol), None,
                                                                      int(s.mgIterations), int(s.mgSmoothingIterations),
                                                                      bool(s.fullMultigrid))
        return st["lam"]

    def gradient_device(self):
        st = self._need()
        if st["grad"] is None:
            g, sim = st["grid"], self._sim
            lam = self.adjoint_device()
            dE = simp_multipliers(sim, sim.getDensities_device()[:g.nelem])[1]
            K0 = np.ascontiguousarray(sim.fullDensityElementStiffnessMatrix())
            out = torch.empty(g.nelem, dtype=torch.float64, device=_dev())
            _lib.check(_lib.load().vfem_stress_pnorm_gradient(*g.head(), _dp(K0), _ptr(st["m"]), _ptr(st["dm"]), _ptr(dE), _ptr(st["u"]),
                                                              _ptr(lam), st["J"], self.P, _ptr(out), _stream()))
            st["grad"] = out
        return st["grad"].clone()

    def gradient(self):
        return _to_np(self.gradient_device())


class PNormStressFunction(ObjectiveFunction):
    """(compliance, J) of the predicted densities as one autograd node, the stress counterpart of ``fem.VoxelFEMFunction``: forward
    sets the densities and solves once; backward is the two gradients weighted by the incoming gradient (the stress gradient costs
    its adjoint solve only where its weight is not zero)."""

    NAME = "pNormStress"
    field = staticmethod(lambda objective: objective.solved._u)

    @classmethod
    def forward(cls, ctx, densities, objective):
        cls.update(ctx, densities, objective)
        return torch.tensor([objective.solved.compliance(), objective.evaluate()], dtype=torch.float64, device=densities.device)

    @classmethod
    def backward(cls, ctx, grad_output):
        cls.refuse_stale(ctx)
        obj = ctx.objective
        wc, ws = (float(v) for v in grad_output.detach().cpu())
        g = torch.zeros(ctx.shape, dtype=torch.float64, device=grad_output.device).reshape(-1)
        if ws != 0.0:
            g = g + ws * obj.gradient_device()
        if wc != 0.0:
            g = g + wc * obj.solved.gradient_device()
        return g.to(ctx.dtype).reshape(ctx.shape), None


def complianceAndPNormStress(densities, objective):
    """the float64 tensor (compliance 1/2 f.u, J) of ``objective`` (a ``PNormStressObjective``) at the element densities
    ``densities`` (a device tensor of numElements values, float32 or float64), differentiable with respect to them; one primal
    solve serves both.  The simulator is left holding these densities."""
    return PNormStressFunction.apply(densities, objective)


def pNormStress(densities, objective):
    """J of ``objective`` at ``densities`` as a differentiable scalar: backward is grad_output x ``objective.gradient_device()`` in
    the densities' dtype and shape"""
    return complianceAndPNormStress(densities, objective)[1]
