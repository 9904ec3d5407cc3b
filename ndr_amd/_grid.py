"""What the feature modules built on the handle-free grid calls of ``libvfem.so`` (stress, modal, buckling, loadcases,
homogenization; thermal and mma for the pointer helper and the autograd base) share: the grid taken from a simulator, the SIMP
multiplier law, and an objective as an autograd node."""
import ctypes

import numpy as np
import torch

from .pyVoxelFEM import _dev


def _dp(a):
    """a contiguous float64 numpy array (or None) as the ``double *`` of a call"""
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class Grid:
    """what every grid call starts with, taken from a degree-1 simulator that stores the whole grid: ``N``, ``ne``, ``nelem``,
    ``nnode``, the voxel's edge lengths ``h``, ``head(...)`` and the node mask.  ``needs`` ("element stresses need") and ``whole``
    word the two refusals."""

    def __init__(self, sim, needs, whole="grid"):
        N = getattr(sim, "N", None)
        if N not in (2, 3) or getattr(sim, "P", None) != 1:
            raise RuntimeError("%s a degree-1 simulator (TensorProductSimulator1_1 or 1_1_1)" % needs)
        if sim._num_stored_elements() != sim.numElements():
            raise RuntimeError("%s a whole %s: this simulator stores slab padding layers" % (needs, whole))
        self.sim, self.N = sim, N
        self.ne = [int(n) for n in sim.NbElementsPerDimension()]
        self.nelem, self.nnode = sim.numElements(), sim.numNodes()
        self.h = np.ascontiguousarray((sim._bbmax - sim._bbmin) / np.asarray(self.ne, dtype=np.float64))
        self._nelems = np.asarray(self.ne, dtype=np.int64)
        self._mask = None

    def head(self, *extras):
        """``dim, nelems`` and what the family's calls take after them"""
        return (self.N, self._nelems.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) + extras

    @property
    def fixed(self):
        """does the simulator fix any component"""
        return bool(self.sim._mask.any())

    @property
    def mask(self):
        """one byte per node on the device, bit c set where component c is fixed; built at the first use"""
        if self._mask is None:
            bits = np.zeros(self.nnode, dtype=np.uint8)
            for c in range(self.N):
                bits |= self.sim._mask[:, c].astype(np.uint8) << c
            self._mask = torch.from_numpy(bits).to(_dev())
        return self._mask


def simp_multipliers(sim, rho, exponent=None, floor=None):
    """(m, dm/drho) of the densities ``rho`` on the device: m = floor + rho^exponent (E_0 - floor).  The defaults are the stiffness
    law of the simulator: its gamma and E_min."""
    q = float(sim.gamma if exponent is None else exponent)
    lo = float(sim.E_min if floor is None else floor)
    span = float(sim.E_0) - lo
    return (lo + rho ** q * span).contiguous(), (q * rho ** (q - 1.0) * span).contiguous()


class ObjectiveFunction(torch.autograd.Function):
    """An objective (``updateCache``, ``evaluate``, ``gradient_device``) as an autograd node of the densities: forward sets them and
    solves, backward is ``gradient_device()`` weighted by the incoming gradient, in the densities' dtype and shape.  A subclass
    says ``NAME`` (the public function, for the message) and, where it is not ``objective._u``, ``field``: the solved field, a new
    tensor with every solve, by which backward tells that the objective was updated in between."""

    NAME = None

    @staticmethod
    def field(objective):
        return objective._u

    @classmethod
    def update(cls, ctx, densities, objective):
        objective.updateCache(densities.detach().reshape(-1))
        ctx.objective, ctx.u, ctx.dtype, ctx.shape = objective, cls.field(objective), densities.dtype, densities.shape

    @classmethod
    def refuse_stale(cls, ctx):
        if cls.field(ctx.objective) is not ctx.u:
            raise RuntimeError("%s: the objective was updated between forward and backward" % cls.NAME)

    @classmethod
    def forward(cls, ctx, densities, objective):
        cls.update(ctx, densities, objective)
        return torch.tensor(objective.evaluate(), dtype=torch.float64, device=densities.device)

    @classmethod
    def backward(cls, ctx, grad_output):
        cls.refuse_stale(ctx)
        w = float(grad_output.detach().cpu())
        g = ctx.objective.gradient_device()
        if w != 1.0:
            g = w * g
        return g.to(ctx.dtype).reshape(ctx.shape), None
