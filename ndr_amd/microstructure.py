"""Design of periodic cells: the homogenised tensor as an objective of the package's design loop and as an autograd node (what the
gradient of ``TPPeriodicHomogenization.hh`` exists for in the reference: ``gradientDescent`` there, ``knitro_optimization.hh``).

    sim = pyVoxelFEM.TensorProductSimulator([1, 1], [[0, 0], [1, 1]], [64, 64]); sim.E_min, sim.gamma = 1e-3, 3.0
    objective = HomogenizedTensorObjective(sim, [[1, 1, 0], [1, 1, 0], [0, 0, 0]], skipSolve=True)     # maximise the bulk modulus
    smooth = PeriodicSmoothingFilter(); smooth.radius = 2
    problem = pyVoxelFEM.TopologyOptimizationProblem(sim, objective, [pyVoxelFEM.TotalVolumeConstraint(0.5)], [smooth])
    problem.setVars(x0); oc = pyVoxelFEM.OCOptimizer(problem); oc.step()
    Eh = objective.tensor()

``HomogenizedTensorObjective`` is  J = - sum_qr C[q, r] Eh[q, r]  for a positive semidefinite weight matrix; any other function of
the tensor (the reference's distance to a target tensor) goes through ``homogenizedTensor``, whose backward is the same contracted
gradient with the incoming gradient as the matrix.  Neither forms the [numElements, S, S] array of
``homogenizedElasticityTensorGradient``.  Strain cases follow ``ndr_amd.materials``: xx yy xy / xx yy zz yz xz xy.
"""
import numpy as np
import torch

from . import _lib
from . import homogenization as _hom
from .pyVoxelFEM import _Filter, _ptr, _stream, _to_np

__all__ = ["PeriodicSmoothingFilter", "HomogenizedTensorObjective", "HomogenizedTensorFunction", "homogenizedTensor"]


class PeriodicSmoothingFilter(_Filter):
    """Box filter on a periodic cell (``vfem_box_filter_periodic``): the mean over the (2 radius + 1)^N elements around each one,
    wrapped at the cell's faces, every offset counted once.  Unlike ``SmoothingFilter``, which clips its neighbourhoods at the grid
    boundary, it is translation invariant, has no seams and preserves the mean, so the filtered design has the design's volume.  It
    is symmetric: backprop is the same launch as apply."""

    def __init__(self):
        super().__init__()
        self._radius = 1

    def _get_radius(self):
        return self._radius

    def _set_radius(self, r):
        if int(r) < 0:
            raise RuntimeError("negative filter radius")
        self._radius = int(r)

    radius = property(_get_radius, _set_radius)

    def _run(self, x):
        self._check()
        if x.numel() != int(np.prod(self._grid)):
            raise RuntimeError("PeriodicSmoothingFilter: input of size %d does not match the grid (%d elements)"
                               % (x.numel(), int(np.prod(self._grid))))
        x = x.contiguous()
        out = torch.empty_like(x)
        _lib.check(_lib.load().vfem_box_filter_periodic(self._n3(), self._radius, _ptr(x), _ptr(out), _stream()))
        return out

    def apply_dev(self, x):
        return self._run(x)

    def backprop_dev(self, g, x):
        return self._run(g)


def _symmetric_weights(weights, S):
    C = np.array(weights, dtype=np.float64)
    if C.shape != (S, S):
        raise ValueError("weights must be a %d x %d matrix in the strain-case order of ndr_amd.materials (got shape %s)"
                         % (S, S, C.shape))
    if not np.all(np.isfinite(C)):
        raise ValueError("weights must be finite")
    Cs = 0.5 * (C + C.T)
    low = float(np.linalg.eigvalsh(Cs)[0])
    if low < -1e-12 * max(float(np.abs(Cs).max()), 1e-300):
        raise ValueError("the symmetric part of weights must be positive semidefinite (smallest eigenvalue %.3e): every element's "
                         "block of the tensor's gradient is positive semidefinite, so such weights give dJ/drho <= 0, which the "
                         "optimality-criteria step needs (it takes sqrt(dJ / (dc lambda))); sign-indefinite functions of the "
                         "tensor go through microstructure.homogenizedTensor" % low)
    return Cs


class HomogenizedTensorObjective:
    """J(rho) = - sum_qr Cs[q, r] Eh[q, r], Cs the symmetric part of ``weights`` (S x S, positive semidefinite; ValueError
    otherwise), Eh the homogenised tensor of the simulator's cell: an objective of ``TopologyOptimizationProblem``.  ``updateCache``
    solves the S cell problems (``homogenization.solveCellProblems`` with ``tol``, ``maxIter``, ``preconditioner``, ``levels``,
    ``smoothing``; the iteration counts stay in ``homogenization.last_iterations``); the gradient is the contracted kernel's."""

    def __init__(self, sim, weights, tol=1e-8, maxIter=20000, preconditioner="jacobi", levels=None, smoothing=1, skipSolve=False):
        self._sim = sim
        self.tol, self.maxIter, self.preconditioner, self.levels, self.smoothing = tol, maxIter, preconditioner, levels, smoothing
        N = getattr(sim, "N", None)
        if N not in (2, 3):
            raise RuntimeError("periodic homogenisation needs a degree-1 simulator (TensorProductSimulator1_1 or 1_1_1)")
        self._Cs = _symmetric_weights(weights, 3 if N == 2 else 6)
        self._cell = self._Wp = self._Eh = None
        if not skipSolve:
            self.updateCache(None)

    weights = property(lambda self: self._Cs.copy())

    def updateCache(self, xPhys):
        if xPhys is not None:
            self._sim.setElementDensities(xPhys)
        self._cell = self._Wp = self._Eh = None
        c = _hom._Cell(self._sim)
        Wp = _hom._solve(c, float(self.tol), int(self.maxIter), self.preconditioner, self.levels, int(self.smoothing))
        self._cell, self._Wp, self._Eh = c, Wp, _hom._tensor_of(c, Wp)

    def _need(self):
        if self._Wp is None:
            raise RuntimeError("HomogenizedTensorObjective: no solved cell (call updateCache first)")

    def evaluate(self, xPhys=None):
        if xPhys is not None:
            self.updateCache(xPhys)
        self._need()
        return -float(np.sum(self._Cs * self._Eh))

    def gradient_device(self):
        self._need()
        return -_hom._contracted(self._cell, self._Wp, self._Cs)

    def gradient(self):
        return _to_np(self.gradient_device())

    def tensor(self):
        self._need()
        return _hom._tensor_from(self._Eh, self._cell.N)

    def w_device(self):
        """the S fluctuation fields, one device tensor [S, numNodes, N]"""
        self._need()
        return self._cell.to_full(self._Wp)


class HomogenizedTensorFunction(torch.autograd.Function):
    """The homogenised tensor of the predicted densities as an autograd node, the periodic counterpart of ``fem.VoxelFEMFunction``:
    forward sets the simulator's densities, solves the cell problems and keeps the fields; backward is the gradient contracted with
    the incoming [S, S] gradient."""

    @staticmethod
    def forward(ctx, densities, sim, tol, preconditioner, levels, smoothing):
        sim.setElementDensities(densities.detach().reshape(-1))
        c = _hom._Cell(sim)
        Wp = _hom._solve(c, float(tol), 20000, preconditioner, levels, int(smoothing))
        ctx.cell, ctx.Wp, ctx.dtype, ctx.shape = c, Wp, densities.dtype, densities.shape
        return torch.from_numpy(_hom._tensor_of(c, Wp)).to(densities.device)

    @staticmethod
    def backward(ctx, grad_output):
        g = _hom._contracted(ctx.cell, ctx.Wp, grad_output)
        return g.to(ctx.dtype).reshape(ctx.shape), None, None, None, None, None


def homogenizedTensor(densities, sim, tol=1e-10, preconditioner="jacobi", levels=None, smoothing=1):
    """Eh [S, S] (float64, on the densities' device) of the cell of ``sim`` with the element densities ``densities`` (a device tensor
    of numElements values, float32 or float64), differentiable with respect to them: any torch loss on the tensor, such as the
    reference's ``((Eh - T) ** 2).sum() / (T ** 2).sum()``, can drive a torch optimiser or the package's MLP density field.  The
    simulator is left holding these densities."""
    return HomogenizedTensorFunction.apply(densities, sim, tol, preconditioner, levels, smoothing)
