"""Periodic homogenisation of a voxel cell (``VoxelFEM/TPPeriodicHomogenization.hh`` and ``TensorProjection.hh`` of the reference).

    w  = solveCellProblems(sim)                       # S fluctuation fields, S = 3 (2-D) or 6 (3-D)
    Eh = homogenizedElasticityTensor(w, sim)          # an ElasticityTensor: the base material of a macro-scale run
    dE = homogenizedElasticityTensorGradient(w, sim)  # [numElements, S, S]: d Eh / d rho_e
    g  = homogenizedElasticityTensorGradientContracted(w, sim, C)   # [numElements]: d (C : Eh) / d rho_e, the blocks never formed

for a degree-1 simulator in 2-D or 3-D holding any material.  The numerics run in ``libvfem.so`` (``vfem_hom_*``, include/vfem.h)
on the PERIODIC node grid: node (i_0, ..) of the simulator's grid is the unknown (i_d mod ne_d), node 0 is pinned.  The simulator
is only read: its Dirichlet conditions and loads play no part and stay as they are.

The element modulus  E_e = E_min + rho_e^gamma (E_0 - E_min)  scales the stiffness, the load and the tensor alike.  (The
reference scales load and tensor by the raw density and the stiffness by the SIMP modulus, which agrees with this only for
gamma = 1, E_0 = 1, E_min = 0.)  Strain cases follow ``ndr_amd.materials``: xx yy xy / xx yy zz yz xz xy; the unit strain of a
shear case has 0.5 on both off-diagonal entries.  DESIGN "Periodic homogenisation" has the formulas.

Fields cross this boundary on the simulator's FULL node grid with the duplicate faces filled, like every other nodal field of the
package: numpy arrays ``[numNodes, N]`` per strain case, or one torch tensor ``[S, numNodes, N]`` for the ``*_device`` variants.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import materials as _materials
from ._grid import Grid, _dp, simp_multipliers
from .pyVoxelFEM import _dev, _ptr, _stream, _stress_load, _to_np

__all__ = ["solveCellProblems", "solveCellProblems_device", "homogenizedElasticityTensor", "homogenizedElasticityTensor_device",
           "homogenizedElasticityTensorGradient", "homogenizedElasticityTensorGradient_device",
           "homogenizedElasticityTensorGradientContracted", "homogenizedElasticityTensorGradientContracted_device", "closestIsotropicTensor",
           "last_iterations", "last_relative_residuals", "last_levels"]

last_iterations = []             # PCG iterations of each strain case in the last solveCellProblems
last_relative_residuals = []     # |r| / |b| of each strain case at its end
last_levels = []                 # per-level cell sizes of the last multigrid solve: [[n_0, ..], [n_0 / 2, ..], ..]


class _Cell(Grid):
    """what every ``vfem_hom_*`` call starts with, taken from a simulator: the grid, K0, L, D, the voxel volume, the moduli"""

    def __init__(self, sim):
        super().__init__(sim, "periodic homogenisation needs", whole="cell")
        N, ne, h = self.N, self.ne, self.h
        if min(ne) < 2:
            raise RuntimeError("periodic homogenisation needs at least 2 elements along every axis (got %s)" % "x".join(map(str, ne)))
        self.S = 3 if N == 2 else 6
        self.pn = int(np.prod(ne))
        self.vol = float(np.prod(h))
        self.cell_volume = self.vol * self.pn
        tensor = sim.ETensor
        self.D = np.ascontiguousarray(tensor.D)
        self.K0 = np.ascontiguousarray(sim.fullDensityElementStiffnessMatrix())
        # L[:, q]: element load of the constant stress C : e_q, e_q = SymmetricMatrix::CanonicalBasis(q)
        one = torch.ones((1,) * N, dtype=torch.float64)
        L = np.empty((self.K0.shape[0], self.S))
        for q, (i, j) in enumerate(_materials._PAIRS[N]):
            eps = np.zeros((N, N))
            eps[i, j] = eps[j, i] = 1.0 if i == j else 0.5
            L[:, q] = _stress_load(tensor.doubleContract(eps), h, 1, one).numpy().reshape(-1)
        self.L = np.ascontiguousarray(L)
        self.E, self.dE = simp_multipliers(sim, sim.getDensities_device()[:self.pn])

    def head(self):
        return super().head(_dp(self.K0), _dp(self.L), _dp(self.D), self.vol, _ptr(self.E))

    # ---- full node grid <-> periodic node grid ----
    def to_full(self, Wp):
        """[S, periodic nodes, N] -> [S, numNodes, N]: the duplicate faces filled"""
        W = Wp.reshape([Wp.shape[0]] + self.ne + [self.N])
        for d, n in enumerate(self.ne):
            W = W.index_select(d + 1, torch.arange(n + 1, device=W.device) % n)
        return W.reshape(Wp.shape[0], -1, self.N).contiguous()

    def to_periodic(self, W):
        """[S, numNodes, N] -> [S, periodic nodes, N]: the first copy of every periodic node"""
        if not isinstance(W, torch.Tensor):
            W = torch.from_numpy(np.ascontiguousarray(np.asarray(W, dtype=np.float64)))
        W = W.to(device=_dev(), dtype=torch.float64)
        nn = int(np.prod([n + 1 for n in self.ne]))
        if W.numel() != self.S * nn * self.N:
            raise RuntimeError("Invalid input size: expected %d fields of %d x %d values" % (self.S, nn, self.N))
        W = W.reshape([self.S] + [n + 1 for n in self.ne] + [self.N])
        for d, n in enumerate(self.ne):
            W = W.narrow(d + 1, 0, n)
        return W.reshape(self.S, self.pn, self.N).contiguous()


class _Hierarchy:
    """the multigrid hierarchy of one cell (``vfem_hom_mg_*``): level 0 is the cell, level l + 1 has half the periodic nodes per axis
    and is made while every extent is even and at least 4 (``levels``: at most that many coarsenings), the last level is solved
    exactly.  Vectors of level l are device tensors [S, nodes_l, N] on the periodic grid."""

    def __init__(self, cell, levels=None):
        self.cell = cell                                         # (keeps the moduli the handle reads alive)
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        cap = -1 if levels is None else int(levels)
        if levels is not None and cap < 0:
            raise ValueError("levels must be None or a non-negative number of coarsenings")
        _lib.check(self._lib.vfem_hom_mg_create(ctypes.byref(self._h), *cell.head(), cap, _stream()))
        n = (ctypes.c_int64 * cell.N)()
        self.dims = []
        for l in range(self._lib.vfem_hom_mg_num_levels(self._h)):
            _lib.check(self._lib.vfem_hom_mg_level_dims(self._h, l, n))
            self.dims.append(list(n))
        self.bytes = int(self._lib.vfem_hom_mg_bytes(self._h))

    def close(self):
        if self._h:
            self._lib.vfem_hom_mg_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        self.close()

    def _like(self, l):
        return torch.empty((self.cell.S, int(np.prod(self.dims[l])), self.cell.N), dtype=torch.float64, device=_dev())

    def level_apply(self, l, W):
        out = self._like(l)
        _lib.check(self._lib.vfem_hom_mg_level_apply(self._h, l, _ptr(W), _ptr(out), _stream()))
        return out

    def smooth(self, l, X, B, forward=True):
        """one colour sweep on X in place"""
        _lib.check(self._lib.vfem_hom_mg_smooth(self._h, l, _ptr(X), _ptr(B), int(bool(forward)), _stream()))
        return X

    def restrict(self, l, fine):
        out = self._like(l + 1)
        _lib.check(self._lib.vfem_hom_mg_restrict(self._h, l, _ptr(fine), _ptr(out), _stream()))
        return out

    def prolong_add(self, l, coarse, fine):
        _lib.check(self._lib.vfem_hom_mg_prolong_add(self._h, l, _ptr(coarse), _ptr(fine), _stream()))
        return fine

    def vcycle(self, B, smoothing=1):
        out = self._like(0)
        _lib.check(self._lib.vfem_hom_mg_vcycle(self._h, _ptr(B), _ptr(out), int(smoothing), _stream()))
        return out

    def solve(self, Wp, tol, maxIter, smoothing, its, res):
        """the status of ``vfem_hom_mg_solve_cells``; ``its`` and ``res`` are the caller's ctypes arrays of S counts and norms"""
        return self._lib.vfem_hom_mg_solve_cells(self._h, _ptr(Wp), float(tol), int(maxIter), int(smoothing), its, res, _stream())


def solveCellProblems_device(sim, tol=1e-10, maxIter=20000, preconditioner="jacobi", levels=None, smoothing=1):
    """the S fluctuation fields as one device tensor [S, numNodes, N]; see ``solveCellProblems``"""
    c = _Cell(sim)
    return c.to_full(_solve(c, tol, maxIter, preconditioner, levels, smoothing))


def _solve(c, tol, maxIter, preconditioner, levels, smoothing):
    """the fields of the cell ``c`` on the periodic grid, [S, periodic nodes, N]"""
    global last_iterations, last_relative_residuals, last_levels
    if preconditioner not in ("jacobi", "multigrid"):
        raise ValueError("preconditioner must be \"jacobi\" or \"multigrid\" (got %r)" % (preconditioner,))
    Wp = torch.empty((c.S, c.pn, c.N), dtype=torch.float64, device=_dev())
    its, res = (ctypes.c_int * c.S)(), (ctypes.c_double * c.S)()
    if preconditioner == "multigrid":
        h = _Hierarchy(c, levels)
        try:
            status = h.solve(Wp, tol, maxIter, smoothing, its, res)
            last_levels = [list(d) for d in h.dims]
        finally:
            h.close()
    else:
        status = _lib.load().vfem_hom_solve_cells(*c.head(), _ptr(Wp), float(tol), int(maxIter), its, res, _stream())
    last_iterations, last_relative_residuals = list(its), list(res)
    _lib.check(status)
    return Wp


def solveCellProblems(sim, tol=1e-10, maxIter=20000, preconditioner="jacobi", levels=None, smoothing=1):
    """TPPeriodicHomogenization::solveCellProblems: for every unit strain e_q the periodic fluctuation w_q with
    K_per w_q = - sum_e E_e L[:, q], w_q = 0 at node 0, by a batched PCG to ``|r| / |b| <= tol``.  Returns a list of S
    arrays [numNodes, N]; raises RuntimeError when a case has not converged after ``maxIter`` iterations.  A singular cell (a node
    whose incident elements all have zero modulus, or non-finite moduli) raises RuntimeError "breakdown in strain case q" as well.  The
    iteration counts and final residuals are left in ``last_iterations`` / ``last_relative_residuals``.  ``sim`` is not changed.

    ``preconditioner``: ``"jacobi"`` (node blocks; the iteration count grows with the cell's extent) or ``"multigrid"``: one V-cycle
    of a periodic geometric multigrid per iteration, with ``smoothing`` multicolour block Gauss-Seidel sweeps before and after the
    coarse correction.  The cell is halved per level while every extent is even and at least 4, at most ``levels`` times
    (None: as far as that goes); the last level is solved exactly, so its dofs must fit the dense coarsest-level solver
    (RuntimeError otherwise: a large cell needs extents with enough factors of 2).  ``last_levels`` then holds the level sizes."""
    return list(_to_np(solveCellProblems_device(sim, tol, maxIter, preconditioner, levels, smoothing)))


def _tensor_from(D, dim):
    t = _materials.ElasticityTensor(dim=dim)
    t._D, t._iso = np.array(D, dtype=np.float64), None           # as computed: ``fromD`` would refuse the unsymmetrised matrix
    return t


def _tensor_of(c, Wp, baseCellVolume=0.0):
    """the homogenised tensor of the periodic fields ``Wp`` of the cell ``c`` as a numpy array [S, S]"""
    Eh = np.empty((c.S, c.S))
    _lib.check(_lib.load().vfem_hom_tensor(*c.head(), _ptr(Wp), float(baseCellVolume) or c.cell_volume, _dp(Eh), _stream()))
    return Eh


def homogenizedElasticityTensor_device(w, sim, baseCellVolume=0.0):
    c = _Cell(sim)
    return _tensor_from(_tensor_of(c, c.to_periodic(w), baseCellVolume), c.N)


def homogenizedElasticityTensor(w, sim, baseCellVolume=0.0):
    """TPPeriodicHomogenization::homogenizedElasticityTensor (stress-like):
    Eh[q, r] = 1/|Y| sum_e E_e (w_{q,e} . L[:, r] + vol D[q, r]), |Y| = ``baseCellVolume`` or the bounding box's volume.
    The result is as computed, not symmetrised (its asymmetry is the solver's residual)."""
    return homogenizedElasticityTensor_device(np.stack([np.asarray(a, dtype=np.float64) for a in w]), sim, baseCellVolume)


def _gradient(w, sim, scaled):
    c = _Cell(sim)
    return _gradient_periodic(c, c.to_periodic(w), scaled)


def _gradient_periodic(c, Wp, scaled):
    G = torch.empty((c.pn, c.S, c.S), dtype=torch.float64, device=_dev())
    _lib.check(_lib.load().vfem_hom_tensor_gradient(*c.head(), _ptr(Wp), c.cell_volume, _ptr(c.dE) if scaled else None, _ptr(G),
                                                    _stream()))
    return G


def homogenizedElasticityTensorGradient_device(w, sim):
    return _gradient(w, sim, True)


def homogenizedElasticityTensorGradient(w, sim):
    """TPPeriodicHomogenization::homogenizedElasticityTensorGradient: [numElements, S, S], the derivative of the homogenised tensor
    with respect to every density, dE_e/drho_e / |Y| (w_q^T K0 w_r + w_q . L[:, r] + L[:, q] . w_r + vol D[q, r]) on element e"""
    return _to_np(_gradient(np.stack([np.asarray(a, dtype=np.float64) for a in w]), sim, True))


def _contracted(c, Wp, C):
    """sum_qr C[q, r] dEh[q, r] / d rho_e for the periodic fields ``Wp`` of the cell ``c``: a device tensor [numElements]"""
    C = np.ascontiguousarray(C.detach().cpu().numpy() if isinstance(C, torch.Tensor) else C, dtype=np.float64)
    if C.shape != (c.S, c.S):
        raise ValueError("the contracting matrix must be %d x %d (got %s)" % (c.S, c.S, "x".join(map(str, C.shape))))
    g = torch.empty(c.pn, dtype=torch.float64, device=_dev())
    _lib.check(_lib.load().vfem_hom_tensor_gradient_contract(*c.head(), _ptr(Wp), c.cell_volume, _ptr(c.dE), _dp(C), _ptr(g),
                                                             _stream()))
    return g


def homogenizedElasticityTensorGradientContracted_device(w, sim, C):
    c = _Cell(sim)
    return _contracted(c, c.to_periodic(w), C)


def homogenizedElasticityTensorGradientContracted(w, sim, C):
    """``einsum("qr,eqr->e", C, homogenizedElasticityTensorGradient(w, sim))`` without the [numElements, S, S] array: the derivative
    of  sum_qr C[q, r] Eh[q, r]  with respect to every density (the vector-Jacobian product of the homogenised tensor).  Only the
    symmetric part of ``C`` acts, since every element's block is symmetric."""
    return _to_np(homogenizedElasticityTensorGradientContracted_device(np.stack([np.asarray(a, dtype=np.float64) for a in w]), sim, C))


def closestIsotropicTensor(C):
    """TensorProjection.hh:22-76: the isotropic tensor closest to ``C`` in the Frobenius norm of the rank-4 tensors.  With the
    hydrostatic and deviatoric extractors J, K (orthogonal, <J, J> = 1, <K, K> = n (n + 1) / 2 - 1):
    n lambda + 2 mu = <C, J> = C_iijj / n and 2 mu = <C, K> / <K, K> = (C_ijij - C_iijj / n) / <K, K>."""
    if not isinstance(C, _materials.ElasticityTensor):
        raise TypeError("closestIsotropicTensor takes an ndr_amd.ElasticityTensor")
    n = C.dim
    full = C.fullTensor()
    c_ijij, c_iijj = float(np.einsum("ijij->", full)), float(np.einsum("iijj->", full))
    alpha = c_iijj / n
    beta = (c_ijij - alpha) / (0.5 * (n * n + n) - 1.0)
    out = _materials.ElasticityTensor(dim=n)
    out._set_lame((alpha - beta) / n, beta / 2.0)
    out._iso = None
    return out
