"""Host-side mirror of the reference's ``pyVoxelFEM`` pybind11 module for the MI355X path.

Same names, argument meaning and error behaviour as
``VoxelFEM/python_bindings/VoxelFEM.cc:41-289`` of the reference; arrays cross this boundary as
float64 numpy arrays (copied, like the Eigen conversions of the reference), the numerics run in
``libvfem.so`` (HIP kernels, include/vfem.h) on device memory held in torch tensors.
``*_device`` methods take/return torch CUDA tensors without copies.

One simulator class (``_Simulator``) and one multigrid class (``_MultigridSolver``) bind every element type: they are
parameterised by ``N``, ``P`` and the prefix of the C entry points, resolved by ``_c(name)`` / ``_mg(name)``.  The tuned
<1,1,1> path (``vfem_sim_`` / ``vfem_mg_``) and the generic path (``vfem_gsim_`` / ``vfem_gmg_``: 2-D and degree 2) are
subclasses that hold only what differs between the two C layers.

Host-side pieces (BC/material parsing, filters, volume constraint, optimality-criterion update,
problem cache) restate ``TopologyOptimization{Problem,Filter,Constraint}.hh`` and
``OptimalityCriterion.hh``; SURVEY 8(f)-1 ranks moving them to the device as the next step.
"""
import ctypes
import json
import os
import sys
import types

import numpy as np
import torch

from . import _lib
from . import band as _band
from . import materials as _materials

__all__ = [
    "TensorProductSimulator", "TopologyOptimizationProblem", "ComplianceObjective",
    "MultigridComplianceObjective", "OCOptimizer", "PythonFilter", "ProjectionFilter",
    "SmoothingFilter", "LangelaarFilter", "applyFilter", "TotalVolumeConstraint",
    "benchmark_reset", "benchmark_report", "benchmark_start_timer_section",
    "benchmark_stop_timer_section", "benchmark_start_timer", "benchmark_stop_timer", "detail", "ElasticityTensor",
]

ElasticityTensor = _materials.ElasticityTensor       # what sim.ETensor returns and takes (MeshFEM binds it in its own `tensors` module)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _to_dev(a, shape=None):
    """float64 contiguous device tensor from numpy / torch / sequence."""
    if isinstance(a, torch.Tensor):
        t = a.to(device=_dev(), dtype=torch.float64).contiguous()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).to(_dev())
    if shape is not None:
        if t.numel() != int(np.prod(shape)):
            raise RuntimeError("Invalid input size")
        t = t.reshape(shape)
    return t


def _to_np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------
# material / boundary-condition files (MeshFEM Materials.cc, BoundaryConditions.cc:255-370)
# ----------------------------------------------------------------------------------------------

def _read_isotropic_material(path):
    """(young, poisson) of an isotropic material file: what the isotropic oracles of the tests are built from; the simulators read
    materials of every type through ``materials.read_material``"""
    with open(path) as fh:
        m = json.load(fh)
    if m.get("type", "isotropic_material") != "isotropic_material":
        raise RuntimeError("unsupported material type: " + str(m.get("type")))
    return float(m["young"]), float(m["poisson"])


def _parse_regions(path):
    with open(path) as fh:
        cfg = json.load(fh)
    regions = []
    for reg in cfg["regions"]:
        t = reg["type"]
        comps = "xyz"
        if t.startswith("dirichlet"):
            tail = t[len("dirichlet"):]
            n = 0
            while n < len(tail) and "x" <= tail[n] <= "z":
                n += 1
            if n > 3:
                raise RuntimeError("invalid mask")
            if n > 0:
                comps = tail[:n]
                if len(set(comps)) != len(comps):
                    raise RuntimeError("invalid component specifier: '%s'" % comps)
            if tail[n:] != "":
                raise RuntimeError('Illegal constraint type, only "dirichlet" and "force" accepted')
            kind = "dirichlet"
        elif t == "force":
            kind = "force"
        else:
            raise RuntimeError('Illegal constraint type, only "dirichlet" and "force" accepted')
        if "box%" in reg:
            relative, box = True, reg["box%"]
        elif "box" in reg:
            relative, box = False, reg["box"]
        else:
            raise RuntimeError("only box / box% regions are supported")
        regions.append((kind, comps, [float(v) for v in reg["value"]],
                        [float(v) for v in box["minCorner"]], [float(v) for v in box["maxCorner"]], relative))
    return regions


class SuiteSparseMatrix:
    """What ``TensorProductSimulator.getK()`` returns (TPS.hh:966-973): the assembled stiffness matrix in compressed-column
    form, upper triangle only (TPS.hh:590-612 accumulates ``di <= dj``), with the attribute names of MeshFEM's binding
    (python_bindings/sparse_matrices.cc:67-125): m, n, nz, Ap, Ai, Ax, symmetry_mode, trace(), apply(), toSciPy().
    Host-side and assembled with numpy: a diagnostic of small problems, not part of the device path."""

    def __init__(self, upper_csc):
        self._A = upper_csc
        self.m, self.n = upper_csc.shape
        self.nz = int(upper_csc.nnz)
        self.Ap = upper_csc.indptr.astype(np.int64)
        self.Ai = upper_csc.indices.astype(np.int64)
        self.Ax = upper_csc.data
        self.symmetry_mode = "UPPER_TRIANGLE"

    def trace(self):
        return float(self._A.diagonal().sum())

    def toSciPy(self):
        return self._A.copy()

    def full(self):
        """the symmetric matrix the upper triangle stands for"""
        import scipy.sparse as sp
        return (self._A + sp.triu(self._A, 1).T).tocsc()

    def apply(self, vec, transpose=False):
        return self.full() @ np.asarray(vec, dtype=np.float64).reshape(-1)


def _assemble_upper(elem_nodes, K0, young, ndof_per_node, num_nodes):
    """sum_e E_e G_e^T K0 G_e, entries with row <= column (TPS.hh:590-625)"""
    import scipy.sparse as sp
    nd = ndof_per_node
    dofs = (elem_nodes[:, :, None] * nd + np.arange(nd)[None, None, :]).reshape(elem_nodes.shape[0], -1)
    ke = K0.shape[0]
    n = num_nodes * nd
    A = sp.csc_matrix((n, n))
    step = max(1, (1 << 22) // (ke * ke))                  # bounded temporary: ~4 M triplets at a time
    for a in range(0, dofs.shape[0], step):
        d = dofs[a:a + step]
        rows = np.repeat(d, ke, axis=1).reshape(-1)
        cols = np.tile(d, (1, ke)).reshape(-1)
        vals = (young[a:a + step, None] * K0.reshape(1, -1)).reshape(-1)
        keep = rows <= cols
        A = A + sp.coo_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n)).tocsc()
    A.sum_duplicates()
    A.sort_indices()
    return SuiteSparseMatrix(A)


def _constant_strain_load(eps, lam, mu, h, degree, rho_grid):
    """TPS::constantStrainLoad (TPS.hh:792-821 with Element::constantStrainLoad, :145-173): nodal load of the unit strain
    ``eps`` (N x N symmetric): every element contributes  rho_e * vol * (C : eps) . int grad(phi_j)  to its node j -- the
    RAW density scales the load (no SIMP law, TPS.hh:813).  int grad(phi_j) factorises over the axes of the tensor-product
    Lagrange basis: int phi' = phi(1) - phi(0), int phi = the Newton-Cotes weights."""
    N = len(h)
    eps = np.asarray(eps, dtype=np.float64).reshape(N, N)
    sigma = lam * np.trace(eps) * np.eye(N) + 2.0 * mu * 0.5 * (eps + eps.T)            # isotropic C : eps
    return _stress_load(sigma, h, degree, rho_grid)


def _stress_load(sigma, h, degree, rho_grid):
    """the nodal load of the constant stress ``sigma`` = C : eps (any tensor C), see ``_constant_strain_load``"""
    N = len(h)
    I = {1: np.array([0.5, 0.5]), 2: np.array([1.0, 4.0, 1.0]) / 6.0}[degree]
    dI = {1: np.array([-1.0, 1.0]), 2: np.array([-1.0, 0.0, 1.0])}[degree]
    vol = float(np.prod(h))
    ne = rho_grid.shape
    nn = tuple(n * degree + 1 for n in ne)
    F = torch.zeros(nn + (N,), dtype=torch.float64, device=rho_grid.device)
    for loc in np.ndindex(*([degree + 1] * N)):
        g = np.array([dI[loc[k]] / h[k] * np.prod([I[loc[m]] for m in range(N) if m != k]) for k in range(N)])
        load = torch.as_tensor(vol * (sigma @ g), dtype=torch.float64, device=rho_grid.device)
        sl = tuple(slice(loc[d], loc[d] + degree * ne[d], degree) for d in range(N))
        F[sl] += rho_grid[..., None] * load
    return F.reshape(-1, N)


def _densities_from_msh(path, field, ne, N):
    """TPS::readDensities (TPS.hh:470-509): per-element scalar field of a Gmsh file; an element's grid cell is found from
    its vertex centroid relative to the bounding box of the mesh vertices"""
    if not str(path).endswith(".msh"):
        raise RuntimeError("Material file extension" + os.path.splitext(str(path))[1] + " is not supported")
    from . import io
    parser = io.MSHFieldParser3(path)
    values = np.asarray(parser.scalarField(field), dtype=np.float64).reshape(-1)
    V, E = np.asarray(parser.vertices(), dtype=np.float64), np.asarray(parser.elements())
    nel = int(np.prod(ne))
    if E.shape[0] != nel:
        raise RuntimeError("The number of elements in the mesh : %d and the number of elements of the simulator : %d must be equal."
                           % (E.shape[0], nel))
    lo, hi = V.min(axis=0), V.max(axis=0)
    rel = (V[E].mean(axis=1) - lo) / np.where(hi > lo, hi - lo, 1.0)
    cell = np.minimum(np.floor(rel[:, :N] * np.asarray(ne)).astype(np.int64), np.asarray(ne) - 1)
    rho = np.zeros(nel)
    rho[np.ravel_multi_index(tuple(cell.T), tuple(int(n) for n in ne))] = values
    return rho


def _factorize(mode, band_bytes):
    """``directSolver`` of the simulators: True = band Cholesky of K, False = the multigrid-preconditioned CG stand-in"""
    if mode == "auto":
        return band_bytes <= _band.BAND_CAP_BYTES
    if mode not in ("cholesky", "pcg"):
        raise RuntimeError("directSolver must be 'auto', 'cholesky' or 'pcg', not %r" % (mode,))
    return mode == "cholesky"


# ----------------------------------------------------------------------------------------------
# MultigridSolver<p,..,p>
# ----------------------------------------------------------------------------------------------

class _LevelView:
    """What ``MultigridSolver.getSimulator(l)`` exposes for coarse levels (sizes + Dirichlet mask)."""

    def __init__(self, mg, l):
        self._mg, self._l = mg, l

    def numNodes(self):
        return self._mg._nn(self._l)

    def NbElementsPerDimension(self):
        ne = (ctypes.c_int64 * 3)()
        _lib.check(self._mg._mg("level_dims")(self._mg._h, self._l, ne))
        return np.array(list(ne)[:self._mg.N], dtype=np.int64)

    def numElements(self):
        return int(np.prod(self.NbElementsPerDimension()))

    @property
    def dirichletMask(self):
        m = np.empty(self.numNodes(), dtype=np.uint8)
        _lib.check(self._mg._mg("level_dirichlet_mask")(self._mg._h, self._l, m.ctypes.data_as(ctypes.c_void_p)))
        return np.stack([(m >> c) & 1 for c in range(self._mg.N)], axis=1).astype(bool)


class _MultigridSolver:
    """MultigridSolver<p,..,p> (VoxelFEM.cc:94-131; MG.hh:11-759) over the hierarchy handles of ``libvfem``.  The two
    subclasses name the C entry points (``_MG_PREFIX``) and hold what only one of the paths has."""

    _MG_PREFIX = None              # "vfem_mg_" (tuned <1,1,1>) or "vfem_gmg_" (generic path)

    def __init__(self, tps, numCoarseningLevels):
        self._lib = _lib.load()
        self._tps = tps                      # keeps the fine simulator alive (MG.hh:32,88)
        self.N = tps.N
        h = ctypes.c_void_p()
        _lib.check(self._mg("create")(ctypes.byref(h), tps._h, int(numCoarseningLevels)))
        self._h = h
        self.L = int(numCoarseningLevels)
        self.buildBlockStiffnessMatrices = True
        self.buildFinestBlockStiffnessMatrix = False
        self.last_iterations = 0
        self.last_relative_residual = 0.0

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._mg("destroy")(h)
            except Exception:
                pass
            self._h = None

    def _mg(self, name):
        return getattr(self._lib, self._MG_PREFIX + name)

    def _nn(self, l):
        n = int(self._mg("level_num_nodes")(self._h, int(l)))
        if n < 0:
            raise IndexError("vector::_M_range_check")      # m_sims.at(l)
        return n

    def getSimulator(self, l):
        self._nn(l)
        return self._tps if int(l) == 0 else _LevelView(self, int(l))

    def setSymmetricGaussSeidel(self, symmetric):
        self._mg("set_symmetric_gauss_seidel")(self._h, int(bool(symmetric)))

    def updateElementStiffnessMatrices(self):
        _lib.check(self._mg("update_operators")(self._h, _stream()))

    updateBlockKs = updateElementStiffnessMatrices

    # ---- per-operator entry points (device variants first) ----
    def applyK_device(self, l, u):
        u = _to_dev(u, (self._nn(l), self.N))
        out = torch.empty_like(u)
        _lib.check(self._mg("apply_k")(self._h, int(l), _ptr(u), _ptr(out), _stream()))
        return out

    def applyK(self, l, u):
        return _to_np(self.applyK_device(l, u))

    def computeResidual_device(self, l, u, b):
        u = _to_dev(u, (self._nn(l), self.N))
        b = _to_dev(b, (self._nn(l), self.N))
        r = torch.empty_like(u)
        _lib.check(self._mg("residual")(self._h, int(l), _ptr(u), _ptr(b), _ptr(r), _stream()))
        return r

    def computeResidual(self, l, u, b):
        return _to_np(self.computeResidual_device(l, u, b))

    def smoothing_device(self, l, u, b, forward=True):
        u = _to_dev(u, (self._nn(l), self.N)).clone()
        b = _to_dev(b, (self._nn(l), self.N))
        _lib.check(self._mg("smooth")(self._h, int(l), _ptr(u), _ptr(b), int(bool(forward)), _stream()))
        return u

    def smoothing(self, l, u, b):
        """Bound as updateElementStiffnessMatrices + one forward sweep on a copy (VoxelFEM.cc:99-104).  The
        reference binding runs the sequential sweep (MG.hh:269-282); the solver itself uses the multicoloured
        sweep (MG.hh:336-340), which is what this returns."""
        self.updateElementStiffnessMatrices()
        return _to_np(self.smoothing_device(l, u, b, True))

    def zeroOutDirichletComponents(self, l, u):
        t = _to_dev(u, (self._nn(l), self.N)).clone()
        _lib.check(self._mg("zero_dirichlet")(self._h, int(l), _ptr(t), _stream()))
        return _to_np(t)

    def restriction_device(self, fine_level, values):
        v = _to_dev(values, (self._nn(fine_level), self.N))
        out = torch.empty((self._nn(fine_level + 1), self.N), dtype=torch.float64, device=_dev())
        _lib.check(self._mg("restrict")(self._h, int(fine_level), _ptr(v), _ptr(out), _stream()))
        return out

    def interpolation_device(self, fine_level, values, out=None):
        v = _to_dev(values, (self._nn(fine_level + 1), self.N))
        acc = out is not None
        if out is None:
            out = torch.empty((self._nn(fine_level), self.N), dtype=torch.float64, device=_dev())
        _lib.check(self._mg("interpolate")(self._h, int(fine_level), _ptr(v), _ptr(out), int(acc), _stream()))
        return out

    def debugMulticolorVisit(self):
        """Visit order of the multicoloured sweep on level 0 (MG.hh:285-334): one colour per local node index of the
        element; along an axis the nodes of an element boundary (local index 0 or p) recur every 2p nodes, interior ones
        every p."""
        nn, p, N = tuple(self._tps._nn), self._tps.P, self.N
        result = np.zeros(nn, dtype=np.int32)
        counter = 0
        for lni in np.ndindex(*([p + 1] * N)):
            sl = tuple(slice(lni[d], None, (2 if lni[d] in (0, p) else 1) * p) for d in range(N))
            sub = result[sl]
            sub[...] = counter + np.arange(sub.size).reshape(sub.shape)
            counter += sub.size
        return result.reshape(-1)

    # ---- solvers ----
    def solve_device(self, u, f, numSteps, numSmoothingSteps, stiffnessUpdated=False, zeroDirichlet=False,
                     it_callback=None, fullMultigrid=False):
        x = _to_dev(u, (self._nn(0), self.N)).clone()
        f = _to_dev(f, (self._nn(0), self.N))
        if it_callback is None:
            _lib.check(self._mg("solve")(self._h, _ptr(x), _ptr(f), int(numSteps), int(numSmoothingSteps),
                                         int(bool(stiffnessUpdated)), int(bool(zeroDirichlet)),
                                         int(bool(fullMultigrid)), _stream()))
            return x
        for i in range(int(numSteps)):
            _lib.check(self._mg("solve")(self._h, _ptr(x), _ptr(f), 1, int(numSmoothingSteps),
                                         int(bool(stiffnessUpdated) or i > 0), int(bool(zeroDirichlet)),
                                         int(bool(fullMultigrid) and i == 0), _stream()))
            it_callback(i, _to_np(x))
        return x

    def solve(self, u, f, numSteps, numSmoothingSteps, stiffnessUpdated=False, zeroDirichlet=False,
              it_callback=None, fullMultigrid=False):
        return _to_np(self.solve_device(u, f, numSteps, numSmoothingSteps, stiffnessUpdated, zeroDirichlet,
                                        it_callback, fullMultigrid))

    def _pcg_check_inputs(self, u, b):
        """what a path rejects before x and b are converted (nothing here)"""

    def _pcg_search_direction(self):
        """third argument of the PCG ``it_callback``: the generic path does not expose its search direction"""
        return None

    def preconditionedConjugateGradient_device(self, u, b, maxIter, tol, it_callback=None, mgIterations=1,
                                               mgSmoothingIterations=1, fullMultigrid=False, residual_cb=None):
        self._pcg_check_inputs(u, b)
        x = _to_dev(u).reshape(-1, self.N).clone()
        b = _to_dev(b).reshape(-1, self.N)
        if x.shape[0] != b.shape[0]:
            raise RuntimeError("x and b should have the same size")
        if x.shape[0] != self._nn(0):
            raise RuntimeError("size of input and number of nodes don't correspond")
        its = ctypes.c_int(0)
        rel = ctypes.c_double(0.0)

        def _cb(_user, it, rnorm):
            if residual_cb is not None:
                residual_cb(it, rnorm)
            if it_callback is not None:
                it_callback(it, _to_np(x), self._pcg_search_direction())

        cb = _lib.RESIDUAL_CB(_cb) if (residual_cb is not None or it_callback is not None) else _lib.RESIDUAL_CB()
        _lib.check(self._mg("pcg")(self._h, _ptr(x), _ptr(b), int(maxIter), float(tol), int(mgIterations),
                                   int(mgSmoothingIterations), int(bool(fullMultigrid)), cb, None,
                                   ctypes.byref(its), ctypes.byref(rel), _stream()))
        self.last_iterations = its.value
        self.last_relative_residual = rel.value
        return x

    def preconditionedConjugateGradient(self, u, b, maxIter, tol, it_callback=None, mgIterations=1,
                                        mgSmoothingIterations=1, fullMultigrid=False):
        return _to_np(self.preconditionedConjugateGradient_device(u, b, maxIter, tol, it_callback, mgIterations,
                                                                  mgSmoothingIterations, fullMultigrid))


class MultigridSolver1_1_1(_MultigridSolver):
    """``pyVoxelFEM.detail.MultigridSolver1_1_1``: the tuned hierarchy (``vfem_mg_*``), which also exposes its coarsest
    solve and its work vectors."""

    _MG_PREFIX = "vfem_mg_"
    _COARSEST_MODES = {"auto": 0, "dense": 1, "planes": 2}          # VFEM_COARSEST_* of include/vfem.h

    # coarsestSolver and coarsestBytes are attributes of the instances, like last_iterations: the public names of the class itself
    # are those of the reference's binding plus the three debug entries.
    #   mg.coarsestSolver = "auto" | "dense" | "planes"   how the coarsest level is solved: "dense" (n x n inverse, at most 40 000
    #       dofs), "planes" (block tridiagonal Cholesky over the x planes, any size that fits 8 GiB) or "auto" (the default: dense up
    #       to its limit, plane blocks above).  Assigning another mode discards the kept factorisation; an unknown one raises.
    #   mg.coarsestBytes()   device bytes of the coarsest-level factorisation currently kept (0 before the first operator update)
    def __setattr__(self, name, value):
        if name == "coarsestSolver":
            if value not in self._COARSEST_MODES:
                raise RuntimeError("coarsestSolver must be one of %s, not %r" % (sorted(self._COARSEST_MODES), value))
            _lib.check(self._mg("set_coarsest_solver")(self._h, self._COARSEST_MODES[value]))
        object.__setattr__(self, name, value)

    def __getattr__(self, name):          # (only reached for names that are neither set on the instance nor defined by the class)
        if name == "coarsestSolver":
            return "auto"
        if name == "coarsestBytes":
            return self._coarsest_bytes
        raise AttributeError(name)

    def _coarsest_bytes(self):
        return int(self._mg("coarsest_bytes")(self._h))

    def coarsestSolve_device(self, b):
        b = _to_dev(b, (self._nn(self.L), 3))
        x = torch.empty_like(b)
        _lib.check(self._mg("coarsest_solve")(self._h, _ptr(b), _ptr(x), _stream()))
        return x

    def _field(self, which, l):
        n = self._nn(l) if which != 2 else self._nn(0)
        p = self._mg("field_ptr")(self._h, which, int(l))
        out = torch.empty((n, 3), dtype=torch.float64, device=_dev())
        _lib.check(self._lib.vfem_copy_d2d(_ptr(out), ctypes.c_void_p(p), n * 3 * 8, _stream()))
        return out

    def debug_get_x(self, l):
        return _to_np(self._field(0, l))

    def debug_get_b(self, l):
        return _to_np(self._field(1, l))

    def _pcg_check_inputs(self, u, b):
        if isinstance(u, torch.Tensor) and isinstance(b, torch.Tensor) and u.shape != b.shape:
            raise RuntimeError("x and b should have the same size")

    def _pcg_search_direction(self):
        return _to_np(self._field(2, 0))


class _GenericMultigridSolver(_MultigridSolver):
    """MultigridSolver<p,..,p> on the generic path (``vfem_gmg_*``)."""

    _MG_PREFIX = "vfem_gmg_"


# ----------------------------------------------------------------------------------------------
# TensorProductSimulator<p,..,p>
# ----------------------------------------------------------------------------------------------

def _matched_regions(sim, bcPath):
    """the regions of a boundary-condition file with the nodes their boxes hold (inclusive test on node coordinates), in file
    order: (kind, comps, value, the matched indices per axis, their count)"""
    N = sim.N
    size = sim._bbmax - sim._bbmin
    spacing = size / (sim._nn - 1.0)
    coords = [sim._bbmin[d] + np.arange(sim._nn[d]) * spacing[d] for d in range(N)]
    for kind, comps, value, lo, hi, relative in _parse_regions(bcPath):
        lo, hi = np.array(lo[:N]), np.array(hi[:N])
        if relative:
            lo, hi = sim._bbmin + lo * size, sim._bbmin + hi * size
        sel = [np.flatnonzero((coords[d] >= lo[d]) & (coords[d] <= hi[d])) for d in range(N)]
        yield kind, comps, value, sel, int(np.prod([s.size for s in sel]))


def _write_force_region(loads, sel, value, count):
    """a force region into the device tensor ``loads`` [nodes per axis.., N]: split evenly over the matched nodes"""
    if count == 0:
        raise RuntimeError("Force constraint region unmatched")
    N = loads.shape[-1]
    ix = tuple(torch.from_numpy(sel[d]).to(_dev()).reshape([-1 if k == d else 1 for k in range(N)]) for d in range(N))
    loads[ix] = torch.tensor(value[:N], dtype=torch.float64, device=_dev()) / count


class _Simulator:
    """TensorProductSimulator<p,..,p> (VoxelFEM.cc:48-92; TPS.hh:219-1419) over a simulator handle of ``libvfem``: N
    dimensions, degree P.  The two subclasses name the C entry points (``_SIM_PREFIX``), create the handle and hold what
    only one of the paths has."""

    N = 3
    P = 1
    _SIM_PREFIX = None             # "vfem_sim_" (tuned <1,1,1>) or "vfem_gsim_" (generic path)
    _COMPLIANCE = None             # full name of the compliance entry point (the tuned one has no "sim_" in its name)
    _MG_CLASS = None
    # whether <prefix>get_densities writes every STORED element (node-grid elements + slab padding) or numElements() only:
    # getDensities_device sizes its result by it, a buffer sized the other way round would be overrun
    _GET_DENSITIES_WRITES_STORED = None

    def __init__(self, domainBoundingBox, numElemg, _element_padding=(0, 0)):
        """``_element_padding`` (slab decomposition, ndr_amd/distributed*.py): element layers kept below / above the node
        grid along x in the density array only (``setElementDensities_padded``)"""
        _lib.require_gpu()
        self._lib = _lib.load()
        N = self.N
        lo = np.asarray(domainBoundingBox[0], dtype=np.float64).reshape(-1)
        hi = np.asarray(domainBoundingBox[1], dtype=np.float64).reshape(-1)
        ne = [int(v) for v in numElemg]
        if len(ne) != N or lo.size != N or hi.size != N:
            raise RuntimeError("Dimension mismatch: %d vs %d" % (len(ne), N))
        self._bbmin, self._bbmax = lo.copy(), hi.copy()
        self._ne = np.array(ne, dtype=np.int64)
        self._nn = self.P * self._ne + 1
        h = ctypes.c_void_p()
        _lib.check(self._create(ctypes.byref(h), lo.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                hi.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                self._ne.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                int(_element_padding[0]), int(_element_padding[1])))
        self._h = h
        self._E0, self._Emin, self._gamma = 1.0, 1e-9, 3.0           # TPS.hh:1392-1394
        self._mask = np.zeros((self.numNodes(), N), dtype=bool)
        self._dvals = np.zeros((self.numNodes(), N))
        self._loads = torch.zeros((self.numNodes(), N), dtype=torch.float64, device=_dev())

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._c("destroy")(h)
            except Exception:
                pass
            self._h = None

    def _c(self, name):
        return getattr(self._lib, self._SIM_PREFIX + name)

    # ---- sizes / geometry ----
    def numNodes(self):
        return int(np.prod(self._nn))

    def numElements(self):
        return int(np.prod(self._ne))

    def NbElementsPerDimension(self):
        return self._ne.copy()

    def nodePosition(self, ni):
        idx = np.array(np.unravel_index(int(ni), tuple(self._nn)), dtype=np.float64)
        return self._bbmin + idx * (self._bbmax - self._bbmin) / (self._nn - 1.0)       # TPS.hh:275-278

    def elementIndexForGridCell(self, cellIdxs):
        return int(np.ravel_multi_index(tuple(int(c) for c in cellIdxs), tuple(self._ne)))

    def elementNodes(self, ei):
        e = np.array(np.unravel_index(int(ei), tuple(self._ne)))
        out = []
        for loc in np.ndindex(*([self.P + 1] * self.N)):
            out.append(int(np.ravel_multi_index(tuple(self.P * e + np.array(loc)), tuple(self._nn))))
        return np.array(out, dtype=np.uint64)

    def elemNodeGlobalIndex(self, ei, n):
        return int(self.elementNodes(ei)[int(n)])

    def _first_nodes(self):
        """(flat index of the first node of every element, node strides)"""
        eidx = np.stack(np.meshgrid(*[np.arange(n) for n in self._ne], indexing="ij"), -1).reshape(-1, self.N)
        nstr = np.array([int(np.prod(self._nn[d + 1:])) for d in range(self.N)])
        return (self.P * eidx) @ nstr, nstr

    def getMesh(self):
        """(V, F): all node positions; per element its corner nodes in Gmsh quad / hexahedron order (TPS.hh:531-565)"""
        N, p = self.N, self.P
        idx = np.stack(np.meshgrid(*[np.arange(n) for n in self._nn], indexing="ij"), -1).reshape(-1, N)
        V = self._bbmin + idx * (self._bbmax - self._bbmin) / (self._nn - 1.0)
        first, nstr = self._first_nodes()
        corners = [(0, 0), (1, 0), (1, 1), (0, 1)] if N == 2 else \
            [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)]
        F = np.stack([first + (p * np.array(c)) @ nstr for c in corners], axis=1)
        return V, F

    # ---- material / SIMP ----
    def readMaterial(self, materialPath):
        """TPS::readMaterial (TPS.hh:326-331): isotropic, orthotropic and symmetric / anisotropic material files"""
        self._set_etensor(_materials.read_material(materialPath, self.N))

    # ``sim.ETensor`` (TPS.hh:333-339) reads and assigns an ``ElasticityTensor``.  It is resolved per instance (the tuned class also
    # names it as a property): the public names of the classes themselves stay those a test pins.
    def __getattr__(self, name):              # (only reached for names that are neither set on the instance nor defined by the class)
        if name == "ETensor":
            return self._get_etensor()
        raise AttributeError(name)

    def __setattr__(self, name, value):
        if name == "ETensor":
            self._set_etensor(value)
        else:
            object.__setattr__(self, name, value)

    def _get_etensor(self):
        t = self.__dict__.get("_etensor")
        if t is None:
            return _materials.ElasticityTensor(1.0, 0.0, dim=self.N)           # ETensor(1, 0) default, TPS.hh:1379
        return _materials.ElasticityTensor(t, dim=self.N)                      # a copy: assigning to ETensor is what changes the simulator

    def _set_etensor(self, tensor):
        if not isinstance(tensor, _materials.ElasticityTensor):
            raise TypeError("ETensor takes an ndr_amd.ElasticityTensor")
        if tensor.dim != self.N:
            raise RuntimeError("Dimension mismatch: %d vs %d" % (tensor.dim, self.N))
        _materials.require_positive_definite(tensor)
        t = _materials.ElasticityTensor(tensor, dim=self.N)
        if t._iso is not None:                    # the isotropic entry point keeps its arithmetic: existing results stay bit-identical
            _lib.check(self._c("set_isotropic")(self._h, t._iso[0], t._iso[1]))
        else:
            self._push_tensor(np.ascontiguousarray(t._D))
        self._etensor = t
        self._direct_mg = None                    # the reference resets its solver when the operator changes (TPS.hh:404)

    def _tensor_paths(self):
        """the VFEM_PATH_* bits of include/vfem.h: which tuned kernels the current material runs on"""
        return int(self._c("tensor_paths")(self._h))

    def _push_simp(self):
        _lib.check(self._c("set_simp")(self._h, self._E0, self._Emin, self._gamma))

    def readDensities(self, materialPath, fieldName="density"):
        """TPS::readDensities (VoxelFEM.cc:54)"""
        self.setElementDensities(_densities_from_msh(materialPath, fieldName, self._ne, self.N))

    def constantStrainLoad(self, eps):
        """TPS::constantStrainLoad (VoxelFEM.cc:66), evaluated on the device"""
        sigma = self._get_etensor().doubleContract(eps)                       # C : eps with the actual tensor
        rho = self.getDensities_device()[:self.numElements()].reshape(tuple(int(n) for n in self._ne))
        return _to_np(_stress_load(sigma, (self._bbmax - self._bbmin) / self._ne, self.P, rho))

    @property
    def _GETK_MAX_ELEMENTS(self):
        """largest grid getK assembles: 2^30 entries of element matrices (the tuned class keeps its own, lower cap)"""
        return (1 << 30) // (self.P + 1) ** (2 * self.N)

    def getK(self):
        """TPS::getK (VoxelFEM.cc:62): assembled stiffness matrix, upper triangle, compressed columns (host, small grids)"""
        if self.numElements() > self._GETK_MAX_ELEMENTS:
            raise RuntimeError("getK assembles on the host; use applyK for grids of this size")
        rho = self.getDensities()[:self.numElements()]
        young = self._Emin + rho ** self._gamma * (self._E0 - self._Emin)
        nodes = self._first_nodes()[0][:, None] + self.elementNodes(0).astype(np.int64)[None, :]
        return _assemble_upper(nodes, self.fullDensityElementStiffnessMatrix(), young, self.N, self.numNodes())

    E_0 = property(lambda s: s._E0, lambda s, v: (setattr(s, "_E0", float(v)), s._push_simp())[0])
    E_min = property(lambda s: s._Emin, lambda s, v: (setattr(s, "_Emin", float(v)), s._push_simp())[0])
    gamma = property(lambda s: s._gamma, lambda s, v: (setattr(s, "_gamma", float(v)), s._push_simp())[0])

    def fullDensityElementStiffnessMatrix(self):
        ke = self.N * (self.P + 1) ** self.N
        K0 = np.empty((ke, ke))
        _lib.check(self._c("k0")(self._h, K0.ctypes.data_as(ctypes.c_void_p)))
        return K0

    def elementStiffnessMatrix(self, ei):
        rho = self.elementDensity(ei)
        return (self._Emin + rho ** self._gamma * (self._E0 - self._Emin)) * self.fullDensityElementStiffnessMatrix()

    def clearCachedElementStiffness(self):
        pass

    # ---- densities ----
    def _num_stored_elements(self):
        """elements of the density array: those of the node grid plus the padding layers of a slab simulator"""
        return int(self._c("num_stored_elements")(self._h))

    def setUniformDensities(self, density):
        if density > 1.0 or density < 0:
            raise RuntimeError("Density value (%f) has to be in between 0 and 1" % density)
        self.setElementDensities_padded(torch.full((self._num_stored_elements(),), float(density), dtype=torch.float64,
                                                   device=_dev()))

    def setElementDensities(self, rho):
        if self._num_stored_elements() != self.numElements():
            raise RuntimeError("this simulator stores padding element layers: use setElementDensities_padded")
        self.setElementDensities_padded(rho)

    def setElementDensities_padded(self, rho):
        """all stored element layers (padding below, the node grid's elements, padding above), x slowest"""
        t = _to_dev(rho, (self._num_stored_elements(),))
        _lib.check(self._c("set_densities")(self._h, _ptr(t), _stream()))

    def getDensities_device(self):
        n = self._num_stored_elements() if self._GET_DENSITIES_WRITES_STORED else self.numElements()
        t = torch.empty(n, dtype=torch.float64, device=_dev())
        _lib.check(self._c("get_densities")(self._h, _ptr(t), _stream()))
        return t

    def getDensities(self):
        return _to_np(self.getDensities_device())

    def setElementDensity(self, ei, value):
        t = self.getDensities_device()
        t[int(ei)] = float(value)
        # what came back is either the stored array or the unpadded one (which a padded simulator refuses)
        (self.setElementDensities_padded if self._GET_DENSITIES_WRITES_STORED else self.setElementDensities)(t)

    def elementDensity(self, ei):
        return float(self.getDensities_device()[int(ei)].item())

    # ---- boundary conditions ----
    def _push_dirichlet(self):
        m = np.zeros(self.numNodes(), dtype=np.uint8)
        for c in range(self.N):
            m |= self._mask[:, c].astype(np.uint8) << c
        vals = np.ascontiguousarray(self._dvals)
        _lib.check(self._c("set_dirichlet")(self._h, m.ctypes.data_as(ctypes.c_void_p),
                                            vals.ctypes.data_as(ctypes.c_void_p)))
        self._direct_mg = None                    # coarse Dirichlet masks of a cached hierarchy would be stale (TPS.hh:404)

    def _push_loads(self):
        """mirror ``_loads`` into the C simulator where it keeps a copy (the tuned path)"""

    def applyDisplacementsAndLoadsFromFile(self, bcPath):
        """applyDisplacementsAndLoads (TPS.hh:358-409): inclusive box test on node coordinates; forces are
        split evenly over the matched nodes; Dirichlet components merge, conflicting values throw.  Force regions are
        written on the device: a host copy of the loads of a 513^3 grid would be 3.2 GB."""
        N = self.N
        shape = tuple(self._nn)
        mask3 = self._mask.reshape(shape + (N,))
        vals3 = self._dvals.reshape(shape + (N,))
        loads = self._loads.reshape(shape + (N,))
        for kind, comps, value, sel, count in _matched_regions(self, bcPath):
            if kind == "force":
                _write_force_region(loads, sel, value, count)
            else:
                if count == 0:
                    raise RuntimeError("Dirichlet region unmatched")
                blk = np.ix_(*sel)
                for c, name in enumerate("xyz"[:N]):
                    if name not in comps:
                        continue
                    already = mask3[..., c][blk]
                    if np.any(already & (np.abs(vals3[..., c][blk] - value[c]) > 1e-10)):
                        raise RuntimeError("Conflicting dirichlet displacements.")
                    vc = vals3[..., c]
                    mc = mask3[..., c]
                    vc[blk] = np.where(already, vc[blk], value[c])
                    mc[blk] = True
        self._push_dirichlet()
        self._push_loads()

    def _get_mask(self):
        return self._mask.copy()

    def _set_mask(self, mask):
        mask = np.asarray(mask, dtype=bool)
        if mask.shape != (self.numNodes(), self.N):
            raise RuntimeError("Size mismatch")
        self._mask = mask.copy()
        self._push_dirichlet()

    def _get_dvals(self):
        return self._dvals.copy()

    def _set_dvals(self, values):
        values = np.asarray(values, dtype=np.float64)
        if values.shape != (self.numNodes(), self.N):
            raise RuntimeError("Size mismatch")
        self._dvals = values.copy()
        self._push_dirichlet()

    dirichletMask = property(_get_mask, _set_mask)
    dirichletValues = property(_get_dvals, _set_dvals)

    def getDirichletVarsAndValues(self):
        idx = np.flatnonzero(self._mask.reshape(-1))
        return list(idx), list(self._dvals.reshape(-1)[idx])

    def getForceMask(self):
        return (_to_np(self._loads) != 0)

    def setLoads_device(self, f):
        self._loads = _to_dev(f, (self.numNodes(), self.N)).clone()
        self._push_loads()

    def buildLoadVector_device(self):
        return self._loads.clone()

    def buildLoadVector(self):
        return _to_np(self._loads)

    # ---- operators ----
    def applyK_device(self, u):
        u = _to_dev(u, (self.numNodes(), self.N))
        out = torch.empty_like(u)
        _lib.check(self._c("apply_k")(self._h, _ptr(u), _ptr(out), _stream()))
        return out

    def applyK(self, u):
        return _to_np(self.applyK_device(u))

    def complianceGradient_device(self, u):
        u = _to_dev(u, (self.numNodes(), self.N))
        g = torch.empty(self.numElements(), dtype=torch.float64, device=_dev())
        _lib.check(self._c("compliance_gradient")(self._h, _ptr(u), _ptr(g), _stream()))
        return g

    def _compliance(self, f, u):
        v = ctypes.c_double(0.0)
        _lib.check(getattr(self._lib, self._COMPLIANCE)(self._h, _ptr(f), _ptr(u), ctypes.byref(v), _stream()))
        return v.value

    def multigridSolver(self, numCoarseningLevels):
        return self._MG_CLASS(self, int(numCoarseningLevels))

    def _direct_levels(self):
        lv, ne = 0, self._ne.copy()
        while np.all(ne % 2 == 0) and np.prod(self.P * ne + 1) * self.N > 3000 and lv < 12:
            ne //= 2
            lv += 1
        return lv

    # TPS::solve's method: "auto" factorises K (band Cholesky, <prefix>direct_solve) when its band fits in band.BAND_CAP_BYTES
    # (8 GiB, a fixed cap: the choice depends on the grid only) and runs the multigrid-preconditioned CG stand-in above it;
    # "cholesky" and "pcg" force one of the two
    directSolver = "auto"

    def directBandBytes(self):
        return int(self._c("direct_band_bytes")(self._h))

    def numDirectFactorizations(self):
        return int(self._c("direct_factorizations")(self._h))

    def solve_device(self, f):
        """TPS::solve (TPS.hh:834-865) on the device: u = K^-1 f, 0 at the Dirichlet components.  The band Cholesky factor of K is
        kept until the operator changes, as the reference keeps its CHOLMOD factor; the stand-in is MG-PCG to a relative residual
        of 1e-11 (``_stand_in_solve`` of the two paths)."""
        if np.any(self._dvals[self._mask] != 0):
            raise RuntimeError("Nonzero Dirichlet constraints currently unsupported")
        f = _to_dev(f, (self.numNodes(), self.N))
        if _factorize(self.directSolver, self.directBandBytes()):
            u = torch.empty_like(f)
            _lib.check(self._c("direct_solve")(self._h, _ptr(f), _ptr(u), _stream()))
            return u
        mg = getattr(self, "_direct_mg", None)
        if mg is None:
            mg = self.multigridSolver(self._direct_levels())
            self._direct_mg = mg
        return self._stand_in_solve(mg, f)

    def solve(self, f):
        return _to_np(self.solve_device(f))

    def solveWithImposedLoads(self):
        return self.solve(self.buildLoadVector())


class TensorProductSimulator1_1_1(_Simulator):
    """``pyVoxelFEM.detail.TensorProductSimulator1_1_1``: the tuned <1,1,1> path (``vfem_sim_*``)."""

    N, P = 3, 1
    _SIM_PREFIX = "vfem_sim_"
    _COMPLIANCE = "vfem_compliance"
    _MG_CLASS = MultigridSolver1_1_1
    _GET_DENSITIES_WRITES_STORED = True
    _GETK_MAX_ELEMENTS = 1 << 21

    def _create(self, out, lo, hi, ne, pad_lo, pad_hi):
        return self._c("create_padded")(out, lo, hi, ne, pad_lo, pad_hi)

    ETensor = property(_Simulator._get_etensor, _Simulator._set_etensor)

    def _push_tensor(self, D):
        _lib.check(self._c("set_elasticity_tensor")(self._h, D.ctypes.data_as(ctypes.c_void_p)))

    def setUniformDensities(self, density):
        # filled by the library: no temporary (1 GiB at 512^3); it raises the same range error
        _lib.check(self._c("set_uniform_density")(self._h, float(density), _stream()))

    def _push_loads(self):
        _lib.check(self._c("set_loads")(self._h, _ptr(self._loads), _stream()))

    def applyK_device(self, u, variant=0):
        u = _to_dev(u, (self.numNodes(), 3))
        out = torch.empty_like(u)
        _lib.check(self._c("apply_k")(self._h, _ptr(u), _ptr(out), int(variant), _stream()))
        return out

    def _stand_in_solve(self, mg, f):
        u = mg.preconditionedConjugateGradient_device(torch.zeros((self.numNodes(), 3), dtype=torch.float64,
                                                                  device=_dev()),
                                                      f, 500, 1e-11, None, 1, 2, True)
        if not mg.last_relative_residual <= 1e-11:
            raise RuntimeError("TensorProductSimulator.solve: the iterative solve that stands in for the direct factorisation "
                               "did not converge (relative residual %.3e after %d iterations)"
                               % (mg.last_relative_residual, mg.last_iterations))
        return u


class _GenericSimulator(_Simulator):
    """Generic path (``vfem_gsim_*``): TensorProductSimulator<p,..,p> for N = 2, 3 and p = 1, 2 other than the tuned
    <1,1,1> instantiation -- the 2-D simulators the reference binds (VoxelFEM.cc:226, plane stress) and the degree-2
    elements its templates support (TPS.hh:97-110)."""

    _SIM_PREFIX = "vfem_gsim_"
    _COMPLIANCE = "vfem_gsim_compliance"
    _MG_CLASS = _GenericMultigridSolver
    _GET_DENSITIES_WRITES_STORED = False

    def _create(self, out, lo, hi, ne, pad_lo, pad_hi):
        return self._c("create_padded")(out, self.N, self.P, lo, hi, ne, pad_lo, pad_hi)

    def _push_tensor(self, D):
        _lib.check(self._c("set_elasticity_tensor")(self._h, D.ctypes.data_as(ctypes.c_void_p), int(D.shape[0])))

    def _stand_in_solve(self, mg, f):
        # a grid with odd element counts cannot be coarsened; beyond the dense-factorisation size it is solved by plain CG
        plain = mg.L == 0 and self.numNodes() * self.N > 40000
        u = mg.preconditionedConjugateGradient_device(
            torch.zeros((self.numNodes(), self.N), dtype=torch.float64, device=_dev()),
            f, 500000 if plain else 2000, 1e-11, None, 1, 0 if plain else 2, True)
        if mg.last_relative_residual > 1e-10:
            raise RuntimeError("direct-solve replacement did not converge (relative residual %g)" % mg.last_relative_residual)
        return u


class TensorProductSimulator1_1(_GenericSimulator):
    """``pyVoxelFEM.detail.TensorProductSimulator1_1`` (VoxelFEM.cc:226): bilinear quadrilaterals, plane stress."""
    N, P = 2, 1


class TensorProductSimulator2_2(_GenericSimulator):
    N, P = 2, 2


class TensorProductSimulator2_2_2(_GenericSimulator):
    """27-node hexahedra; supported by the reference templates (TPS.hh:97-110), unbound there (VoxelFEM.cc:226-229)."""
    N, P = 3, 2


# ----------------------------------------------------------------------------------------------
# objectives (TopologyOptimizationObjective.hh)
# ----------------------------------------------------------------------------------------------

class ComplianceObjective1_1_1:
    """ComplianceObjective (TopologyOptimizationObjective.hh:24-63): 1/2 f.u with a direct solve."""

    def __init__(self, simulator, skipSolve=False):
        self._sim = simulator
        self._f = simulator.buildLoadVector_device()
        self._u = torch.zeros_like(self._f)
        if not skipSolve:
            self.updateCache(None)

    def compliance(self):
        return self._sim._compliance(self._f, self._u)

    def evaluate(self, xPhys=None):
        return self.compliance()

    def gradient_device(self):
        return self._sim.complianceGradient_device(self._u)

    def gradient(self):
        return _to_np(self.gradient_device())

    def updateCache(self, xPhys):
        if xPhys is not None:
            self._sim.setElementDensities(xPhys)
        self._u = self._sim.solve_device(self._f)

    def u(self):
        return _to_np(self._u)

    def f(self):
        return _to_np(self._f)


class MultigridComplianceObjective1_1_1(ComplianceObjective1_1_1):
    """MultigridComplianceObjective (TopologyOptimizationObjective.hh:67-102)."""

    def __init__(self, mg_solver):
        self._mg = mg_solver
        self.cgIter = 100
        self.tol = 1e-5
        self.mgIterations = 1
        self.mgSmoothingIterations = 2
        self.fullMultigrid = True
        self.zeroInit = False
        self.residual_cb = None
        super().__init__(mg_solver.getSimulator(0), skipSolve=True)
        self.updateCache(None)          # the reference constructor solves once (:78-82)

    @property
    def mg(self):
        return self._mg

    def updateCache(self, xPhys):
        if xPhys is not None:
            self._sim.setElementDensities(xPhys)
        if self.zeroInit:
            self._u = torch.zeros_like(self._u)
        self._u = self._mg.preconditionedConjugateGradient_device(
            self._u, self._f, int(self.cgIter), float(self.tol), None, int(self.mgIterations),
            int(self.mgSmoothingIterations), bool(self.fullMultigrid), residual_cb=self.residual_cb)


# ----------------------------------------------------------------------------------------------
# filters / constraint (TopologyOptimizationFilter.hh, TopologyOptimizationConstraint.hh) -- device kernels
# (vfem_box_filter, vfem_projection*, vfem_mean); the public methods take/return numpy like the bound C++ classes,
# the *_dev variants work on float64 CUDA tensors.
# ----------------------------------------------------------------------------------------------

class _Filter:
    def __init__(self):
        self._grid = None

    def _set_grid(self, dims):
        self._grid = tuple(int(d) for d in dims)

    def _check(self):
        if self._grid is None:
            raise RuntimeError("Filter grid dimensions not set. Initialize a TopologyOpimizationProblem object "
                               "with this filter before using it.")

    def getGridDimensions(self):
        return np.array(self._grid)

    def _n3(self):
        g = list(self._grid) + [1] * (3 - len(self._grid))
        return (ctypes.c_int64 * 3)(*g)

    def apply(self, x):
        return _to_np(self.apply_dev(_to_dev(x).reshape(-1)))

    def backprop(self, g, x):
        return _to_np(self.backprop_dev(_to_dev(g).reshape(-1), _to_dev(x).reshape(-1)))


class ProjectionFilter(_Filter):
    """tanh projection (TopologyOptimizationFilter.hh:55-79)."""

    def __init__(self):
        super().__init__()
        self._beta = 1.0

    def _get_beta(self):
        return self._beta

    def _set_beta(self, beta):
        if beta <= 0:
            raise RuntimeError("Beta parameter has to be positive (received beta = %f)" % beta)
        self._beta = float(beta)

    beta = property(_get_beta, _set_beta)

    def apply_dev(self, x):
        out = torch.empty_like(x)
        _lib.check(_lib.load().vfem_projection(x.numel(), self._beta, _ptr(x), _ptr(out), _stream()))
        return out

    def backprop_dev(self, g, x):
        out = torch.empty_like(g)
        _lib.check(_lib.load().vfem_projection_backprop(g.numel(), self._beta, _ptr(g), _ptr(x), _ptr(out), _stream()))
        return out


class SmoothingFilter(_Filter):
    """Box filter, each row normalised by its in-bounds neighbour count (TopologyOptimizationFilter.hh:105-162);
    the sparse matrix of the reference is replaced by a direct stencil kernel."""

    def __init__(self):
        super().__init__()
        self._radius = 1

    def _get_radius(self):
        return self._radius

    def _set_radius(self, r):
        self._radius = int(r)

    radius = property(_get_radius, _set_radius)

    def _run(self, x, transpose):
        self._check()
        out = torch.empty_like(x)
        _lib.check(_lib.load().vfem_box_filter(self._n3(), self._radius, _ptr(x), _ptr(out), int(transpose), _stream()))
        return out

    def apply_dev(self, x):
        return self._run(x, 0)

    def backprop_dev(self, g, x):
        return self._run(g, 1)


class PythonFilter(_Filter):
    """Callback filter (TopologyOptimizationFilter.hh:81-103): apply_cb(in, out), backprop_cb(in, vars, out) on numpy."""

    def __init__(self):
        super().__init__()
        self.apply_cb = None
        self.backprop_cb = None

    def apply_dev(self, x):
        if self.apply_cb is None:
            raise RuntimeError("Apply callback must be configured")
        xin = _to_np(x)
        out = np.zeros_like(xin)
        self.apply_cb(xin, out)
        return _to_dev(out)

    def backprop_dev(self, g, x):
        if self.backprop_cb is None:
            raise RuntimeError("Backprop callback must be configured")
        gin = _to_np(g)
        out = np.zeros_like(gin)
        self.backprop_cb(gin, _to_np(x), out)
        return _to_dev(out)


class LangelaarFilter(_Filter):
    """Additive-manufacturing overhang filter (TopologyOptimizationFilter.hh:164-278): each element of layer k >= 1 (the
    last grid axis) is capped by a smooth maximum of the filtered elements that support it on layer k-1, so the forward is
    a march up the layers and the backward a march down (vfem_langelaar_*).  As in the reference, backprop differentiates
    the most recent apply: its output and smax caches stay on the device, owned by the filter (the tensor apply_dev returns
    is that output cache).  The adjoint march covers all layers also on 3-D grids with ny != nz, where the reference's loop
    stops after ny layers."""

    _EPS, _P, _Q = 1e-4, 40.0, 40.0 - 1.58      # fixed by the reference (:266-276), not exposed by its binding

    def __init__(self):
        super().__init__()
        self._out = self._smax = self._work = None

    def _set_grid(self, dims):
        super()._set_grid(dims)
        self._out = self._smax = self._work = None

    def _nl(self):
        g = self._grid
        return (ctypes.c_int64 * 3)(*((g[0], 1, g[1]) if len(g) == 2 else g))    # layer axis last

    def _check_size(self, *ts):
        n = int(np.prod(self._grid))
        for t in ts:
            if t.numel() != n:
                raise RuntimeError("LangelaarFilter: input of size %d does not match the grid (%d elements)" % (t.numel(), n))

    def apply_dev(self, x):
        self._check()
        self._check_size(x)
        out, smax = torch.empty_like(x), torch.empty_like(x)
        _lib.check(_lib.load().vfem_langelaar_apply(self._nl(), self._EPS, self._P, self._Q, _ptr(x), _ptr(out), _ptr(smax),
                                                    _stream()))
        self._out, self._smax = out, smax
        return out

    def backprop_dev(self, g, x):
        self._check()
        if self._out is None:
            raise RuntimeError("LangelaarFilter: backprop called before apply")
        self._check_size(g, x)
        n = self._nl()
        if self._work is None:
            self._work = torch.empty(2 * n[0] * n[1], dtype=torch.float64, device=_dev())
        grad = torch.empty_like(g)
        _lib.check(_lib.load().vfem_langelaar_backprop(n, self._EPS, self._P, self._Q, _ptr(g), _ptr(x), _ptr(self._out),
                                                       _ptr(self._smax), _ptr(self._work), _ptr(grad), _stream()))
        return grad


def applyFilter(filter, x):
    filter._check()
    return filter.apply(np.asarray(x, dtype=np.float64))


class TotalVolumeConstraint:
    """1 - mean(x)/v (TopologyOptimizationConstraint.hh:21-34)."""

    def __init__(self, volumeFraction):
        self.volumeFraction = float(volumeFraction)

    def evaluate_dev(self, x):
        m = ctypes.c_double(0.0)
        _lib.check(_lib.load().vfem_mean(x.numel(), _ptr(x), ctypes.byref(m), _stream()))
        return 1.0 - m.value / self.volumeFraction

    def evaluate(self, x):
        return self.evaluate_dev(_to_dev(x).reshape(-1))

    def backprop_dev(self, x):
        return torch.full((x.numel(),), -1.0 / (self.volumeFraction * x.numel()), dtype=torch.float64, device=_dev())

    def backprop(self, x):
        return np.full(np.size(x), -1.0 / (self.volumeFraction * np.size(x)))


# ----------------------------------------------------------------------------------------------
# problem + optimality criterion (TopologyOptimizationProblem.hh, OptimalityCriterion.hh); the design variables,
# every filtered stage and the sensitivities stay on the device between calls
# ----------------------------------------------------------------------------------------------

class TopologyOptimizationProblem1_1_1:
    def __init__(self, simulator, objective, constraints, filters=()):
        self._sim = simulator
        self._objective = objective
        self._constraints = list(constraints)
        self._filters = list(filters)
        self._nvars = simulator.numElements()
        for f in self._filters:
            f._set_grid(simulator.NbElementsPerDimension())
        z = lambda: torch.zeros(self._nvars, dtype=torch.float64, device=_dev())
        self._cached = [z() for _ in range(len(self._filters) + 1)]
        self._vars_set = False

    def numVars(self):
        return self._nvars

    def getVars(self):
        return _to_np(self._cached[0])

    def getVars_device(self):
        return self._cached[0]

    def setVars(self, x, forceUpdate=False):
        x = _to_dev(x, (self._nvars,))
        if (not forceUpdate) and self._vars_set and float((x - self._cached[0]).norm()) < 1e-16:
            return False                                             # Problem.hh:50-51
        self._cached[0] = x.clone()
        for i, f in enumerate(self._filters):
            self._cached[i + 1] = f.apply_dev(self._cached[i])
        self._objective.updateCache(self._cached[-1])
        self._vars_set = True
        return True

    def _need_vars(self):
        if not self._vars_set:
            raise RuntimeError("Must call setVars first!")

    def evaluateOCConstraintAtVars_dev(self, x):
        if len(self._constraints) != 1 or not isinstance(self._constraints[0], TotalVolumeConstraint):
            raise RuntimeError("Applicable only for a topology optimization with a single (volume) constraint")
        for f in self._filters:
            x = f.apply_dev(x)
        return self._constraints[0].evaluate_dev(x)

    def evaluateOCConstraintAtVars(self, x):
        return self.evaluateOCConstraintAtVars_dev(_to_dev(x, (self._nvars,)))

    def evaluateObjective(self):
        self._need_vars()
        return self._objective.evaluate(None)

    def evaluateObjectiveGradient_device(self):
        self._need_vars()
        g = self._objective.gradient_device()
        nf = len(self._filters)
        for i in range(nf):
            g = self._filters[nf - 1 - i].backprop_dev(g, self._cached[nf - 1 - i])
        return g

    def evaluateObjectiveGradient(self):
        return _to_np(self.evaluateObjectiveGradient_device())

    def evaluateConstraints(self):
        self._need_vars()
        return np.array([c.evaluate_dev(self._cached[-1]) for c in self._constraints])

    def evaluateConstraintsJacobian_device(self):
        self._need_vars()
        nf = len(self._filters)
        rows = []
        for c in self._constraints:
            d = c.backprop_dev(self._cached[-1])
            for i in range(nf):
                d = self._filters[nf - 1 - i].backprop_dev(d, self._cached[nf - 1 - i])
            rows.append(d)
        return rows

    def evaluateConstraintsJacobian(self):
        return np.stack([_to_np(r) for r in self.evaluateConstraintsJacobian_device()]).reshape(len(self._constraints), self._nvars)

    def getDensities(self):
        return self._sim.getDensities()

    def getSimulator(self):
        return self._sim

    objective = property(lambda s: s._objective, lambda s, o: setattr(s, "_objective", o))
    constraints = property(lambda s: list(s._constraints), lambda s, c: setattr(s, "_constraints", list(c)))

    def _set_filters(self, filters):
        self._filters = list(filters)
        for f in self._filters:
            f._set_grid(self._sim.NbElementsPerDimension())
        self._cached = [self._cached[0]] + [torch.zeros(self._nvars, dtype=torch.float64, device=_dev()) for _ in self._filters]

    filters = property(lambda s: list(s._filters), _set_filters)


class OCOptimizer1_1_1:
    """OCOptimizer (OptimalityCriterion.hh:30-81); the multiplier bracket persists across steps.  Each bisection
    probe is three small kernels (candidate step, filters, mean) and one scalar read-back."""

    def __init__(self, problem):
        self._p = problem
        self._lmin, self._lmax = 1.0, 2.0

    def step(self, m=0.2, ctol=1e-6):
        p = self._p
        lib = _lib.load()
        dJ = p.evaluateObjectiveGradient_device()
        dc = p.evaluateConstraintsJacobian_device()[0]
        x0 = p.getVars_device().clone()
        cand = torch.empty_like(x0)

        def stepped(lam):
            _lib.check(lib.vfem_oc_candidate(x0.numel(), _ptr(x0), _ptr(dJ), _ptr(dc), float(lam), float(m), _ptr(cand), _stream()))
            return cand

        def ceval(lam):
            return p.evaluateOCConstraintAtVars_dev(stepped(lam))

        while ceval(self._lmin) > 0:
            self._lmax = self._lmin
            self._lmin /= 2
        while ceval(self._lmax) < 0:
            self._lmin = self._lmax
            self._lmax *= 2
        mid = 0.5 * (self._lmin + self._lmax)
        vol = ceval(mid)
        while abs(vol) > ctol:
            if vol < 0:
                self._lmin = mid
            if vol > 0:
                self._lmax = mid
            mid = 0.5 * (self._lmin + self._lmax)
            vol = ceval(mid)
        p.setVars(stepped(mid).clone())
        print("objective, constraint, lambda estimate: %g\t%g\t%g" % (p.evaluateObjective(),
                                                                      p.evaluateConstraints()[0], mid))


# ----------------------------------------------------------------------------------------------
# module-level factories (VoxelFEM.cc:136-216, 234-240)
# ----------------------------------------------------------------------------------------------

def TensorProductSimulator(degreesPerDimension, domainBBox, elementsPerDimension):
    """VoxelFEM.cc:234-240 (+ the degree-2 instantiations the reference leaves commented out, :227,229)"""
    degs = [int(d) for d in degreesPerDimension]
    classes = {(1, 1, 1): TensorProductSimulator1_1_1, (1, 1): TensorProductSimulator1_1,
               (2, 2): TensorProductSimulator2_2, (2, 2, 2): TensorProductSimulator2_2_2}
    cls = classes.get(tuple(degs))
    if cls is None:
        raise RuntimeError("No template instantiation matching degreesPerDimension!")
    return cls(domainBBox, elementsPerDimension)


def TopologyOptimizationProblem(simulator, objective, constraints, filters):
    return TopologyOptimizationProblem1_1_1(simulator, objective, constraints, filters)


def ComplianceObjective(simulator):
    return ComplianceObjective1_1_1(simulator)


def MultigridComplianceObjective(mg_solver):
    return MultigridComplianceObjective1_1_1(mg_solver)


def OCOptimizer(problem):
    return OCOptimizer1_1_1(problem)


# ----------------------------------------------------------------------------------------------
# benchmark registry (VoxelFEM.cc:245-255)
# ----------------------------------------------------------------------------------------------
import time as _time

_py_timers = {}
_py_running = {}


def benchmark_reset():
    _lib.load().vfem_timers_reset()
    _py_timers.clear()
    _py_running.clear()


def benchmark_start_timer_section(name):
    _py_running[name] = _time.perf_counter()


def benchmark_stop_timer_section(name):
    t0 = _py_running.pop(name, None)
    if t0 is not None:
        s, c = _py_timers.get(name, (0.0, 0))
        _py_timers[name] = (s + _time.perf_counter() - t0, c + 1)


benchmark_start_timer = benchmark_start_timer_section
benchmark_stop_timer = benchmark_stop_timer_section


def benchmark_to_dict():
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.load().vfem_timers_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, sec, calls = line.split("\t")
        out[name] = {"seconds": float(sec), "invocations": int(calls)}
    for name, (s, c) in _py_timers.items():
        out[name] = {"seconds": s, "invocations": c}
    return out


def benchmark_report(include_messages=False):
    for name, e in sorted(benchmark_to_dict().items()):
        print("%-40s %12.6f s  (%d calls)" % (name, e["seconds"], e["invocations"]))


detail = types.ModuleType(__name__ + ".detail")
detail.TensorProductSimulator1_1_1 = TensorProductSimulator1_1_1
detail.TensorProductSimulator2_2_2 = TensorProductSimulator2_2_2
detail.TensorProductSimulator1_1 = TensorProductSimulator1_1
detail.TensorProductSimulator2_2 = TensorProductSimulator2_2
detail.MultigridSolver1_1_1 = MultigridSolver1_1_1
detail.TopologyOptimizationProblem1_1_1 = TopologyOptimizationProblem1_1_1
detail.ComplianceObjective1_1_1 = ComplianceObjective1_1_1
detail.MultigridComplianceObjective1_1_1 = MultigridComplianceObjective1_1_1
detail.OCOptimizer1_1_1 = OCOptimizer1_1_1
detail.Filter = _Filter
detail.Constraint = TotalVolumeConstraint
sys.modules[detail.__name__] = detail
