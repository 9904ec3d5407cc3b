"""CPU-only checks: the C-ABI library loads and exports every symbol include/vfem.h declares (no compute
calls), the ctypes table matches the header, and the host-side logic (filters, constraint, BC parsing,
Dirichlet coarsening inputs) agrees with the oracle."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _header_functions():
    src = open(os.path.join(ROOT, "include", "vfem.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vfem_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from ndr_amd import _lib
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = _header_functions()
    assert len(names) > 40
    for n in names:
        assert hasattr(lib, n), n


def test_ctypes_table_matches_header():
    from ndr_amd import _lib
    assert sorted(_lib.SIGNATURES) == _header_functions()
    lib = _lib.load()
    assert lib.vfem_version() >= 100
    assert lib.vfem_device_count() >= 0


def test_no_gpu_means_loud_failure():
    from ndr_amd import _lib
    if _lib.load().vfem_device_count() > 0:
        pytest.skip("GPU present")
    from ndr_amd import pyVoxelFEM as pv
    with pytest.raises(RuntimeError):
        pv.TensorProductSimulator([1, 1, 1], [np.zeros(3), np.ones(3)], [4, 4, 4])


def _create_padded(lib, ne, pad):
    import ctypes
    h = ctypes.c_void_p()
    lo, hi, n = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1), (ctypes.c_int64 * 3)(*ne)
    return lib.vfem_sim_create_padded(ctypes.byref(h), lo, hi, n, pad[0], pad[1]), h


def test_padded_create_refuses_negative_padding():
    """the argument checks of vfem_sim_create_padded come before any device call: error code 1, a message, no handle"""
    from ndr_amd import _lib
    lib = _lib.load()
    assert not hasattr(lib, "vfem_sim_set_next_element_padding")
    for pad in ((-1, 0), (0, -1)):
        rc, h = _create_padded(lib, (4, 4, 4), pad)
        assert rc == 1 and not h.value
        assert b"negative padding" in lib.vfem_last_error()
    rc, h = _create_padded(lib, (0, 4, 4), (2, 2))
    assert rc == 1 and not h.value


@pytest.mark.gpu
def test_failed_padded_create_leaves_nothing_behind():
    """a create that fails its argument checks must not pad the next simulator of the thread"""
    import ctypes
    from ndr_amd import _lib
    lib = _lib.load()
    rc, h = _create_padded(lib, (0, 4, 4), (2, 3))
    assert rc == 1
    h = ctypes.c_void_p()
    lo, hi, n = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1), (ctypes.c_int64 * 3)(4, 4, 4)
    _lib.check(lib.vfem_sim_create(ctypes.byref(h), lo, hi, n))
    try:
        assert lib.vfem_sim_num_stored_elements(h) == lib.vfem_sim_num_elements(h) == 64
    finally:
        lib.vfem_sim_destroy(h)
    rc, h = _create_padded(lib, (4, 4, 4), (2, 3))
    assert rc == 0
    try:
        assert lib.vfem_sim_num_stored_elements(h) == (4 + 5) * 16 and lib.vfem_sim_num_elements(h) == 64
    finally:
        lib.vfem_sim_destroy(h)


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "ndr_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "voxel_ref" not in txt, (dirpath, f)


@pytest.mark.parametrize("name", ["sincos_f32", "voxel_xyz", "unscale_lo", "mkd", "glds16"])
def test_shared_device_helpers_are_defined_once(name):
    """the backward MLP kernels must see the forward kernels' features, coordinates and ReLU masks bit for bit (mlp_device.h), and
    mkd / glds16 live in device_utils.h: a second definition in any kernel file is a copy that can drift"""
    csrc = os.path.join(ROOT, "ndr_amd", "csrc")
    definition = re.compile(r"^[ \t]*__device__\b[^;{}()]*\b%s[ \t]*\(" % name, re.M)
    found = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))
             for _ in definition.finditer(open(os.path.join(csrc, f)).read())]
    assert found == ["device_utils.h" if name in ("mkd", "glds16") else "mlp_device.h"]


@pytest.mark.parametrize("text,home", [(r"MG\.hh:301-305", ["gs_colors.h"]),                                  # the colour walk's increment rule
                                       (r"__global__[^;{}]*\bk\w*_dense_finish\s*\(", ["kernels_mg.hip"]),       # a finish kernel of a dense inverse
                                       (r"\b40000\b", ["vfem_internal.h"] * 2),     # DENSE_COARSEST_MAX_DOFS, and WAVE_SWEEP_MAX_NODES which is another limit
                                       (r"it % 8 == 0", ["hom.hip"]),                                            # the cell problems' read-back rule
                                       (r"no convergence in %d iterations", ["hom.hip"])])                       # and their error
def test_shared_host_rules_are_written_once(text, home):
    """the colour order of the multicolour sweep, the kernel that finishes a coarsest-level inverse and the dense solver's limit are
    said in one file each: the four sweep launchers, the two hierarchies and the C boundary use that one; so is the batched PCG of
    the periodic cell problems (hom_pcg), which both of its preconditioners run"""
    csrc = os.path.join(ROOT, "ndr_amd", "csrc")
    found = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))
             for _ in re.finditer(text, open(os.path.join(csrc, f)).read())]
    assert found == home


@pytest.mark.gpu
def test_filters_and_constraint_match_oracle():
    from ndr_amd import pyVoxelFEM as pv
    from oracle import vfem_oracle as vo
    rng = np.random.default_rng(0)
    for grid in [(7, 5), (6, 4, 5)]:
        x = rng.uniform(0, 1, size=int(np.prod(grid)))
        g = rng.standard_normal(x.size)
        for radius in (1, 2):
            a, b = pv.SmoothingFilter(), vo.OracleSmoothingFilter(radius)
            a._set_grid(grid)
            a.radius = radius
            b.set_grid(grid)
            assert np.abs(a.apply(x) - b.apply(x)).max() < 1e-14
            assert np.abs(a.backprop(g, x) - b.backprop(g, x)).max() < 1e-14
            assert np.abs(pv.applyFilter(a, x) - b.apply(x)).max() < 1e-14
        for beta in (1.0, 4.0):
            a, b = pv.ProjectionFilter(), vo.OracleProjectionFilter(beta)
            a.beta = beta
            assert np.abs(a.apply(x) - b.apply(x)).max() < 1e-15
            assert np.abs(a.backprop(g, x) - b.backprop(g, x)).max() < 1e-15
        c, d = pv.TotalVolumeConstraint(0.4), vo.OracleVolumeConstraint(0.4)
        assert abs(c.evaluate(x) - d.evaluate(x)) < 1e-15
        assert np.abs(c.backprop(x) - d.backprop(x)).max() < 1e-18
    with pytest.raises(RuntimeError):
        pv.ProjectionFilter().beta = -1.0
    with pytest.raises(RuntimeError):
        pv.applyFilter(pv.SmoothingFilter(), np.zeros(4))
    with pytest.raises(RuntimeError):
        f = pv.PythonFilter()
        f._set_grid((2, 2))
        f.apply(np.zeros(4))


def test_region_parser_matches_reference_semantics(tmp_path):
    from ndr_amd.pyVoxelFEM import _parse_regions
    golden = os.path.join(ROOT, "bcs", "3d", "bridge.bc")
    regs = _parse_regions(golden)
    assert [r[0] for r in regs] == ["dirichlet", "dirichlet", "force"]
    assert regs[0][1] == "xyz" and regs[1][1] == "x"
    bad = tmp_path / "bad.bc"
    bad.write_text('{"regions": [{"type": "traction", "value": [0,0,0], "box%": {"minCorner": [0,0,0], "maxCorner": [1,1,1]}}]}')
    with pytest.raises(RuntimeError):
        _parse_regions(str(bad))


@pytest.mark.parametrize("source,kernels,windows", [
    ("kernels_q2.hip", ["k_apply_q2_marchILi0"], 84),
    ("kernels_l1_merged.hip", ["k_l1_mergedILi0E", "k_l1_mergedILi1E", "k_l1_mergedILi2E", "k_l1_pair_rowsILi0E", "k_l1_pair_rowsILi1E"], None),
    ("kernels_gs_march.hip", ["k_gs_march_mf0ILi%dELi%dELi%dEEE" % (a, f, m) for a in (0, 1) for f in (0, 1) for m in (0, 1)], None)])
def test_pipelined_scalar_loads_are_hazard_free(tmp_path, source, kernels, windows):
    """k_apply_q2_march (sload12_issue / sload12_wait), the level-1 per-class kernels and the node-per-lane marching sweep (coef_rows.h:
    srow_issue / srow_wait) leave scalar loads in flight across compiler-generated code; that is only safe while no instruction
    touches the destination SGPRs before the wait.  Compile the kernels to ISA (cross-compile, no GPU needed) and scan them."""
    import shutil
    import subprocess
    import sys
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "ndr_amd", "csrc", source)
    asm = str(tmp_path / "k.s")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=on", "-S", "--cuda-device-only",
                           src, "-o", asm], stderr=subprocess.DEVNULL)
    for k in kernels:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_sload_pipeline.py"), asm, k], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout
        assert " 0 violations" in out.stdout and " 0 request..wait windows" not in out.stdout, out.stdout
        if windows is not None:
            assert "%d request..wait windows" % windows in out.stdout, out.stdout


def test_host_helpers_of_getk_constant_strain_load_read_densities(tmp_path):
    """host logic behind TensorProductSimulator.getK / constantStrainLoad / readDensities (VoxelFEM.cc:54,62,66) against the
    oracle, 2-D and 3-D (no GPU: the helpers take plain arrays)"""
    import scipy.sparse as sp
    import torch
    from ndr_amd import io, pyVoxelFEM as pv
    from oracle import vfem_oracle as vo
    for ne, dom in (((5, 3), ([0, 0], [2.0, 1.0])), ((4, 3, 2), ([0, 0, 0], [1.5, 1.0, 0.8]))):
        N = len(ne)
        o = vo.OracleSim(dom, ne, vo.lame(1.0, 0.3, N))
        o.Emin = 1e-4
        rho = np.random.default_rng(3).uniform(0.05, 1.0, o.num_elems)
        o.set_densities(rho)
        nodes, _ = o.element_dofs()
        K = pv._assemble_upper(nodes, o.K0, o.young(), N, o.num_nodes)
        A = o.assemble()
        assert abs(K.full() - A).max() < 1e-13 and sp.tril(K.toSciPy(), -1).nnz == 0
        assert K.nz == K.Ap[-1] == len(K.Ai) == len(K.Ax) and K.symmetry_mode == "UPPER_TRIANGLE"
        eps = np.random.default_rng(4).standard_normal((N, N))
        eps = eps + eps.T
        lam, mu = o.lam_mu
        F = pv._constant_strain_load(eps, lam, mu, o.h, 1, torch.from_numpy(rho.reshape(ne))).numpy()
        ref = o.constant_strain_load(eps)
        assert np.abs(F - ref).max() < 1e-13 * np.abs(ref).max()
    # element field of a hexahedral .msh, elements in reverse order
    ne = (4, 3, 2)
    idx = np.stack(np.meshgrid(*[np.arange(n + 1) for n in ne], indexing="ij"), -1).reshape(-1, 3)
    V = idx * np.array([0.4, 0.3, 0.2]) + np.array([1.0, -2.0, 0.5])
    nstr = np.array([(ne[1] + 1) * (ne[2] + 1), ne[2] + 1, 1])
    eidx = np.stack(np.meshgrid(*[np.arange(n) for n in ne], indexing="ij"), -1).reshape(-1, 3)
    Fh = np.stack([eidx @ nstr + np.array([(m >> 2) & 1, (m >> 1) & 1, m & 1]) @ nstr for m in (0, 1, 3, 2, 4, 5, 7, 6)], 1)
    rho = np.random.default_rng(5).uniform(size=len(Fh))
    path = str(tmp_path / "field.msh")
    io.MSHFieldWriter(path, V, Fh[::-1]).addField("density", rho[::-1])
    assert np.array_equal(pv._densities_from_msh(path, "density", ne, 3), rho)
    with pytest.raises(RuntimeError):
        pv._densities_from_msh(str(tmp_path / "field.obj"), "density", ne, 3)


# Public surface of the single-GPU binding classes (names without a leading underscore; inspect.signature of the callables, the
# kind of everything else), recorded before the simulators and the multigrid solvers were folded onto one base class each.
_SIM_SURFACE = {"E_0": "property",
 "E_min": "property",
 "N": "int",
 "NbElementsPerDimension": "(self)",
 "P": "int",
 "applyDisplacementsAndLoadsFromFile": "(self, bcPath)",
 "applyK": "(self, u)",
 "applyK_device": "(self, u)",
 "buildLoadVector": "(self)",
 "buildLoadVector_device": "(self)",
 "clearCachedElementStiffness": "(self)",
 "complianceGradient_device": "(self, u)",
 "constantStrainLoad": "(self, eps)",
 "directBandBytes": "(self)",
 "directSolver": "str",
 "dirichletMask": "property",
 "dirichletValues": "property",
 "elemNodeGlobalIndex": "(self, ei, n)",
 "elementDensity": "(self, ei)",
 "elementIndexForGridCell": "(self, cellIdxs)",
 "elementNodes": "(self, ei)",
 "elementStiffnessMatrix": "(self, ei)",
 "fullDensityElementStiffnessMatrix": "(self)",
 "gamma": "property",
 "getDensities": "(self)",
 "getDensities_device": "(self)",
 "getDirichletVarsAndValues": "(self)",
 "getForceMask": "(self)",
 "getK": "(self)",
 "getMesh": "(self)",
 "multigridSolver": "(self, numCoarseningLevels)",
 "nodePosition": "(self, ni)",
 "numDirectFactorizations": "(self)",
 "numElements": "(self)",
 "numNodes": "(self)",
 "readDensities": "(self, materialPath, fieldName='density')",
 "readMaterial": "(self, materialPath)",
 "setElementDensities": "(self, rho)",
 "setElementDensities_padded": "(self, rho)",
 "setElementDensity": "(self, ei, value)",
 "setLoads_device": "(self, f)",
 "setUniformDensities": "(self, density)",
 "solve": "(self, f)",
 "solveWithImposedLoads": "(self)",
 "solve_device": "(self, f)"}
_MG_SURFACE = {"applyK": "(self, l, u)",
 "applyK_device": "(self, l, u)",
 "computeResidual": "(self, l, u, b)",
 "computeResidual_device": "(self, l, u, b)",
 "debugMulticolorVisit": "(self)",
 "getSimulator": "(self, l)",
 "interpolation_device": "(self, fine_level, values, out=None)",
 "preconditionedConjugateGradient": "(self, u, b, maxIter, tol, it_callback=None, mgIterations=1, mgSmoothingIterations=1, "
                                    "fullMultigrid=False)",
 "preconditionedConjugateGradient_device": "(self, u, b, maxIter, tol, it_callback=None, mgIterations=1, "
                                           "mgSmoothingIterations=1, fullMultigrid=False, residual_cb=None)",
 "restriction_device": "(self, fine_level, values)",
 "setSymmetricGaussSeidel": "(self, symmetric)",
 "smoothing": "(self, l, u, b)",
 "smoothing_device": "(self, l, u, b, forward=True)",
 "solve": "(self, u, f, numSteps, numSmoothingSteps, stiffnessUpdated=False, zeroDirichlet=False, it_callback=None, "
          "fullMultigrid=False)",
 "solve_device": "(self, u, f, numSteps, numSmoothingSteps, stiffnessUpdated=False, zeroDirichlet=False, it_callback=None, "
                 "fullMultigrid=False)",
 "updateBlockKs": "(self)",
 "updateElementStiffnessMatrices": "(self)",
 "zeroOutDirichletComponents": "(self, l, u)"}
_VIEW_SURFACE = {"NbElementsPerDimension": "(self)", "dirichletMask": "property", "numElements": "(self)", "numNodes": "(self)"}
_SIM_TUNED_ONLY = {"ETensor": "property", "applyK_device": "(self, u, variant=0)"}
_MG_TUNED_ONLY = {"coarsestSolve_device": "(self, b)", "debug_get_b": "(self, l)", "debug_get_x": "(self, l)"}


def _surface(cls):
    import inspect
    out = {}
    for name in dir(cls):
        if not name.startswith("_"):
            a = inspect.getattr_static(cls, name)
            out[name] = str(inspect.signature(a)) if callable(a) else type(a).__name__
    return out


def _helper_arguments(cls, helper):
    """string arguments of the ``_c("...")`` / ``_mg("...")`` calls in the methods ``cls`` ends up with (overrides win)"""
    import inspect
    names = set()
    for attr in dir(cls):
        a = inspect.getattr_static(cls, attr)
        for f in ([a.fget, a.fset] if isinstance(a, property) else [a]):
            if inspect.isfunction(f):
                names.update(re.findall(r"\._%s\(\"(\w+)\"\)" % helper, inspect.getsource(f)))
    return names


def test_binding_classes_keep_their_surface_and_resolve_only_declared_c_names():
    import inspect
    from ndr_amd import _lib
    from ndr_amd import pyVoxelFEM as pv
    # the tuned simulator gained P (the shared code is parameterised by it) and the _element_padding argument of the generic one
    tuned = dict(_SIM_SURFACE, **_SIM_TUNED_ONLY)
    assert _surface(pv.TensorProductSimulator1_1_1) == tuned
    for cls in (pv.TensorProductSimulator1_1, pv.TensorProductSimulator2_2, pv.TensorProductSimulator2_2_2):
        assert _surface(cls) == _SIM_SURFACE, cls
    for cls in (pv.TensorProductSimulator1_1_1, pv.TensorProductSimulator1_1, pv.TensorProductSimulator2_2, pv.TensorProductSimulator2_2_2):
        assert str(inspect.signature(cls.__init__)) == "(self, domainBoundingBox, numElemg, _element_padding=(0, 0))"
    assert (pv.TensorProductSimulator1_1_1.N, pv.TensorProductSimulator1_1_1.P) == (3, 1)
    assert [(c.N, c.P) for c in (pv.TensorProductSimulator1_1, pv.TensorProductSimulator2_2, pv.TensorProductSimulator2_2_2)] == \
        [(2, 1), (2, 2), (3, 2)]
    generic_mg = pv.TensorProductSimulator2_2_2._MG_CLASS
    assert pv.TensorProductSimulator1_1_1._MG_CLASS is pv.MultigridSolver1_1_1 is pv.detail.MultigridSolver1_1_1
    assert _surface(pv.MultigridSolver1_1_1) == dict(_MG_SURFACE, **_MG_TUNED_ONLY)
    assert _surface(generic_mg) == _MG_SURFACE
    for cls in (pv.MultigridSolver1_1_1, generic_mg):
        assert str(inspect.signature(cls.__init__)) == "(self, tps, numCoarseningLevels)"
    assert _surface(pv._LevelView) == _VIEW_SURFACE
    assert str(inspect.signature(pv._LevelView.__init__)) == "(self, mg, l)"

    # every C name the prefix helpers can build is declared: a name put together from strings fails only when it is called
    generic_sim = type("G111", (pv._GenericSimulator,), {"N": 3, "P": 1})
    for cls in (pv.TensorProductSimulator1_1_1, generic_sim, pv.TensorProductSimulator2_2):
        args = _helper_arguments(cls, "c")
        assert {"destroy", "set_densities", "get_densities", "apply_k"} <= args, sorted(args)      # the scan sees the methods
        for name in args:
            assert cls._SIM_PREFIX + name in _lib.SIGNATURES, (cls.__name__, name)
        assert cls._COMPLIANCE in _lib.SIGNATURES
    view_args = _helper_arguments(pv._LevelView, "mg")
    assert view_args == {"level_dims", "level_dirichlet_mask"}
    for cls in (pv.MultigridSolver1_1_1, generic_mg):
        args = _helper_arguments(cls, "mg")
        assert {"create", "destroy", "solve", "pcg"} <= args, sorted(args)
        for name in args | view_args:
            assert cls._MG_PREFIX + name in _lib.SIGNATURES, (cls.__name__, name)
    assert (pv.TensorProductSimulator1_1_1._SIM_PREFIX, pv._GenericSimulator._SIM_PREFIX) == ("vfem_sim_", "vfem_gsim_")
    assert (pv.MultigridSolver1_1_1._MG_PREFIX, generic_mg._MG_PREFIX) == ("vfem_mg_", "vfem_gmg_")
    # the helpers are only ever called with a literal, so the scan above sees every name
    src = open(os.path.join(ROOT, "ndr_amd", "pyVoxelFEM.py")).read()
    assert len(re.findall(r"\._c\(", src)) == len(re.findall(r"\._c\(\"\w+\"\)", src))
    assert len(re.findall(r"\._mg\(", src)) == len(re.findall(r"\._mg\(\"\w+\"\)", src))
    # users of the simulators' helper outside the module: the slab operator holds a tuned simulator, the knobs take either
    for path, prefixes in (("ndr_amd/distributed.py", ("vfem_sim_",)), ("tools/_knobs.py", ("vfem_sim_", "vfem_gsim_"))):
        names = re.findall(r"\._c\(\"(\w+)\"\)", open(os.path.join(ROOT, path)).read())
        assert names, path
        for name in names:
            for prefix in prefixes:
                assert prefix + name in _lib.SIGNATURES, (path, prefix + name)
