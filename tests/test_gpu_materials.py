"""-m gpu: orthotropic and anisotropic materials through every simulator, against the generic sparse-matrix oracle carrying the K0
of tests/material_ref.py (an independent Gauss-quadrature K0 for a general tensor, injected through the oracle's ``K0`` attribute).

Orthotropic tensors keep the structure of K0 that the tuned kernels assume, so they run the production kernels (all
``VFEM_PATH_*`` flags set); the anisotropic fixture (the orthotropic one turned by 30 degrees about z) has none of it and runs the
general kernels end to end.  Tolerances are those the isotropic tests of the same quantity use (imported where they have a name,
quoted with their source where they are literals there); the fixtures' moduli ratio <= 3 keeps the conditioning comparable.

Grids: 16x12x8 (coarsens twice), 9x10x20 (odd: cannot be coarsened, so it carries the level-0 checks and a hierarchy of one level,
whose cycle is the coarsest solve), 4x8x132 (rows of 133 nodes: multi-segment row kernels; level 1 has 67-node rows)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import material_ref as mr
from helpers import BC_BRIDGE, BC_CANTILEVER, ROOT, relerr
from test_gpu_mg_long_rows import TOL_SWEEP
from test_gpu_parity import TOL_OP

pytestmark = pytest.mark.gpu

TOL_K0 = 1e-13            # test_gpu_parity.test_k0_matches_oracle, test_gpu_generic.test_generic_simulator_matches_oracle
TOL_CYCLE = 1e-9          # test_gpu_parity.test_mg_solve_cycles, test_gpu_generic (one V-cycle / FMG cycle)
TOL_COARSEST = 1e-8       # test_gpu_parity.test_mg_operators (coarsest solve)
TOL_COMPLIANCE, TOL_U = 1e-8, 1e-6          # test_gpu_parity.test_pcg_matches_oracle (config 2)
H = (1.0, 0.7, 1.3)       # voxel edge lengths: a non-cubic box
BC2D = os.path.join(ROOT, "bcs", "2d", "mbb_beam.bc")
FILES = {(3, "orthotropic"): mr.ORTHO_3D, (3, "anisotropic"): mr.ANISO_3D, (2, "orthotropic"): mr.ORTHO_2D, (2, "anisotropic"): mr.ANISO_2D}
PATHS_ALL_SIM, PATH_L1, PATH_Q2 = 1 | 2 | 4, 8, 16                      # VFEM_PATH_* of include/vfem.h


def _dom(ne, h=H):
    return ([0.0] * len(ne), [float(n) * h[d] for d, n in enumerate(ne)])


def _rho(ne, seed=5):
    return np.random.default_rng(seed).uniform(0.1, 1.0, size=int(np.prod(ne)))


@functools.lru_cache(maxsize=None)
def _oracle(N, p, ne, bc, material, levels):
    """the generic oracle of one problem with material_ref's K0, built once and shared (tests leave it unchanged); with its
    hierarchy when ``levels`` is not None"""
    from oracle import generic_oracle as go
    o = go.GenericSim(N, p, _dom(ne), ne)
    mr.inject(o, mr.material_file_D(FILES[(N, material)]))
    o.Emin = 1e-4
    if bc:
        o.apply_bc_file(bc)
    o.rho = _rho(ne)
    om = None
    if levels is not None:
        om = go.GenericMG(o, levels)
        om.update_element_stiffness()
    return o, om


def _hip(N, p, ne, bc, material, h=H):
    from ndr_amd import pyVoxelFEM as pv
    dom = _dom(ne, h)
    t = pv.TensorProductSimulator([p] * N, [np.array(dom[0]), np.array(dom[1])], list(ne))
    if material is not None:
        t.readMaterial(FILES[(N, material)])
    if bc:
        t.applyDisplacementsAndLoadsFromFile(bc)
    t.E_0, t.E_min, t.gamma = 1.0, 1e-4, 3.0
    t.setElementDensities(_rho(ne))
    return t


def _opt(t, key, value):
    from ndr_amd import _lib
    _lib.check(t._c("set_option")(t._h, key, value))


def _check_level_operators(tmg, om, levels, N, rng, tol_op, tol_sweep, tol_transfer):
    """applyK, residual, forward and reverse sweeps, transfers of every level against the oracle hierarchy"""
    for l in range(levels + 1):
        n = om.sims[l].num_nodes
        u, b = rng.standard_normal((n, N)), rng.standard_normal((n, N))
        assert relerr(tmg.applyK(l, u), om.apply_k(l, u)) < tol_op, ("applyK", l)
        assert relerr(tmg.computeResidual(l, u, b), om.residual(l, u, b)) < tol_op, ("residual", l)
        if l < levels or levels == 0:
            u0 = om.zero_dirichlet(l, u.copy())
            for fwd in (True, False):
                us = u0.copy()
                om.smoothing(l, us, b, fwd)
                got = tmg.smoothing_device(l, u0, b, fwd).cpu().numpy()
                assert relerr(got, us) < tol_sweep, ("smoothing", l, fwd)
        if l < levels:
            assert relerr(tmg.restriction_device(l, u).cpu().numpy(), om.restriction(l, u)) < tol_transfer, ("restrict", l)
            c = rng.standard_normal((om.sims[l + 1].num_nodes, N))
            assert relerr(tmg.interpolation_device(l, c).cpu().numpy(), om.interpolation(l, c)) < tol_transfer, ("prolong", l)


def _check_cycles(tmg, om, f, levels):
    """one V-cycle and one full-multigrid cycle: the iterate, and the correction left on every coarser level"""
    for fmg in (False, True):
        xo = om.solve(np.zeros_like(f), f, 1, 2, True, False, fmg).copy()
        xg = tmg.solve(np.zeros_like(f), f, 1, 2, True, False, None, fmg)
        assert relerr(xg, xo) < TOL_CYCLE, ("cycle", fmg)
        if hasattr(tmg, "debug_get_x"):
            for l in range(1, levels + 1):
                assert relerr(tmg.debug_get_x(l), om.x[l]) < TOL_CYCLE, ("cycle", fmg, "level", l)


# ----------------------------------------------------------------------------------------------
# operators, trilinear
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", ["orthotropic", "anisotropic"])
@pytest.mark.parametrize("bc", [BC_CANTILEVER, BC_BRIDGE], ids=["cantilever", "bridge"])
@pytest.mark.parametrize("ne", [(16, 12, 8), (9, 10, 20), (4, 8, 132)], ids=lambda ne: "x".join(map(str, ne)))
def test_trilinear_operators_match_oracle(ne, bc, material):
    levels = 2 if all(n % 4 == 0 for n in ne) else 0
    o, om = _oracle(3, 1, ne, bc, material, levels)
    t = _hip(3, 1, ne, bc, material)
    D = mr.material_file_D(FILES[(3, material)])
    assert np.abs(t.ETensor.D - D).max() <= 1e-14 * np.abs(D).max()
    K0 = t.fullDensityElementStiffnessMatrix()
    assert relerr(K0, mr.reference_stiffness(D, H)) < TOL_K0
    assert np.array_equal(K0, K0.T)
    assert np.array_equal(t.dirichletMask, o.mask) and np.abs(t.buildLoadVector() - o.loads).max() < 1e-15
    want_paths = PATHS_ALL_SIM if material == "orthotropic" else 0
    assert t._tensor_paths() == want_paths
    rng = np.random.default_rng(1)
    u = rng.standard_normal((o.num_nodes, 3))
    ref = o.apply_k(u)
    for variant in (0, 1):                   # the path's own kernel and the gather kernel (one and the same for the anisotropic tensor)
        assert relerr(t.applyK_device(u, variant).cpu().numpy(), ref) < TOL_OP, ("applyK", variant)
    assert relerr(t.complianceGradient_device(u).cpu().numpy(), o.compliance_gradient(u)) < TOL_OP
    tmg = t.multigridSolver(levels)
    tmg.updateElementStiffnessMatrices()
    from ndr_amd import _lib
    assert _lib.load().vfem_mg_tensor_paths(tmg._h) == (want_paths | PATH_L1 if material == "orthotropic" else 0)
    for l in range(levels + 1):
        assert np.array_equal(tmg.getSimulator(l).dirichletMask, om.sims[l].mask), l
    _check_level_operators(tmg, om, levels, 3, rng, TOL_OP, TOL_SWEEP, TOL_OP)
    _check_cycles(tmg, om, o.loads.copy(), levels)
    bL = om.zero_dirichlet(levels, rng.standard_normal((om.sims[levels].num_nodes, 3)))
    assert relerr(tmg.coarsestSolve_device(bL).cpu().numpy(), om.coarsest_solve(bL)) < TOL_COARSEST


# ----------------------------------------------------------------------------------------------
# routing
# ----------------------------------------------------------------------------------------------

def test_tensor_paths_by_material():
    from ndr_amd import ElasticityTensor, _lib
    lib = _lib.load()
    ortho = ElasticityTensor(mr.ORTHO_3D)
    quarter = ortho.transform(np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]))
    aniso = ElasticityTensor(mr.ANISO_3D)
    for h in (H, (1.0, 1.0, 1.0), (2.0 / 256, 1.0 / 256, 1.0 / 256)):
        t = _hip(3, 1, (8, 4, 4), BC_CANTILEVER, None, h)
        for name, tensor, want in (("default", None, True), ("isotropic", ElasticityTensor(1.0, 0.3), True),
                                   ("isotropic through D", ElasticityTensor.fromD(ElasticityTensor(1.0, 0.3).D), True),
                                   ("orthotropic", ortho, True), ("quarter turn", quarter, True), ("anisotropic", aniso, False)):
            if tensor is not None:
                t.ETensor = tensor
                assert t.ETensor == tensor
            mg = t.multigridSolver(1)
            mg.updateElementStiffnessMatrices()
            assert t._tensor_paths() == (PATHS_ALL_SIM if want else 0), (h, name)
            assert lib.vfem_mg_tensor_paths(mg._h) == (PATHS_ALL_SIM | PATH_L1 if want else 0), (h, name)
    q = _hip(3, 2, (2, 2, 2), None, None)
    assert q._tensor_paths() == PATH_Q2
    q.ETensor = ortho
    assert q._tensor_paths() == PATH_Q2
    q.ETensor = aniso
    assert q._tensor_paths() == 0
    q.ETensor = ElasticityTensor(1.0, 0.3)
    assert q._tensor_paths() == PATH_Q2
    assert _hip(2, 1, (4, 4), None, "anisotropic")._tensor_paths() == 0
    with pytest.raises(RuntimeError, match="Dimension mismatch"):
        q.ETensor = ElasticityTensor(dim=2)
    bad = ElasticityTensor.fromD(np.diag([1.0, 1.0, 1.0, 1.0, 1.0, -1.0]))
    with pytest.raises(RuntimeError, match="not positive definite"):
        t.ETensor = bad
    assert t.ETensor == aniso                                   # a refused tensor changes nothing
    D = np.ascontiguousarray(aniso.D)
    D[0, 1] += 1e-3
    assert lib.vfem_sim_set_elasticity_tensor(t._h, D.ctypes.data_as(__import__("ctypes").c_void_p)) == 1
    assert "not symmetric" in lib.vfem_last_error().decode()


def test_orthotropic_cross_check_kernels_agree_with_the_defaults():
    """the tolerances of test_gpu_parity.test_tuning_and_cross_check_options_agree: 1e-13 between applies, 1e-12 between sweeps"""
    ne = (16, 12, 8)
    t = _hip(3, 1, ne, BC_CANTILEVER, "orthotropic")
    mg = t.multigridSolver(2)
    mg.updateElementStiffnessMatrices()
    g = torch.Generator(device="cuda").manual_seed(11)
    u = torch.randn((t.numNodes(), 3), dtype=torch.float64, device="cuda", generator=g)
    x = {l: torch.randn((mg._nn(l), 3), dtype=torch.float64, device="cuda", generator=g) for l in (0, 1)}
    b = {l: torch.randn((mg._nn(l), 3), dtype=torch.float64, device="cuda", generator=g) for l in (0, 1)}

    def close(a, r, tol, what):
        assert float((a - r).abs().max()) <= tol * float(r.abs().max()), what

    def sweeps(l):
        return [mg.smoothing_device(l, x[l], b[l], fwd).clone() for fwd in (True, False)]

    close(t.applyK_device(u, 1), t.applyK_device(u, 0), 1e-13, "gather apply")
    r0 = mg.computeResidual_device(0, x[0], b[0]).clone()
    _opt(t, 19, 0)                                              # VFEM_OPT_GS_MARCH: row kernels
    ref0 = sweeps(0)
    for key, value, back in ((2, 1, 0), (13, 0, 1), (19, 2, 0)):           # gather sweeps; coefficient table; marching sweep
        _opt(t, key, value)
        for got, r in zip(sweeps(0), ref0):
            close(got, r, 1e-12, ("level-0 sweep", key, value))
        _opt(t, key, back)
    _opt(t, 19, 1)
    ref1, a1 = sweeps(1), mg.applyK_device(1, x[1]).clone()
    _opt(t, 22, 0)                                              # VFEM_OPT_L1_MERGED: per incident element
    for got, r in zip(sweeps(1), ref1):
        close(got, r, 1e-12, "level-1 sweep per element")
    close(mg.applyK_device(1, x[1]), a1, 1e-12, "level-1 apply per element")
    _opt(t, 22, 2)
    close(mg.computeResidual_device(0, x[0], b[0]), r0, 1e-13, "residual unchanged by the sweep options")


def test_anisotropic_ignores_or_refuses_the_tuned_options():
    """every tuned option switched on: a flag that failed its check keeps the general kernel (results stay oracle-correct), and the
    entry points that have no general form raise their message"""
    from ndr_amd import _lib
    from ndr_amd.pyVoxelFEM import _ptr, _stream
    ne, bc = (16, 12, 8), BC_CANTILEVER
    o, om = _oracle(3, 1, ne, bc, "anisotropic", 2)
    t = _hip(3, 1, ne, bc, "anisotropic")
    mg = t.multigridSolver(2)
    rng = np.random.default_rng(3)
    # VFEM_OPT_*: 13 resident K0, 19 marching sweep, 22 level 1 per mirror class, 12 level-1 diagonal blocks, 21 level 1 stored as a
    # (half) stencil, 15 level-1 slot split, 4 apply implementation, 10 fused z colours, 2 gather sweeps
    for options in (((13, 1), (19, 2), (22, 2), (12, 1)), ((22, 1), (21, 1), (12, 0)), ((21, 2), (15, 2), (4, 1), (10, 0)),
                    ((21, 0), (2, 1), (4, 0))):
        for key, value in options:
            _opt(t, key, value)
        mg.updateElementStiffnessMatrices()
        assert t._tensor_paths() == 0 and not _lib.load().vfem_mg_can_smooth_planes(mg._h, 0)
        _check_level_operators(mg, om, 2, 3, rng, TOL_OP, TOL_SWEEP, TOL_OP)
    u = torch.randn((t.numNodes(), 3), dtype=torch.float64, device="cuda")
    out = torch.empty_like(u)
    with pytest.raises(RuntimeError, match="plane-range apply needs the mode-space kernel"):
        _lib.check(t._lib.vfem_sim_apply_k_planes(t._h, _ptr(u), _ptr(out), 1, 3, _stream()))
    with pytest.raises(RuntimeError, match="plane-range sweeps need the marching finest-level kernel"):
        _lib.check(t._lib.vfem_mg_smooth_group_planes(mg._h, 0, _ptr(u), _ptr(out), 1, 0, 1, 3, _stream()))


# ----------------------------------------------------------------------------------------------
# generic path
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", ["orthotropic", "anisotropic"])
@pytest.mark.parametrize("N,p,ne,bc,levels", [(2, 1, (12, 8), BC2D, 2), (2, 2, (12, 8), BC2D, 2), (3, 2, (4, 4, 6), BC_CANTILEVER, 1)],
                         ids=["2d-q1", "2d-q2", "3d-q2"])
def test_generic_path_matches_oracle(N, p, ne, bc, levels, material):
    """tolerances of test_gpu_generic: K0 1e-13, apply and gradient 1e-12, level operators 1e-11, sweeps 1e-10, transfers 1e-13,
    cycles 1e-9"""
    o, om = _oracle(N, p, ne, bc, material, levels)
    t = _hip(N, p, ne, bc, material, H[:N])
    D = mr.material_file_D(FILES[(N, material)])
    assert relerr(t.fullDensityElementStiffnessMatrix(), mr.reference_stiffness(D, H[:N], p)) < TOL_K0
    assert t._tensor_paths() == (PATH_Q2 if (N, p, material) == (3, 2, "orthotropic") else 0)
    assert np.array_equal(t.dirichletMask, o.mask)
    rng = np.random.default_rng(1)
    u = rng.standard_normal((o.num_nodes, N))
    assert relerr(t.applyK(u), o.apply_k(u)) < 1e-12
    assert relerr(t.complianceGradient_device(u).cpu().numpy(), o.compliance_gradient(u)) < 1e-12
    mg = t.multigridSolver(levels)
    mg.updateElementStiffnessMatrices()
    _check_level_operators(mg, om, levels, N, rng, 1e-11, 1e-10, 1e-13)
    _check_cycles(mg, om, o.loads.copy(), levels)
    if (N, p) == (3, 2):                     # the dense gather apply (VFEM_OPT_Q2_IMPL = 1) agrees with the path's own kernel
        a = t.applyK(u)
        _opt(t, 6, 1)
        assert relerr(t.applyK(u), a) < 1e-12
        _opt(t, 6, 0)


# ----------------------------------------------------------------------------------------------
# solves
# ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("material", ["orthotropic", "anisotropic"])
def test_pcg_matches_the_direct_solve_and_the_oracle_iteration_count(material):
    ne = (16, 8, 8)
    o, om = _oracle(3, 1, ne, BC_CANTILEVER, material, 2)
    t = _hip(3, 1, ne, BC_CANTILEVER, material)
    mg = t.multigridSolver(2)
    f = o.loads.copy()
    ud = o.solve(f)
    ug = mg.preconditionedConjugateGradient(np.zeros_like(f), f, 200, 1e-10, None, 1, 2, True)
    uo = om.pcg(np.zeros_like(f), f, 200, 1e-10, 1, 2, True)
    cd, cg = float((f * ud).sum()), float((f * ug).sum())
    print("%s: PCG iterations %d (oracle %d), compliance rel %.3e, u rel %.3e"
          % (material, mg.last_iterations, om.last_iters, abs(cg - cd) / abs(cd), relerr(ug, ud)))
    assert mg.last_relative_residual <= 1e-10 and mg.last_iterations < 200
    assert abs(cg - cd) < TOL_COMPLIANCE * abs(cd)
    assert relerr(ug, ud) < TOL_U
    if material == "orthotropic":
        assert mg.last_iterations == om.last_iters
    assert relerr(t.complianceGradient_device(ug).cpu().numpy(), o.compliance_gradient(ud)) < TOL_U


@pytest.mark.parametrize("material", ["orthotropic", "anisotropic"])
@pytest.mark.parametrize("N,ne,bc", [(2, (12, 8), BC2D), (3, (6, 4, 4), BC_CANTILEVER)], ids=["2d", "3d"])
def test_band_cholesky_solve_get_k_and_constant_strain_load(N, ne, bc, material):
    o, _ = _oracle(N, 1, ne, bc, material, None)
    t = _hip(N, 1, ne, bc, material, H[:N])
    t.directSolver = "cholesky"
    f = o.loads.copy()
    ud, ug = o.solve(f), t.solve(f)
    cd = float((f * ud).sum())
    assert t.numDirectFactorizations() == 1
    assert abs(float((f * ug).sum()) - cd) < TOL_COMPLIANCE * abs(cd) and relerr(ug, ud) < TOL_U
    # getK / elementStiffnessMatrix follow K0 (tolerances of test_gpu_parity.test_get_k_constant_strain_load_read_densities)
    A = o.assemble()
    assert abs(t.getK().full() - A).max() < 1e-13 * abs(A).max()
    assert relerr(t.elementStiffnessMatrix(3), o.young()[3] * o.K0) < TOL_K0
    # C : eps with the actual tensor, for an eps that is not symmetric (only its symmetric part can matter)
    eps = np.array([[0.3, 0.1, -0.2], [0.4, -0.5, 0.4], [-0.7, 0.1, 1.0]])[:N, :N]
    D = mr.material_file_D(FILES[(N, material)])
    want = mr.constant_strain_load(D, eps, H[:N], ne, o.rho)
    assert relerr(t.constantStrainLoad(eps), want) < 1e-13
    assert relerr(t.constantStrainLoad(0.5 * (eps + eps.T)), want) < 1e-13


def test_a_new_tensor_after_a_solve_rebuilds_the_operators():
    """bit for bit what a fresh simulator gives: the band factorisation, a hierarchy made before the change (it rebuilds its
    coarsened reference matrices) and the cached hierarchy of TPS::solve's stand-in"""
    from ndr_amd import ElasticityTensor
    ne = (16, 8, 8)
    o, _ = _oracle(3, 1, ne, BC_CANTILEVER, "anisotropic", None)
    f = o.loads.copy()
    ortho, aniso = ElasticityTensor(mr.ORTHO_3D), ElasticityTensor(mr.ANISO_3D)

    def run(t, mg):
        out = {}
        for mode in ("cholesky", "pcg"):
            t.directSolver = mode
            out[mode] = t.solve(f)
        out["mg"] = mg.preconditionedConjugateGradient(np.zeros_like(f), f, 50, 1e-9, None, 1, 2, True)
        out["l1"] = mg.applyK(1, np.ones((mg._nn(1), 3)) * np.arange(3))
        return out

    t = _hip(3, 1, ne, BC_CANTILEVER, "orthotropic")
    mg = t.multigridSolver(2)
    first = run(t, mg)
    t.ETensor = aniso
    changed = run(t, mg)
    fresh_t = _hip(3, 1, ne, BC_CANTILEVER, "anisotropic")
    fresh = run(fresh_t, fresh_t.multigridSolver(2))
    for k in fresh:
        assert np.array_equal(changed[k], fresh[k]), k
        assert not np.array_equal(changed[k], first[k]), k
    assert relerr(changed["cholesky"], o.solve(f)) < TOL_U
    t.ETensor = ortho                                           # and back: the flags return with the structure
    assert t._tensor_paths() == PATHS_ALL_SIM
    again = run(t, mg)
    for k in first:
        assert np.array_equal(again[k], first[k]), k


def test_isotropic_tensor_through_the_general_entry_point_equals_set_isotropic():
    from ndr_amd import ElasticityTensor
    ne = (9, 10, 20)
    a, b = _hip(3, 1, ne, None, None), _hip(3, 1, ne, None, None)
    a.ETensor = ElasticityTensor(1.0, 0.3)                                  # vfem_sim_set_isotropic
    b.ETensor = ElasticityTensor.fromD(ElasticityTensor(1.0, 0.3).D)        # vfem_sim_set_elasticity_tensor
    assert a._tensor_paths() == b._tensor_paths() == PATHS_ALL_SIM
    u = np.random.default_rng(2).standard_normal((a.numNodes(), 3))
    assert relerr(b.applyK(u), a.applyK(u)) < 1e-14
    assert relerr(b.fullDensityElementStiffnessMatrix(), a.fullDensityElementStiffnessMatrix()) < 1e-15
    # 2-D, plane stress, degree 2
    a2, b2 = _hip(2, 2, (5, 4), None, None, H[:2]), _hip(2, 2, (5, 4), None, None, H[:2])
    a2.ETensor = ElasticityTensor(1.0, 0.3, dim=2)
    b2.ETensor = ElasticityTensor.fromD(ElasticityTensor(1.0, 0.3, dim=2).D)
    u2 = np.random.default_rng(2).standard_normal((a2.numNodes(), 2))
    assert relerr(b2.applyK(u2), a2.applyK(u2)) < 1e-14


# ----------------------------------------------------------------------------------------------
# slabs
# ----------------------------------------------------------------------------------------------

def _slab_worker(rank, world, port, ne, levels, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    import material_ref as mr
    from helpers import BC_CANTILEVER, seeded_density
    from ndr_amd import ElasticityTensor, distributed as vd, pyVoxelFEM as pv
    dom = ([0.0, 0.0, 0.0], [2.0, 1.0, 1.0])
    refused = ""
    try:
        vd.DistributedMGSolver(ne, dom[0], dom[1], BC_CANTILEVER, mr.ANISO_3D, levels)
    except RuntimeError as e:
        refused = str(e)
    rho = torch.from_numpy(seeded_density(ne, 88)).cuda()
    ds = vd.DistributedMGSolver(ne, dom[0], dom[1], BC_CANTILEVER, ElasticityTensor(mr.ORTHO_3D), levels)
    ds.set_global_densities(rho)
    f = ds.local_loads()
    u = ds.pcg(torch.zeros_like(f), f, 100, 1e-8, 1, 2, True)
    comp = 2.0 * ds.compliance(f, u)
    t = pv.TensorProductSimulator([1, 1, 1], [np.array(dom[0]), np.array(dom[1])], list(ne))
    t.readMaterial(mr.ORTHO_3D)
    t.applyDisplacementsAndLoadsFromFile(BC_CANTILEVER)
    t.E_0, t.E_min, t.gamma = 1.0, 1e-4, 3.0
    t.setElementDensities(rho)
    mg = t.multigridSolver(levels)
    fg = t.buildLoadVector_device()
    ug = mg.preconditionedConjugateGradient_device(torch.zeros_like(fg), fg, 100, 1e-8, None, 1, 2, True)
    cg = float((fg * ug).sum())
    g = ds.geom[0]
    mine = u.view(g.n_planes, -1)[g.first_owned:g.last_owned + 1]
    want = ug.view(ne[0] + 1, -1)[ds.part.x0:ds.part.x1 + 1]
    err = float((mine - want).abs().max() / want.abs().max())
    q.put((rank, ds.Ld, ds.last_iterations, mg.last_iterations, comp, cg, err, refused, ds.lsim._tensor_paths()))
    dist.destroy_process_group()


def test_two_slab_ranks_solve_the_orthotropic_problem_and_refuse_the_anisotropic_one():
    """what test_gpu_distributed.test_distributed_pcg_matches_single_process asserts, for the orthotropic material"""
    import torch.multiprocessing as mp
    from helpers import collect_from_ranks, free_port
    world, ne, levels = 2, (32, 8, 8), 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_slab_worker, args=(r, world, port, ne, levels, q)) for r in range(world)]
    for p in procs:
        p.start()
    for rank, Ld, it_d, it_s, comp, cg, err, refused, paths in collect_from_ranks(q, procs):
        assert Ld >= 1
        assert it_d == it_s, (it_d, it_s)
        assert abs(comp - cg) < 1e-9 * abs(cg), (comp, cg)
        assert err < 1e-7, err
        assert "slab decomposition supports isotropic and grid-aligned orthotropic materials only" in refused
        assert paths == PATHS_ALL_SIM


def test_slab_rank_operator_takes_the_tensor_and_refuses_without_the_mirror_flags():
    from ndr_amd import ElasticityTensor, distributed as vd
    ne = (8, 6, 10)
    part = vd.SlabPartition(ne, 1, 0)
    ops = vd.HipLocalOps(part, [0, 0, 0], [8 * H[0], 6 * H[1], 10 * H[2]], tensor=ElasticityTensor(mr.ORTHO_3D), Emin=1e-4)
    ops.set_densities(torch.from_numpy(_rho(ne)).cuda())
    o, _ = _oracle(3, 1, ne, None, "orthotropic", None)
    u = np.random.default_rng(4).standard_normal((o.num_nodes, 3))
    ud = torch.from_numpy(u).cuda()
    assert relerr(ops.apply(ud).cpu().numpy(), o.apply_k(u)) < TOL_OP
    out = torch.full_like(ud, float("nan"))
    ops.apply_planes(ud, out, 2, 5)
    full = ops.apply(ud).view(ne[0] + 1, -1)
    assert torch.equal(out.view(ne[0] + 1, -1)[2:6], full[2:6])
    with pytest.raises(RuntimeError, match="slab decomposition supports isotropic and grid-aligned orthotropic materials only"):
        vd.HipLocalOps(part, [0, 0, 0], [8.0, 6.0, 10.0], tensor=ElasticityTensor(mr.ANISO_3D))
