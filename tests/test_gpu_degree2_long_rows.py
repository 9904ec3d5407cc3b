"""The degree-2 multigrid against the sparse-matrix oracle (oracle.generic_oracle.GenericSim / GenericMG: assembled K, P^T K P,
per-colour sparse rows) on grids that reach the kernels the production solves run.

tests/test_gpu_generic.py meets the oracle on (8, 4, 4) only, where
  - the finest sweep (launch_gs_sweep_q2_level0_nodes, kernels_q2.hip) never fills a wave of k_gs_q2_level0_rows, never gets a second
    wave along z or a second block of VFEM_Q2ROWS_WAVES rows along y, and never hands a row's tail (cnt_z > 64 with 1 to 16 nodes
    over a multiple of 64) to k_gs_q2_level0_nodes with a shifted start[2];
  - the virtual level 1 (k_q2_level1<1|2|3>, k_q2_level1_gs, VFEM_OPT_Q2_L1_VIRTUAL = 1) has blockIdx.x = 0 only: no lanes packed
    across a row end, no dead lanes in a last block, and the level-2 matrices built through it (coarsen_through_virtual_level1)
    meet only the stored path;
  - the axis-by-axis transfers (above 100 000 fine nodes) and the three degree-2 applies at their chunk seams meet only each other.
Every shape carries the claims it is there for; test_shapes_cover_every_branch (no GPU) recomputes them from the launcher's
arithmetic, restated here, and asserts that together they reach every branch.  A boundary condition that masks rows partway along z
(helpers.write_cut_bc) is used beside the cantilever's whole-plane one.

(33, 9, 70) of test_q2_apply_kernels_agree_across_chunk_seams is left to that test: the oracle's element-matrix array for it is 1.1 GB
on top of what the process already holds, and its seams (x-chunk, 63-element z-chunk) are those of (17, 6, 63) and (16, 5, 130).

An oracle pair is built once per (shape, boundary condition) by a module-scoped fixture, so at most one is alive; the module's peak
resident size is asserted below 4 GB when it ends."""
import os
import re
import resource

import numpy as np
import pytest

from helpers import BC_CANTILEVER, MATERIAL, ROOT, record_deltas, relerr, write_cut_bc

gpu = pytest.mark.gpu

TOL_APPLY, TOL_SWEEP, TOL_TRANSFER, TOL_CYCLE, TOL_SEAM = 1e-11, 1e-10, 1e-13, 1e-9, 1e-12
DOM = ([0, 0, 0], [2, 1, 1])
LEVELS = 2

# option keys of include/vfem.h
Q2_IMPL, Q2_L1_VIRTUAL, Q2_GS_IMPL, TRANSFER_AXIS = 6, 14, 16, 17
WAVE = 64                       # lanes of a wave: nodes of a z-row per wave of k_gs_q2_level0_rows, nodes per block of k_q2_level1_gs
L1_APPLY_BLOCK = 256            # nodes per block of k_q2_level1 (launch_apply_q2_level1, kernels_q2.hip: blk(64, 4, 1))
TRANSFER_AXIS_MIN_NODES = 100000          # gmg_restrict / gmg_prolong, generic.hip: axis by axis above this many fine nodes


def _kernel_literals():
    """VFEM_Q2ROWS_WAVES and the largest row tail handed to the gather kernel, from the text of kernels_q2.hip"""
    src = open(os.path.join(ROOT, "ndr_amd", "csrc", "kernels_q2.hip")).read()
    waves = re.findall(r"^#define\s+VFEM_Q2ROWS_WAVES\s+(\d+)", src, flags=re.M)
    tail = re.findall(r"const bool split = rows_in_lds && col\.cnt\[2\] > 64 && over >= 1 && over <= (\d+);", src)
    assert len(waves) == 1 and len(tail) == 1, (waves, tail)
    return int(waves[0]), int(tail[0])


# ---- the launchers' arithmetic, restated ----------------------------------------------------------------------------------------------
def colour_count(NN, l):
    """nodes of local index l along an axis of NN nodes (gs_colors.h): every 4th for an element-boundary node, every 2nd for a mid node"""
    stride = 2 if l == 1 else 4
    return 0 if l > NN - 1 else (NN - 1 - l) // stride + 1


def level_nodes(ne, l):
    return tuple(2 * (n // 2 ** l) + 1 for n in ne)


def level0_rows(ne, rows_waves, max_tail):
    """launch_gs_sweep_q2_level0_nodes with rows_in_lds: per z colour (cnt_z, over, split), per y colour the blocks of rows_waves rows"""
    _, NY, NZ = level_nodes(ne, 0)
    z = []
    for l in range(3):
        cnt = colour_count(NZ, l)
        over = cnt % WAVE
        z.append((cnt, over, cnt > WAVE and 1 <= over <= max_tail))
    return tuple(z), tuple(-(-colour_count(NY, l) // rows_waves) for l in range(3))


def level1_planes(ne):
    """level 1: the largest parity class of launch_apply_q2_level1 per x-plane, and (nodes per x-plane, row length) of the largest colour
    of launch_gs_sweep_q2_level1"""
    _, NY, NZ = level_nodes(ne, 1)
    cls = ((NY - 1) // 2 + 1) * ((NZ - 1) // 2 + 1)
    colour = max((colour_count(NY, ly) * colour_count(NZ, lz), colour_count(NZ, lz)) for ly in range(3) for lz in range(3))
    return cls, colour


# (fine grid, claims): "z" = (cnt_z, over, split) of the z colours 0, 1, 2 on level 0, "yblocks" = blocks of rows along y per y colour,
# "l1" = (largest parity class per plane, (nodes per plane, row length) of the largest colour) on level 1; two coarsening levels each
SHAPES = [
    ((4, 4, 128), {"z": ((65, 1, True), (128, 0, False), (64, 0, False)), "yblocks": (1, 1, 1), "l1": (195, (128, 64))}),
    ((4, 8, 132), {"z": ((67, 3, True), (132, 4, True), (66, 2, True)), "yblocks": (2, 2, 1), "l1": (335, (264, 66))}),
    ((4, 12, 160), {"z": ((81, 17, False), (160, 32, False), (80, 16, True)), "yblocks": (2, 3, 2), "l1": (567, (480, 80))}),
]
BCS = ("cut", "cantilever")
PAIRS = [(ne, bc) for ne, _ in SHAPES for bc in BCS]
PAIR_IDS = ["%s-%s" % ("x".join(map(str, ne)), bc) for ne, bc in PAIRS]


def check_claims(ne, claims):
    rows_waves, max_tail = _kernel_literals()
    z, yblocks = level0_rows(ne, rows_waves, max_tail)
    assert z == claims["z"] and yblocks == claims["yblocks"], (ne, z, yblocks)
    assert level1_planes(ne) == claims["l1"], (ne, level1_planes(ne))


def _partly_masked_rows(mask, nn):
    rows = np.asarray(mask).reshape(tuple(nn) + (3,)).any(axis=-1)
    return int((rows.any(axis=2) & ~rows.all(axis=2)).sum())


def _oracle_sim(ne, bc_path):
    from ndr_amd import pyVoxelFEM as pv
    from oracle import generic_oracle as go
    young, poisson = pv._read_isotropic_material(MATERIAL)
    o = go.GenericSim(3, 2, DOM, ne, young, poisson)
    o.Emin = 1e-4
    if bc_path:
        o.apply_bc_file(bc_path)
    return o


def test_shapes_cover_every_branch(tmp_path):
    _, max_tail = _kernel_literals()
    for ne, claims in SHAPES:
        check_claims(ne, claims)
        assert all(n % 2 ** LEVELS == 0 for n in ne)
    z = [c for _, claims in SHAPES for c in claims["z"]]
    # the finest sweep: the smallest and the largest tail handed to the gather kernel, the rows kernel alone on whole waves and with a
    # partial last wave, exactly one full wave, more than one block of rows along y
    assert any(split and over == 1 for _, over, split in z)
    assert any(split and over == max_tail for _, over, split in z)
    assert any(not split and over == 0 and cnt > WAVE for cnt, over, split in z)
    assert any(not split and over > max_tail and cnt > WAVE for cnt, over, split in z)
    assert any(cnt == WAVE for cnt, _, _ in z)
    assert any(split and 1 < over < max_tail for _, over, split in z)
    yb = [b for _, claims in SHAPES for b in claims["yblocks"]]
    assert {2, 3} <= set(yb)
    # level 1: a second block of the apply, several blocks of the sweep with a partial last one, blocks that straddle row ends
    l1 = [claims["l1"] for _, claims in SHAPES]
    assert any(cls > L1_APPLY_BLOCK for cls, _ in l1)
    assert any(cls > L1_APPLY_BLOCK and cls % L1_APPLY_BLOCK for cls, _ in l1)
    assert any(n > WAVE and n % WAVE and row % WAVE for _, (n, row) in l1)
    # the cutting boundary condition leaves rows partly masked on every level of every shape (the oracle's masks; the GPU test
    # test_dirichlet_masks_match_oracle asserts that the HIP hierarchy holds the same ones)
    from oracle import generic_oracle as go
    cut = write_cut_bc(tmp_path / "cut_rows.bc")
    for ne, _ in SHAPES:
        om = go.GenericMG(_oracle_sim(ne, cut), LEVELS)
        for l in range(LEVELS + 1):
            assert _partly_masked_rows(om.sims[l].mask, level_nodes(ne, l)) >= 1, (ne, l)


# ---- one oracle / HIP pair per (shape, boundary condition) ---------------------------------------------------------------------------
_RSS = {"gpu_ran": False}


@pytest.fixture(scope="module", autouse=True)
def _peak_memory_stays_bounded():
    """the module's peak resident size stays below 4 GB (a peak above it reached before the module started is not this module's)"""
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    yield
    after = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    if _RSS["gpu_ran"]:
        record_deltas("degree2_long_rows.peak_rss_gb", {"at_start": round(before / 2 ** 20, 2), "at_end": round(after / 2 ** 20, 2)})
    assert after < 4 * 2 ** 20 or after == before, (before, after)


@pytest.fixture(scope="module")
def cut_bc(tmp_path_factory):
    return write_cut_bc(tmp_path_factory.mktemp("bc") / "cut_rows.bc")


class Pair:
    def __init__(self, ne, bc, bc_path):
        from ndr_amd import pyVoxelFEM as pv
        from oracle import generic_oracle as go
        self.ne, self.bc = ne, bc
        self.name = "degree2_long_rows[%s-%s]" % ("x".join(map(str, ne)), bc)
        self.o = _oracle_sim(ne, bc_path)
        self.o.rho = np.random.default_rng(3).uniform(0.05, 1.0, size=self.o.num_elems)
        self.om = go.GenericMG(self.o, LEVELS)
        self.om.update_element_stiffness()
        self.t = pv.TensorProductSimulator([2, 2, 2], DOM, list(ne))
        self.t.readMaterial(MATERIAL)
        self.t.applyDisplacementsAndLoadsFromFile(bc_path)
        self.t.E_min = 1e-4
        self.t.setElementDensities(self.o.rho)
        self.mg = self.t.multigridSolver(LEVELS)
        self.mg.updateElementStiffnessMatrices()

    def option(self, key, value):
        from ndr_amd import _lib
        _lib.check(_lib.load().vfem_gsim_set_option(self.t._h, key, value))


@pytest.fixture(scope="module", params=PAIRS, ids=PAIR_IDS)
def pair(request, cut_bc):
    ne, bc = request.param
    _RSS["gpu_ran"] = True
    p = Pair(ne, bc, cut_bc if bc == "cut" else BC_CANTILEVER)
    yield p
    p.__dict__.clear()


class Deltas:
    """achieved errors of one test: printed and asserted one by one, written to the deltas file whatever the outcome"""

    def __init__(self, name):
        self.name, self.seen = name, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        record_deltas(self.name, self.seen)
        return False

    def check(self, key, got, ref, tol):
        got = got.cpu().numpy() if hasattr(got, "cpu") else got
        err = relerr(got, ref)
        self.seen[key] = err
        print("%s %s: %.3e (tolerance %.0e)" % (self.name, key, err, tol))
        assert err < tol, (self.name, key, err)


def _sweeps(d, p, l, x0, b, refs, what):
    for fwd in (True, False):
        d.check("%s sweep %s" % (what, "forward" if fwd else "backward"), p.mg.smoothing_device(l, x0, b, fwd), refs[fwd], TOL_SWEEP)


def _sweep_refs(p, l, x0, b):
    refs = {}
    for fwd in (True, False):
        refs[fwd] = x0.copy()
        p.om.smoothing(l, refs[fwd], b, fwd)
    return refs


def _transfers(d, p, l, rng, what):
    import torch
    nf, nc = p.om.sims[l].num_nodes, p.om.sims[l + 1].num_nodes
    r, c, base = rng.standard_normal((nf, 3)), rng.standard_normal((nc, 3)), rng.standard_normal((nf, 3))
    d.check(what + " restriction", p.mg.restriction_device(l, r), p.om.restriction(l, r), TOL_TRANSFER)
    pc = p.om.interpolation(l, c)
    d.check(what + " interpolation", p.mg.interpolation_device(l, c), pc, TOL_TRANSFER)
    d.check(what + " interpolation accumulated", p.mg.interpolation_device(l, c, out=torch.as_tensor(base, device="cuda").clone()), base + pc,
            TOL_TRANSFER)


@gpu
def test_dirichlet_masks_match_oracle(pair):
    check_claims(pair.ne, dict(SHAPES)[pair.ne])
    for l in range(LEVELS + 1):
        got = pair.mg.getSimulator(l).dirichletMask
        assert np.array_equal(got, pair.om.sims[l].mask), l
        assert np.asarray(got).any(), l
        if pair.bc == "cut":
            assert _partly_masked_rows(got, level_nodes(pair.ne, l)) >= 1, l


@gpu
def test_level0_operators_match_oracle(pair):
    """apply, residual, the three finest-level sweeps (VFEM_OPT_Q2_GS_IMPL 2: neighbour rows through LDS, whole waves, the row tails by
    the gather kernel; 1: the gather kernel; 0: element by element) and the transfers to level 1, each against the oracle"""
    p = pair                    # (the oracle is reached through the pair only: a failed test's traceback then keeps no oracle alive)
    rng = np.random.default_rng(4)
    v, b = rng.standard_normal((p.o.num_nodes, 3)), rng.standard_normal((p.o.num_nodes, 3))
    with Deltas(p.name + ".level0") as d:
        d.check("apply", p.mg.applyK_device(0, v), p.om.apply_k(0, v), TOL_APPLY)
        d.check("residual", p.mg.computeResidual_device(0, v, b), p.om.residual(0, v, b), TOL_APPLY)
        x0 = p.om.zero_dirichlet(0, v.copy())
        refs = _sweep_refs(p, 0, x0, b)
        try:
            for impl in (2, 1, 0):
                p.option(Q2_GS_IMPL, impl)
                _sweeps(d, p, 0, x0, b, refs, "impl %d" % impl)
        finally:
            p.option(Q2_GS_IMPL, 2)
        _transfers(d, p, 0, rng, "0 -> 1")


@gpu
def test_coarse_levels_match_oracle(pair):
    """levels 1 and 2 with level 1 virtual (VFEM_OPT_Q2_L1_VIRTUAL = 1: k_q2_level1, k_q2_level1_gs, level-2 matrices through
    coarsen_through_virtual_level1) and stored (0), each against the oracle's P^T K P"""
    p = pair
    rng = np.random.default_rng(5)
    with Deltas(p.name + ".coarse") as d:
        data = {}
        for l in (1, 2):
            n = p.om.sims[l].num_nodes
            v, b = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
            x0 = p.om.zero_dirichlet(l, v.copy())
            data[l] = (v, b, x0, p.om.apply_k(l, v), p.om.residual(l, v, b), _sweep_refs(p, l, x0, b))
        try:
            for mode in (1, 0):
                p.option(Q2_L1_VIRTUAL, mode)
                p.mg.updateElementStiffnessMatrices()
                for l in (1, 2):
                    v, b, x0, ref_apply, ref_res, refs = data[l]
                    what = "level %d, %s level 1:" % (l, "virtual" if mode else "stored")
                    d.check(what + " apply", p.mg.applyK_device(l, v), ref_apply, TOL_APPLY)
                    d.check(what + " residual", p.mg.computeResidual_device(l, v, b), ref_res, TOL_APPLY)
                    _sweeps(d, p, l, x0, b, refs, what)
        finally:
            p.option(Q2_L1_VIRTUAL, 2)
            p.mg.updateElementStiffnessMatrices()
        _transfers(d, p, 1, rng, "1 -> 2")


@gpu
def test_cycles_match_oracle(pair):
    """one V-cycle and one full-multigrid cycle of 2 + 2 sweeps under the default options"""
    p = pair
    p.mg.updateElementStiffnessMatrices()
    f = p.o.loads.copy()
    assert np.abs(f).max() > 0
    with Deltas(p.name + ".cycle") as d:
        for fmg in (False, True):
            xo = p.om.solve(np.zeros_like(f), f, 1, 2, True, False, fmg).copy()
            xg = p.mg.solve(np.zeros_like(f), f, 1, 2, True, False, None, fmg)
            d.check("full multigrid" if fmg else "V-cycle", xg, xo, TOL_CYCLE)


# ---- transfers above the axis-by-axis threshold ---------------------------------------------------------------------------------------
@gpu
def test_transfers_above_axis_threshold_match_oracle():
    """kg_restrict_axis / kg_prolong_axis (level 0: 41 x 41 x 65 = 109 265 nodes) and the single-pass kernels on the same level
    (VFEM_OPT_TRANSFER_AXIS = 0), both against the oracle's P; level 1 (14 553 nodes) takes the single pass either way"""
    import types
    from ndr_amd import _lib, pyVoxelFEM as pv
    from oracle import generic_oracle as go
    ne = (20, 20, 32)
    om = go.GenericMG(_oracle_sim(ne, None), LEVELS)
    t = pv.TensorProductSimulator([2, 2, 2], DOM, list(ne))
    t.readMaterial(MATERIAL)
    mg = t.multigridSolver(LEVELS)
    assert mg._nn(0) == om.sims[0].num_nodes and mg._nn(1) == om.sims[1].num_nodes
    assert mg._nn(0) > TRANSFER_AXIS_MIN_NODES >= mg._nn(1)
    with Deltas("degree2_long_rows.transfers[20x20x32]") as d:
        for mode in (1, 0):
            _lib.check(_lib.load().vfem_gsim_set_option(t._h, TRANSFER_AXIS, mode))
            for l in (0, 1):
                _transfers(d, types.SimpleNamespace(mg=mg, om=om), l, np.random.default_rng(21 + l), "axis %d, %d -> %d" % (mode, l, l + 1))


# ---- the three degree-2 applies and the gradient at the chunk seams -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ne", [(17, 6, 63), (16, 5, 130), (70, 3, 3)], ids=lambda ne: "x".join(map(str, ne)))
def test_q2_applies_at_chunk_seams_match_oracle(ne):
    """the marching (0), dense gather (1) and pencil (2) applies on the grids of test_q2_apply_kernels_agree_across_chunk_seams, each
    against the oracle's element loop, and k_gradient_q2 (four elements per block)"""
    from ndr_amd import _lib, pyVoxelFEM as pv
    from oracle import generic_oracle as go
    dom = ([0, 0, 0], [1.0, 0.7, 1.3])
    young, poisson = pv._read_isotropic_material(MATERIAL)
    o = go.GenericSim(3, 2, dom, ne, young, poisson)
    t = pv.TensorProductSimulator([2, 2, 2], dom, list(ne))
    t.readMaterial(MATERIAL)
    t.E_min = o.Emin = 1e-4
    o.rho = np.random.default_rng(11).uniform(0.05, 1.0, size=o.num_elems)
    t.setElementDensities(o.rho)
    u = np.random.default_rng(12).standard_normal((o.num_nodes, 3))
    ref = o.apply_k(u)
    with Deltas("degree2_long_rows.seams[%s]" % "x".join(map(str, ne))) as d:
        for impl in (0, 1, 2):
            _lib.check(_lib.load().vfem_gsim_set_option(t._h, Q2_IMPL, impl))
            d.check("apply impl %d" % impl, t.applyK_device(u), ref, TOL_SEAM)
        _lib.check(_lib.load().vfem_gsim_set_option(t._h, Q2_IMPL, 0))
        d.check("gradient", t.complianceGradient_device(u), o.compliance_gradient(u), TOL_SEAM)
