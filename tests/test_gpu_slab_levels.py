"""-m gpu: the kernels of a slab rank's multigrid hierarchy (vfem_mg_create_slab), one operation at a time, against the element-loop
oracle (oracle.vfem_oracle.OracleMG) and against the single-grid HIP hierarchy of the whole grid.

A multi-GPU solve runs every rank on a slab hierarchy that differs from the single-grid one in four values: the local node grid
starts at a ghost plane, the Gauss-Seidel colours follow the global x parity of local plane 0 (`xparity`), the transfers to the next
level start one fine plane earlier (`xshift` = -1), and the element arrays carry padding layers that level_E() (mg.hip) skips for the
on-the-fly level 1.  The multi-process solves of tests/test_gpu_distributed.py reach these values but assert a converged PCG, which
forgives a slightly wrong preconditioner.  Here `DistributedMGSolver(..., proxy=(world, rank))` builds ONE rank's slab in this process
(its degree-1 form; no message is ever sent) and every kernel is called through the C entry points the solver itself uses, on local
fields cut out of global seeded ones: the ghost planes hold the global values, as after a halo exchange.  Compared are the owned
planes [first_owned, last_owned] of the level written (ghost planes of an output belong to the exchange); every output lives in a
NaN-filled buffer with GUARD doubles on either side, which must still be NaN afterwards.

Shapes (test_geometry_claims, no GPU, pins them with SlabPartition / LevelGeom):
  A  24 x 4 x 260, rank 1 of 3, two coarsenings, one distributed: both ghosts, xparity 1 on levels 0 and 1, xshift -1, level-0 pads
     1/1, NZ = 261 / 131 (three level-0 pair segments per colour, one level-1 pair-row segment); cantilever and the row-cutting
     boundary condition (helpers.write_cut_bc);
  B  24 x 8 x 264, rank 1 of 3, three coarsenings, two distributed: level-0 pads 3/3, level-1 pads 1/1 (level_E with a non-zero
     ex_lo), level 2 a stored stencil with xparity 1 and rows of 67 nodes (past the 64-lane edge), level 3 the transfer target with
     xparity 0;
  C  the grid of B over two ranks: rank 0 (right ghost only, xparity 0, xshift 0) and rank 1 (left ghost only, the last rank).
z is never shortened: the segment arithmetic of the row kernels needs it.

What a slab does NOT reach at these shapes, and why it is not claimed: a slab hierarchy never stores level 1 (update_operators,
mg.hip: `!mg->slab`), so VFEM_OPT_L1_STORED leaves the slab on the on-the-fly kernels -- the test asserts exactly that (bit for bit
the result of L1_STORED = 0) while the single-grid side runs the stored forms; and level 2 of B has 1005 nodes, below
WAVE_SWEEP_MAX_NODES, so it runs k_gs_color_stencil_wave whatever VFEM_OPT_STENCIL_SPLIT says.

References.  Oracle: everything, at TOL_OP = 1e-11 (operators, transfers, element matrices) and TOL_SWEEP = 1e-10 (sweeps), the bounds
of tests/test_gpu_parity.py and tests/test_gpu_mg_long_rows.py.  The exported element matrices are compared with the x-slice of the
level-T Galerkin matrices the oracle hierarchy holds after update_element_stiffness (OracleSim.Ke, one 24 x 24 block per element).
Single-grid HIP: the same bounds, except where the kernel shows that a node's sum cannot depend on NX or the plane offset, where
torch.equal is asserted:
  - k_restrict sums a coarse node over its fine planes di = -1, 0, 1, rows dj = -1, 0, 1 and nodes 2k-1, 2k, 2k+1 with explicit
    fma in that order, for the first and the second coarse plane of a wave alike; a plane outside the grid is skipped, never
    reordered;
  - k_prolong_rows sums a fine node over its (up to) four coarse rows t = 0..3 with explicit fma, whatever the shift;
  - k_coarsen_ke / k_coarsen_ke_two_levels give one block (or one slot of a block) to a coarse element and read its children only.
The sweeps and operators of a slab may run another kernel than the single grid (the apply of level 0 tiles by NX), so they keep the
tolerance.  The partial (one colour group) sweeps have no oracle; the composed sweep ties them to it.

Measured on an MI355X (largest relative error over all cases; stored by helpers.record_deltas under slab_levels/).  Slab against the
oracle: apply 9.8e-16, residual 1.1e-15 / 6.0e-16 / 8.8e-16 on levels 0 / 1 / 2, restriction and both interpolations 0.0, composed
sweeps 9.0e-16 / 1.2e-15 / 3.0e-15 on levels 0 / 1 / 2 (the single grid: 6.6e-16 / 1.1e-15 / 3.0e-15), marching sweep by plane ranges
3.3e-16, exported element matrices 2.0e-15 (level 2) and 3.3e-15 (level 3).  Slab against the single grid: 0.0 for every operation
and every colour group on the same kernels; 4.0e-16 per colour group where the single grid runs level 1 from a stored stencil.  The
31 GPU tests of the file take 3.8 s together, the slowest (the first, which builds the hierarchies of A) 0.8 s.
With `lv.xparity = 0` in vfem_mg_create_slab the sweep, plane-range and variant tests fail (16), with `lv.xshift = 0` the transfer
tests of every slab with a left ghost (4), without the ex_lo term of level_E the level-1 residual, sweep and variant tests of B and
C1 (10).
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import (BC_CANTILEVER, MATERIAL, l0_pair_segments, l1_pair_segments, level_nodes, make_hip, make_oracle, record_deltas,
                     relerr, seeded_density, write_cut_bc)

gpu = pytest.mark.gpu

TOL_SWEEP, TOL_OP = 1e-10, 1e-11
DOM = ([0.0, 0.0, 0.0], [2.0, 1.0, 1.0])
GUARD = 64                               # NaN doubles on either side of an output (512 bytes: the field keeps its alignment)

# option keys of include/vfem.h and their defaults (vfem_internal.h, Tuning)
GS_PAIR, GS_RESIDENT, STENCIL_SPLIT, GS_MARCH, L1_STORED, L1_MERGED = 10, 13, 18, 19, 21, 22
DEFAULTS = {GS_PAIR: 1, GS_RESIDENT: 1, STENCIL_SPLIT: 1, GS_MARCH: 1, L1_STORED: 0, L1_MERGED: 2}
WAVE_SWEEP_MAX_NODES = 40000             # ndr_amd/csrc/vfem_internal.h

# name -> (grid, world, rank, coarsenings L, distributed coarsenings Ld)
CASES = {
    "A": ((24, 4, 260), 3, 1, 2, 1),
    "B": ((24, 8, 264), 3, 1, 3, 2),
    "C0": ((24, 8, 264), 2, 0, 3, 2),
    "C1": ((24, 8, 264), 2, 1, 3, 2),
}
# per level: (node planes, first_owned, last_owned, xshift, xparity, (pad lo, pad hi), NZ)
GEOMETRY = {
    "A": [(11, 1, 9, 0, 1, (1, 1), 261), (7, 1, 5, -1, 1, (0, 0), 131), (5, 1, 3, -1, 1, (0, 0), 66)],
    "B": [(11, 1, 9, 0, 1, (3, 3), 265), (7, 1, 5, -1, 1, (1, 1), 133), (5, 1, 3, -1, 1, (0, 0), 67), (4, 1, 2, -1, 0, (0, 0), 34)],
    "C0": [(18, 0, 16, 0, 0, (0, 3), 265), (10, 0, 8, 0, 0, (0, 1), 133), (6, 0, 4, 0, 0, (0, 0), 67), (4, 0, 2, 0, 0, (0, 0), 34)],
    "C1": [(10, 1, 9, 0, 1, (3, 0), 265), (6, 1, 5, -1, 1, (1, 0), 133), (4, 1, 3, -1, 1, (0, 0), 67), (3, 1, 2, -1, 1, (0, 0), 34)],
}
# (case, boundary condition) of the slabs under test
SLABS = [("A", "cantilever"), ("A", "cut"), ("B", "cantilever"), ("C0", "cantilever"), ("C1", "cantilever")]
SLAB_IDS = ["%s-%s" % s for s in SLABS]


def _geoms(name):
    from ndr_amd.distributed import LevelGeom, SlabPartition
    ne, world, rank, L, Ld = CASES[name]
    part = SlabPartition(ne, world, rank, align=2 ** (Ld + 1))
    return [LevelGeom(part, l, Ld, ne) for l in range(Ld + 2)]


def test_geometry_claims():
    """no GPU: the shapes reach what the docstring says, so that a later change of shape cannot drop coverage silently"""
    seen = {"xparity": set(), "xshift": set(), "l1_ex_lo": set(), "ghosts": set()}
    for name, (ne, world, rank, L, Ld) in CASES.items():
        gs = _geoms(name)
        assert len(gs) == len(GEOMETRY[name]) == Ld + 2 <= L + 1, name
        for l, (g, claim) in enumerate(zip(gs, GEOMETRY[name])):
            got = (g.n_planes, g.first_owned, g.last_owned, g.xshift, g.xparity, (g.extra_lo, g.extra_hi), g.nz + 1)
            assert got == claim, (name, l, got)
            assert g.nz + 1 == level_nodes(ne, l)[2] and g.plane == level_nodes(ne, l)[1] * level_nodes(ne, l)[2]
            assert g.xparity == (g.xoffn & 1)
            if l <= Ld:
                seen["xparity"].add(g.xparity)
            if l >= 1:
                seen["xshift"].add(g.xshift)
        seen["l1_ex_lo"].add(gs[1].extra_lo > 0)
        seen["ghosts"].add((bool(gs[0].gl), bool(gs[0].gr)))
    # A and B: interior rank, xparity 1 on every swept level, one fine plane of shift on every coarse level
    for name in ("A", "B"):
        gs = _geoms(name)
        Ld = CASES[name][4]
        assert (gs[0].gl, gs[0].gr) == (1, 1)
        assert all(g.xparity == 1 for g in gs[:Ld + 1]) and all(g.xshift == -1 for g in gs[1:])
    assert GEOMETRY["A"][0][5] == (1, 1) and GEOMETRY["B"][0][5] == (3, 3) and GEOMETRY["B"][1][5] == (1, 1)
    assert GEOMETRY["B"][3][4] == 0                                     # the transfer target of B sits on an even plane
    # the row kernels' branches: several level-0 pair segments (nA >= 2), whole level-1 pair-row segments (nseg >= 1), a stencil row
    # past the 64-lane edge on a level small enough for the wave-per-node sweep
    for name in ("A", "B"):
        NZ0, NZ1 = GEOMETRY[name][0][6], GEOMETRY[name][1][6]
        for fwd in (True, False):
            assert l0_pair_segments(NZ0, fwd)[0] >= 2 and l1_pair_segments(NZ1, fwd)[0] >= 1, (name, fwd)
    assert l0_pair_segments(265, True) == (3, 3) and l0_pair_segments(265, False) == (3, 3)
    assert l1_pair_segments(133, True) == (1, 3, 2) and l1_pair_segments(133, False) == (1, 2, 3)
    gB2 = _geoms("B")[2]
    assert gB2.nz + 1 == 67 > 64 and gB2.n_planes * gB2.plane <= WAVE_SWEEP_MAX_NODES
    # together
    assert seen["xparity"] == {0, 1} and seen["xshift"] == {0, -1} and seen["l1_ex_lo"] == {False, True}
    assert seen["ghosts"] == {(True, True), (False, True), (True, False)}


# ---- the three hierarchies of a case, built once ------------------------------------------------------------------------------------
_ptr = lambda t: ctypes.c_void_p(t.data_ptr())
_stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(status):
    from ndr_amd import _lib
    _lib.check(status)


class Ref:
    """the whole grid: the oracle hierarchy and the single-grid HIP hierarchy, with global seeded fields per level"""

    def __init__(self, ne, bc, L):
        from oracle import vfem_oracle as vo
        self.ne, self.L = ne, L
        self.rho = seeded_density(ne, 88)
        self.o, self.t = make_oracle(ne, DOM, bc, self.rho), make_hip(ne, DOM, bc, self.rho)
        self.omg = vo.OracleMG(self.o, L, nthreads=4)
        self.omg.update_element_stiffness()
        self.tmg = self.t.multigridSolver(L)
        self.tmg.updateElementStiffnessMatrices()
        self._fields, self._sweeps = {}, {}

    def field(self, l, seed, zero_dirichlet=False):
        """global seeded field of level l (never modified: callers copy)"""
        key = (l, seed, zero_dirichlet)
        if key not in self._fields:
            u = np.random.default_rng(1000 * seed + l).standard_normal((self.omg.sims[l].num_nodes, 3))
            if zero_dirichlet:
                self.omg.enforce_dirichlet(l, u, True)
            self._fields[key] = u
        return self._fields[key]

    def oracle_sweep(self, l, forward):
        if (l, forward) not in self._sweeps:
            u = self.field(l, 3, True).copy()
            self.omg.smoothing(l, u, self.field(l, 4), forward)
            self._sweeps[(l, forward)] = u
        return self._sweeps[(l, forward)]


class Slab:
    """one rank's local simulator and slab hierarchy through the proxy"""

    def __init__(self, name, bc, ref):
        from ndr_amd.distributed import DistributedMGSolver
        ne, world, rank, L, Ld = CASES[name]
        self.name, self.ref = name, ref
        self.ds = ds = DistributedMGSolver(ne, DOM[0], DOM[1], bc, MATERIAL, L, dist_levels=Ld, proxy=(world, rank))
        ds.set_global_densities(torch.as_tensor(ref.rho, device="cuda"))
        ds.update_operators()
        self.lib, self.lmg, self.geom, self.Ld, self.T = ds.lib, ds.lmg, ds.geom, ds.Ld, ds.T

    def cut(self, l, glob):
        """the local planes of a global level-l field (numpy or device), flat [n_planes * plane, 3]"""
        g = self.geom[l]
        return glob.reshape(-1, g.plane * 3)[g.xoffn:g.xoffn + g.n_planes].reshape(-1, 3)

    def dev(self, l, glob):
        return torch.as_tensor(np.ascontiguousarray(self.cut(l, glob)), device="cuda")

    def owned(self, l, local):
        g = self.geom[l]
        v = local.reshape(g.n_planes, -1)[g.first_owned:g.last_owned + 1]
        return v.cpu().numpy() if isinstance(v, torch.Tensor) else v

    def out(self, l, init=None):
        """(parent, field): a NaN-filled buffer with the level-l local field inside, GUARD doubles away from either end"""
        g = self.geom[l]
        n = g.n_planes * g.plane * 3
        parent = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        f = parent[GUARD:GUARD + n].view(-1, 3)
        if init is not None:
            f.copy_(init)
        return parent, f


def guards_intact(parent):
    return bool(torch.isnan(parent[:GUARD]).all() and torch.isnan(parent[-GUARD:]).all())


_cache = {}


@pytest.fixture(scope="module")
def bcs(tmp_path_factory):
    return {"cantilever": BC_CANTILEVER, "cut": write_cut_bc(tmp_path_factory.mktemp("bc") / "cut_rows.bc")}


def _ref(name, bc, bcs):
    ne, _, _, L, _ = CASES[name]
    key = ("ref", ne, bc, L)
    if key not in _cache:
        _cache[key] = Ref(ne, bcs[bc], L)
    return _cache[key]


def _slab(name, bc, bcs):
    key = ("slab", name, bc)
    if key not in _cache:
        _cache[key] = Slab(name, bcs[bc], _ref(name, bc, bcs))
    return _cache[key]


_deltas = {}


def _record(test, what, value):
    _deltas.setdefault(test, {})[what] = max(float(value), _deltas.get(test, {}).get(what, 0.0))
    record_deltas("slab_levels/" + test, {k: float("%.3g" % v) for k, v in _deltas[test].items()})


def _opt(sim, key, value):
    _chk(sim._lib.vfem_sim_set_option(sim._h, key, value))


def _set_options(slab, options):
    """on the slab's simulator and on the single-grid one, then the operators that depend on them"""
    for sim in (slab.ds.lsim, slab.ref.t):
        for key, value in options.items():
            _opt(sim, key, value)
    slab.ds.update_operators()
    slab.ref.tmg.updateElementStiffnessMatrices()


# ---- 1. apply and residual -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,bc", SLABS, ids=SLAB_IDS)
def test_apply_and_residual(name, bc, bcs):
    s = _slab(name, bc, bcs)
    ref, lib = s.ref, s.lib
    what = "%s-%s" % (name, bc)
    for l in range(s.Ld + 1):
        u, b = ref.field(l, 1), ref.field(l, 2)
        ul, bl = s.dev(l, u), s.dev(l, b)
        if l == 0:
            parent, out = s.out(0)
            _chk(lib.vfem_mg_apply_k(s.lmg, 0, _ptr(ul), _ptr(out), _stream()))
            eo = relerr(s.owned(0, out), s.owned(0, s.cut(0, ref.omg.apply_k(0, u))))
            eh = relerr(s.owned(0, out), s.owned(0, s.cut(0, ref.tmg.applyK(0, u))))
            print("apply_k level 0 %s: slab - oracle %.3g, slab - single grid %.3g" % (what, eo, eh))
            _record("apply_residual", "apply_l0_vs_oracle", eo)
            _record("apply_residual", "apply_l0_vs_single_grid", eh)
            assert eo < TOL_OP and eh < TOL_OP, (what, eo, eh)
            assert guards_intact(parent), what
        parent, out = s.out(l)
        _chk(lib.vfem_mg_residual(s.lmg, l, _ptr(ul), _ptr(bl), _ptr(out), _stream()))
        eo = relerr(s.owned(l, out), s.owned(l, s.cut(l, ref.omg.residual(l, u.copy(), b))))
        eh = relerr(s.owned(l, out), s.owned(l, s.cut(l, ref.tmg.computeResidual(l, u, b))))
        print("residual level %d %s: slab - oracle %.3g, slab - single grid %.3g" % (l, what, eo, eh))
        _record("apply_residual", "residual_l%d_vs_oracle" % l, eo)
        _record("apply_residual", "residual_l%d_vs_single_grid" % l, eh)
        assert eo < TOL_OP and eh < TOL_OP, (what, l, eo, eh)
        assert guards_intact(parent), (what, l)


# ---- 2. transfers --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,bc", SLABS, ids=SLAB_IDS)
def test_transfers(name, bc, bcs):
    """restriction and both interpolations of every distributed level, level T = Ld + 1 being the target of the last; bit for bit the
    single grid's values (module docstring)"""
    s = _slab(name, bc, bcs)
    ref, lib = s.ref, s.lib
    what = "%s-%s" % (name, bc)
    for l in range(s.Ld + 1):
        fine, coarse, base = ref.field(l, 5), ref.field(l + 1, 6), ref.field(l, 7)
        # restriction: fine level l -> coarse level l + 1
        parent, out = s.out(l + 1)
        _chk(lib.vfem_mg_restrict(s.lmg, l, _ptr(s.dev(l, fine)), _ptr(out), _stream()))
        eo = relerr(s.owned(l + 1, out), s.owned(l + 1, s.cut(l + 1, ref.omg.restriction(l, fine))))
        single = ref.tmg.restriction_device(l, fine)
        print("restrict %d -> %d %s: slab - oracle %.3g" % (l, l + 1, what, eo))
        _record("transfers", "restrict_vs_oracle", eo)
        assert eo < TOL_OP, (what, l, eo)
        assert np.array_equal(s.owned(l + 1, out), s.owned(l + 1, s.cut(l + 1, single))), (what, l)
        assert guards_intact(parent), (what, l)
        # interpolation: coarse level l + 1 -> fine level l, overwriting and accumulating
        cl = s.dev(l + 1, coarse)
        for acc in (0, 1):
            parent, out = s.out(l, s.dev(l, base) if acc else None)
            _chk(lib.vfem_mg_interpolate(s.lmg, l, _ptr(cl), _ptr(out), acc, _stream()))
            want = ref.omg.interpolation(l, coarse, out=base.copy() if acc else None, accumulate=bool(acc))
            single = ref.tmg.interpolation_device(l, coarse, out=torch.as_tensor(base, device="cuda").clone() if acc else None)
            eo = relerr(s.owned(l, out), s.owned(l, s.cut(l, want)))
            print("interpolate %d -> %d accumulate %d %s: slab - oracle %.3g" % (l + 1, l, acc, what, eo))
            _record("transfers", "interpolate_acc%d_vs_oracle" % acc, eo)
            assert eo < TOL_OP, (what, l, acc, eo)
            assert np.array_equal(s.owned(l, out), s.owned(l, s.cut(l, single))), (what, l, acc)
            assert guards_intact(parent), (what, l, acc)


# ---- 3. sweeps, colour group by colour group -----------------------------------------------------------------------------------------
def _sweep_by_groups(s, l, forward, what, test):
    """one sweep of level l as two colour groups with the halo exchange emulated between them; returns the slab's local field after
    the first group, before the exchange"""
    ref, lib, g = s.ref, s.lib, s.geom[l]
    u0, b = ref.field(l, 3, True), ref.field(l, 4)
    ug, bg = torch.as_tensor(u0, device="cuda").clone(), torch.as_tensor(b, device="cuda")
    parent, ul = s.out(l, s.dev(l, u0))
    bl = s.dev(l, b)
    pl = ul.view(g.n_planes, -1)
    free = ~s.cut(l, ref.omg.sims[l].dmask != 0).reshape(g.n_planes, -1).all(axis=1)      # planes with something to relax
    after_first = None
    for group in (0, 1):
        cx = group if forward else 1 - group                            # global x parity of the planes this group relaxes
        before = pl.clone()
        _chk(lib.vfem_mg_smooth_colors(ref.tmg._h, l, _ptr(ug), _ptr(bg), int(forward), 4 * group, 4, _stream()))
        _chk(lib.vfem_mg_smooth_colors(s.lmg, l, _ptr(ul), _ptr(bl), int(forward), 4 * group, 4, _stream()))
        sg = s.cut(l, ug).view(g.n_planes, -1)
        err = relerr(s.owned(l, ul), s.owned(l, sg))
        print("sweep level %d %s group %d %s: slab - single grid %.3g" % (l, "forward" if forward else "backward", group, what, err))
        _record(test, "group_l%d_vs_single_grid" % l, err)
        assert err < TOL_SWEEP, (what, l, forward, group, err)
        relaxed = [p for p in range(g.n_planes) if ((g.xoffn + p) & 1) == cx]
        for p in range(g.n_planes):
            if p not in relaxed:
                assert torch.equal(pl[p], before[p]), (what, l, forward, group, "plane of the other parity changed", p)
        for p in relaxed:
            if g.first_owned <= p <= g.last_owned and free[p]:
                assert not torch.equal(pl[p], before[p]), (what, l, forward, group, "plane not relaxed", p)
        if group == 0:
            after_first = ul.clone()
        pl[:g.first_owned] = sg[:g.first_owned]                         # the halo exchange
        pl[g.last_owned + 1:] = sg[g.last_owned + 1:]
        assert guards_intact(parent), (what, l, forward, group)
    want = ref.oracle_sweep(l, forward)
    eo = relerr(s.owned(l, ul), s.owned(l, s.cut(l, want)))
    es = relerr(ug.cpu().numpy(), want)
    print("sweep level %d %s %s: slab - oracle %.3g (single grid - oracle %.3g)" % (l, "forward" if forward else "backward", what, eo, es))
    _record(test, "sweep_l%d_vs_oracle" % l, eo)
    assert eo < TOL_SWEEP, (what, l, forward, eo)
    return after_first


@gpu
@pytest.mark.parametrize("name,bc", SLABS, ids=SLAB_IDS)
def test_sweeps_group_by_group(name, bc, bcs):
    s = _slab(name, bc, bcs)
    assert s.lib.vfem_mg_can_smooth_planes(s.lmg, 0) == 0               # small grids: the row kernels (the marching sweep: below)
    for l in range(s.Ld + 1):
        for forward in (True, False):
            _sweep_by_groups(s, l, forward, "%s-%s" % (name, bc), "sweeps")


# ---- 4. plane-range sweeps of the marching kernel ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("bc", ["cantilever", "cut"])
def test_plane_range_sweeps(bc, bcs):
    """vfem_mg_smooth_group_planes in the order DistributedMGSolver.smooth uses (the plane a neighbour waits for on either side, then
    the planes between), then the two outermost owned planes, which the group of the other parity relaxes: five disjoint ranges that
    cover [first_owned, last_owned].  Planes of one parity do not read each other, so the result is that of one call, bit for bit."""
    s = _slab("A", bc, bcs)
    ref, lib, g = s.ref, s.lib, s.geom[0]
    what = "A-%s" % bc
    fo, lo = g.first_owned, g.last_owned
    ranges = [(fo + 1, fo + 1), (lo - 1, lo - 1), (fo + 2, lo - 2), (fo, fo), (lo, lo)]
    assert sorted(p for a, c in ranges for p in range(a, c + 1)) == list(range(fo, lo + 1))
    try:
        _set_options(s, {GS_MARCH: 2})
        assert lib.vfem_mg_can_smooth_planes(s.lmg, 0) == 1
        assert lib.vfem_mg_can_smooth_planes(ref.tmg._h, 0) == 1
        u0, b = ref.field(0, 3, True), ref.field(0, 4)
        bg, bl = torch.as_tensor(b, device="cuda"), s.dev(0, b)
        for forward in (True, False):
            ug = torch.as_tensor(u0, device="cuda").clone()
            pa, ua = s.out(0, s.dev(0, u0))                             # range by range
            pb, ub = s.out(0, s.dev(0, u0))                             # one call over the owned planes
            va, vb = ua.view(g.n_planes, -1), ub.view(g.n_planes, -1)
            for group in (0, 1):
                cx = group if forward else 1 - group
                _chk(lib.vfem_mg_smooth_colors(ref.tmg._h, 0, _ptr(ug), _ptr(bg), int(forward), 4 * group, 4, _stream()))
                start = va.clone()
                for a, c in ranges:
                    before = va.clone()
                    _chk(lib.vfem_mg_smooth_group_planes(s.lmg, 0, _ptr(ua), _ptr(bl), int(forward), group, a, c, _stream()))
                    for p in range(g.n_planes):
                        if not (a <= p <= c and ((g.xoffn + p) & 1) == cx):
                            assert torch.equal(va[p], before[p]), (what, forward, group, (a, c), "plane outside the range changed", p)
                _chk(lib.vfem_mg_smooth_group_planes(s.lmg, 0, _ptr(ub), _ptr(bl), int(forward), group, fo, lo, _stream()))
                assert torch.equal(ua, ub), (what, forward, group)
                for p in range(g.n_planes):
                    inside = fo <= p <= lo and ((g.xoffn + p) & 1) == cx
                    assert torch.equal(vb[p], start[p]) != inside, (what, forward, group, p)
                sg = s.cut(0, ug).view(g.n_planes, -1)
                err = relerr(s.owned(0, ua), s.owned(0, sg))
                print("marching sweep %s group %d %s: slab - single grid %.3g" % ("forward" if forward else "backward", group, what, err))
                _record("plane_ranges", "group_vs_single_grid", err)
                assert err < TOL_SWEEP, (what, forward, group, err)
                for v in (va, vb):                                      # the halo exchange
                    v[:fo] = sg[:fo]
                    v[lo + 1:] = sg[lo + 1:]
                assert guards_intact(pa) and guards_intact(pb), (what, forward, group)
            eo = relerr(s.owned(0, ua), s.owned(0, s.cut(0, ref.oracle_sweep(0, forward))))
            print("marching sweep %s %s: slab - oracle %.3g" % ("forward" if forward else "backward", what, eo))
            _record("plane_ranges", "sweep_vs_oracle", eo)
            assert eo < TOL_SWEEP, (what, forward, eo)
    finally:
        _set_options(s, DEFAULTS)


# ---- 5. kernel variants under xparity = 1 --------------------------------------------------------------------------------------------
# (options, level they affect, what the launcher does with them on the slab of B)
VARIANTS = [
    ({GS_PAIR: 1, GS_RESIDENT: 1}, 0, "l0_pair"), ({GS_PAIR: 1, GS_RESIDENT: 0}, 0, "l0_pair"),
    ({GS_PAIR: 0, GS_RESIDENT: 1}, 0, "l0_rows"), ({GS_PAIR: 0, GS_RESIDENT: 0}, 0, "l0_rows"),
    ({L1_MERGED: 0}, 1, "l1_per_element"), ({L1_MERGED: 1}, 1, "l1_merged"), ({L1_MERGED: 2}, 1, "l1_pair_rows"),
    ({L1_STORED: 1, STENCIL_SPLIT: 1}, 1, "l1_stored_ignored"), ({L1_STORED: 1, STENCIL_SPLIT: 0}, 1, "l1_stored_ignored"),
    ({L1_STORED: 2}, 1, "l1_stored_ignored"),
]
OPTION_NAMES = {GS_PAIR: "pair", GS_RESIDENT: "resident", STENCIL_SPLIT: "split", L1_STORED: "stored", L1_MERGED: "merged"}


def _variant_id(options):
    return "-".join("%s%d" % (OPTION_NAMES[k], v) for k, v in sorted(options.items()))


VARIANT_IDS = [_variant_id(o) for o, _, _ in VARIANTS]


@gpu
@pytest.mark.parametrize("options,level,branch", VARIANTS, ids=VARIANT_IDS)
def test_kernel_variants_on_odd_slab(options, level, branch, bcs):
    s = _slab("B", "cantilever", bcs)
    g = s.geom[level]
    assert g.xparity == 1
    NZ = g.nz + 1
    # the branch the launcher takes at this shape (launch_gs_sweep_mf, launch_l1_merged_sweep; mg_smooth of mg.hip)
    if branch == "l0_pair":
        assert all(l0_pair_segments(NZ, f) == (3, 3) for f in (True, False))       # k_gs_rows_mf0_pair, three segments per colour
    elif branch == "l0_rows":
        assert (NZ - 1) // 2 + 1 > 64                                              # k_gs_rows_mf0, more than one wave per row
    elif branch == "l1_pair_rows":
        assert l1_pair_segments(NZ, True) == (1, 3, 2) and l1_pair_segments(NZ, False) == (1, 2, 3)
        assert g.extra_lo == 1                                                     # level_E skips two fine layers
    elif branch in ("l1_merged", "l1_per_element", "l1_stored_ignored"):
        assert g.extra_lo == 1
    try:
        baseline = None
        if branch == "l1_stored_ignored":
            baseline = [_sweep_by_groups(s, level, f, "B default", "variants") for f in (True, False)]
        _set_options(s, options)
        got = [_sweep_by_groups(s, level, f, "B " + _variant_id(options), "variants") for f in (True, False)]
        if baseline is not None:
            # a slab never stores level 1: the option leaves it on the default on-the-fly kernels, bit for bit (the first colour
            # group, ghost planes included: after it the ghost planes come from the single grid, which does run the stored form)
            for a, c in zip(got, baseline):
                assert torch.equal(a, c)
    finally:
        _set_options(s, DEFAULTS)


# ---- 6. exported element matrices ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,bc", [s for s in SLABS if s[1] == "cantilever"], ids=[i for i in SLAB_IDS if i.endswith("cantilever")])
def test_exported_element_matrices(name, bc, bcs):
    """vfem_mg_export_level_ke as DistributedMGSolver._assemble_first_replicated_level calls it: this rank's x-layers of the level-T
    Galerkin element matrices, from the padded fine moduli (A: T = 2) or from the level-2 matrices of the slab (B, C: T = 3)"""
    s = _slab(name, bc, bcs)
    ref, lib, ds, T = s.ref, s.lib, s.ds, s.T
    gT, child = s.geom[T], s.geom[ds._export_child_level()]
    assert (T, child.l) == ((2, 0) if name == "A" else (3, 2))
    ne = CASES[name][0]
    nyz = (ne[1] >> T) * (ne[2] >> T)
    count = gT.X1 - gT.X0
    n = count * nyz * ds.KE_DOUBLES
    parent = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    mine = parent[GUARD:GUARD + n]
    _chk(lib.vfem_mg_export_level_ke(s.lmg, T, child.gl + child.extra_lo, count, _ptr(mine), _stream()))
    torch.cuda.synchronize()
    want = ref.omg.sims[T].Ke.reshape(ne[0] >> T, nyz * ds.KE_DOUBLES)[gT.X0:gT.X1].reshape(-1)
    eo = relerr(mine.cpu().numpy(), want)
    print("export level %d %s: slab - oracle %.3g" % (T, name, eo))
    _record("export_ke", "level%d_vs_oracle" % T, eo)
    assert eo < TOL_OP, (name, eo)
    assert guards_intact(parent), name
    # the single-grid hierarchy's export of the same layers: children start at global layer 2^(T - child level) * X0 of the child level
    single = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    _chk(lib.vfem_mg_export_level_ke(ref.tmg._h, T, gT.X0 << (T - child.l), count, _ptr(single), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(mine, single), name
