"""Caller buffers that start 8 bytes off the 16-byte grid of memory: views `parent[off : off + n]` into a longer device tensor.

Several kernels branch on the ADDRESS of the caller's vectors: the LDS-DMA apply / residual (kernels_apply_dma.hip: `ubase8`,
`last_piece`, `srow` of the line-exclusive tiling), the marching level-0 sweep (kernels_gs_march.hip: eight instantiations
<ALT, QF, QM> picked from the grid parities and from the 8-byte parities `bparR` / `bparO` of the two buffers it reads), the PCG
vector kernels (kernels_vec.hip: VEC = true / false from `aligned16`) and the LangelaarFilter marches (kernels_filter.hip: 16-byte
runs only where every array is 16-byte aligned).  A fresh torch allocation is 256-byte aligned, so the rest of the suite only
ever runs the even-base half of all of this.  Here every vector under test is a slice of a NaN-filled parent at offset 1 (odd: 8
bytes off the grid) or 2 (the control: aligned, same padding); two doubles of padding on either side keep every 16-byte piece
a clamp or the apply's `u - 8` can request inside the allocation, so a wrong shift gives wrong numbers, not a stray access.  After
every call: results finite, the padding of every written buffer still NaN, read-only buffers and their padding unchanged.
References: the fp64 CPU oracle (oracle.vfem_oracle) at the tolerances the aligned tests of the same quantities use, the numpy
restatement tests/langelaar_cpu.py for the filter, and the same call on aligned clones bit for bit.

Reached from the caller's pointers by these entry points: of the VEC = false vector kernels k_dot_partial (||b||^2 of an odd b,
the compliance) and k_pcg_step_dot (an odd x); k_dot_masked_partial and k_pcg_direction only ever see the hierarchy's own vectors.

Grids: the four of the table in test_shapes_reach_every_instantiation.  Shapes unchanged; the third, (6, 44, 61), takes the bridge
boundary condition instead of the cantilever: the cantilever's point load sits at y = z = 1/2 and needs a node there, i.e. an even
ny and nz, which no grid of this parity class (NZ even) has.  The bridge condition constrains whole x faces (all components at
x = 0, the x component at x = max), so the grid still has constrained components to bring back bit for bit.  Each grid has a z
seam and a y seam of the apply's 63 x 11 and of the march's 58 x 14 owned node columns inside it.

What the NaN padding found (fixed with this file): two kernels CONSUMED a double from outside the array, multiplied by a modulus
of 0 (an element outside the grid) -- harmless on finite garbage, NaN on NaN.  k_apply_dma / k_residual_dma read the far half of
last_piece when the array ends 8 bytes into that piece: u 8 bytes off with 3 nn even, but also an ALIGNED u with 3 nn odd, so the
result depended on what lay behind the caller's array (12 non-finite values at the last node column of the last two rows and
planes on grids 0 and 1).  k_gs_march_mf0 did the same, and with an odd buffer also consumed the near half of first_piece, u[-1].
The apply's lanes behind a row's end now read the row's last node (cmax); the sweep's DMA wave zeroes those halves in LDS (patchU).

Measured on an MI355X (helpers.record_deltas, parity_deltas.json), offset buffers against the same call on aligned clones: 0.0 in
every case -- apply, residual, plane ranges, line-exclusive tiling, marching sweeps (all four grids, both directions, 1 to 3 sweeps),
row sweeps, colour groups and plane ranges, PCG iterates (43 and 1 iterations), compliance, filter forward and backward.  The eight
marching instantiations differ in which registers of a staged window hold a row, not in the order of any sum, so equality is asserted.
Against the references: apply / residual <= 7.9e-16, marching sweeps <= 1.7e-15, row sweeps 4.5e-16 relative to the oracle; PCG u
2.0e-9 at (32, 16, 64) and 1.3e-10 at (9, 10, 20) with equal iteration counts; compliance 2.3e-16 of the numpy sum; filter forward
<= 1.4e-15 absolute, backward <= 5.1e-14 relative to tests/langelaar_cpu.py.  Mutations: MUTATIONS below.
"""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import langelaar_cpu as lc  # noqa: E402
from helpers import BC_BRIDGE, BC_CANTILEVER, ROOT, make_hip, make_oracle, record_deltas, relerr, seeded_density  # noqa: E402

TOL_OP = 1e-11            # apply and residual against the oracle (test_gpu_parity.TOL_OP)
TOL_SWEEP = 1e-10         # one sweep against the oracle (test_gpu_gs_march)
DMA_LX, GS_MARCH = 11, 19
DOM = ([0, 0, 0], [2, 1, 1])
# ne, boundary condition; NY, NZ / ppar = 3 NY NZ & 1 / ALT = NZ & 1:  31, 119 / 1 / 1;  30, 119 / 0 / 1;  45, 62 / 0 / 0;  14, 70 / 0 / 0
GRIDS = [((6, 30, 118), BC_CANTILEVER), ((6, 29, 118), None), ((6, 44, 61), BC_BRIDGE), ((5, 13, 69), None)]
OFFSETS = (1, 2)          # odd, and the aligned control with the same padding
SWEEP_CASES = [(fwd, n) for fwd in (1, 0) for n in (1, 2, 3)]
PCG_GRIDS = [((32, 16, 64), 2), ((9, 10, 20), 0)]          # 3 nn odd / even
PCG_OFFSETS = [(1, 2), (2, 1), (1, 1)]                      # (x, b)
NAN_BITS = 0x7FF8000000000000

MUTATIONS = """
  Each built as a library of its own, one change, and run on an MI355X against this file and the older files that cover the same
  kernels.  Each fails this file and no older one.
  1. launcher of k_gs_march_mf0: bparR dropped from the QM line.  This file: test_marching_sweeps_on_offset_buffers[0], [2] and
     test_marching_colour_groups_and_plane_ranges_on_offset_buffers[0], [2] fail at offset 1 (1.1e-7 and 4.8e-8 from the oracle against
     the bound 1e-10), grids 1 and 3 pass.  tests/test_gpu_gs_march.py: 8 passed.  (QM and QF place the ten-double read of a window:
     the doubles consumed are the same, a wrong value makes the five 16-byte LDS reads start 8 bytes off a 16-byte boundary.)
  2. the same with bparO dropped from the QF line.  This file: the two colour-group cases [0], [2] fail at offset 1 (a bitwise
     comparison); tests/test_gpu_gs_march.py: 8 passed.
  3. k_pcg_step_dot<VEC = false> skips the odd last element.  This file: test_pcg_on_offset_buffers[(32, 16, 64)] fails at (x, b)
     offsets (1, 2) (3 nn odd, x odd), (9, 10, 20) passes (3 nn even).  The PCG / CG tests of tests/test_gpu_parity.py and
     tests/test_gpu_gs_march.py: 11 passed.
  4. scalar path of store_run (kernels_filter.hip) stops one layer early where nz is even -- the scalar path at an even nz is what only
     an offset buffer reaches; at an odd nz it is what every buffer takes and tests/test_gpu_langelaar.py already covers.  This file:
     the three test_langelaar_on_offset_buffers cases fail; tests/test_gpu_langelaar.py (without its 512 x 256 x 256 case): 19 passed.
"""


# ------------------------------------------------------------------------------------------------------------------------------
# what the launchers select, restated (no GPU needed)
# ------------------------------------------------------------------------------------------------------------------------------
def march_instantiation(NY, NZ, cxl, forward, par_r, par_o):
    """<ALT, QF, QM> of launch_gs_march_mf0 for relaxed planes of local parity cxl read from a buffer of 8-byte parity par_r, the
    other planes from one of parity par_o"""
    P = 0 if forward else 1
    ppar, ALT = (3 * NY * NZ) & 1, NZ & 1
    QF = ((P + 1) + par_o + ((cxl + 1) & ppar) + ALT * P) & 1
    QM = ((P + 1) + par_r + (cxl & ppar) + ALT * P) & 1
    return ALT, QF, QM


def sweeps_launches(NY, NZ, u_par, forward, n):
    """the marching launches of mg_smooth_n: the planes of either parity ping-pong between u and the level's scratch vector (its own
    allocation: parity 0); xparity = 0 on a whole grid"""
    cur = ["u", "u"]
    par = {"u": u_par, "tmp": 0}
    out = []
    for _ in range(n):
        for half in range(2):
            cxl = half if forward else 1 - half
            dst = "tmp" if cur[cxl] == "u" else "u"
            out.append(march_instantiation(NY, NZ, cxl, forward, par[cur[cxl]], par[cur[1 - cxl]]))
            cur[cxl] = dst
    return out


def half_launches(NY, NZ, u_par, forward):
    """mg_smooth_half (vfem_mg_smooth_colors group by group, vfem_mg_smooth_group_planes): both halves read u only"""
    return [march_instantiation(NY, NZ, (half if forward else 1 - half), forward, u_par, u_par) for half in range(2)]


def instantiations_reached(offsets):
    got = set()
    for ne, _ in GRIDS:
        NY, NZ = ne[1] + 1, ne[2] + 1
        for off in offsets:
            for fwd, n in SWEEP_CASES:
                got.update(sweeps_launches(NY, NZ, off & 1, fwd, n))
            for fwd in (1, 0):
                got.update(half_launches(NY, NZ, off & 1, fwd))
    return got


def _source(name):
    with open(os.path.join(ROOT, "ndr_amd", "csrc", name)) as fh:
        return fh.read()


def test_shapes_reach_every_instantiation():
    """| grid          | NY, NZ  | ppar | ALT |      the GPU cases below launch all eight <ALT, QF, QM> of the marching sweep; the
       | (6, 30, 118)  | 31, 119 |  1   |  1  |      aligned controls alone only five; the apply meets both parities of u and of 3 nn
       | (6, 29, 118)  | 30, 119 |  0   |  1  |      (where last_piece falls); the restated formulas are still the launcher's text
       | (6, 44, 61)   | 45, 62  |  0   |  0  |
       | (5, 13, 69)   | 14, 70  |  0   |  0  |"""
    every = {(a, f, m) for a in (0, 1) for f in (0, 1) for m in (0, 1)}
    assert instantiations_reached(OFFSETS) == every
    assert instantiations_reached((2,)) == {(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1)}
    assert (1, 0, 0) in instantiations_reached((1,))
    # (0,0,1), (0,1,0): uR and uO of different parity, i.e. an odd u against the even scratch vector
    mixed = set()
    for ne, _ in GRIDS:
        for fwd, n in SWEEP_CASES:
            mixed.update(sweeps_launches(ne[1] + 1, ne[2] + 1, 1, fwd, n))
    assert {(0, 0, 1), (0, 1, 0)} <= mixed
    ends = {(off & 1, (3 * int(np.prod([n + 1 for n in ne]))) & 1) for ne, _ in GRIDS for off in OFFSETS}
    ends |= {(off & 1, (3 * int(np.prod([n + 1 for n in ne]))) & 1) for ne, _ in PCG_GRIDS for off in OFFSETS}
    assert ends == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert [(3 * int(np.prod([n + 1 for n in ne]))) & 1 for ne, _ in PCG_GRIDS] == [1, 0]
    # the restatement is the launcher's own line
    src = re.sub(r"\s+", " ", _source("kernels_gs_march.hip"))
    assert re.search(r"const int P = forward \? 0 : 1;", src)
    assert re.search(r"const int ppar = \(int\) \(\(3 \* plane\) & 1\), ALT = d\.NZ & 1;", src)
    assert re.search(r"const int QF = \(\(P \+ 1\) \+ bparO \+ \(\(cxl \+ 1\) & ppar\) \+ ALT \* P\) & 1, "
                     r"QM = \(\(P \+ 1\) \+ bparR \+ \(cxl & ppar\) \+ ALT \* P\) & 1;", src)
    assert re.search(r"switch \(ALT \* 4 \+ QF \* 2 \+ QM\)", src)
    cases = re.findall(r"case (\d): VFEM_GSM_LAUNCH\((\d), (\d), (\d)\); break;", src)
    assert [int(c[0]) for c in cases] == list(range(7)) and "default: VFEM_GSM_LAUNCH(1, 1, 1); break;" in src
    assert all(int(n) == 4 * int(a) + 2 * int(f) + int(m) for n, a, f, m in cases)
    mg = re.sub(r"\s+", " ", _source("mg.hip"))
    assert re.search(r"double \*cur\[2\] = \{u, u\};", mg)
    assert re.search(r"const int cx = forward \? half : 1 - half;", mg)
    assert re.search(r"double \*dst = cur\[cxl\] == u \? L\.tmp\.p : u;", mg)
    assert re.search(r"launch_gs_march_mf0\(L\.d, march_table\(sim\), level_E\(mg, 0\), cur\[cxl\], cur\[1 - cxl\], dst, b,", mg)
    assert re.search(r"launch_gs_march_mf0\(L\.d, march_table\(sim\), level_E\(mg, 0\), u, u, L\.tmp\.p, b,", mg)
    # the filter's 16-byte runs hang on the pointers as well as on nz
    flt = re.sub(r"\s+", " ", _source("kernels_filter.hip"))
    assert re.search(r"runs_aligned16\(nz, in, out, smax\)", flt) and re.search(r"runs_aligned16\(nz, g, vars, out, smax, grad\)", flt)
    assert "(nz & 1) == 0 && (((reinterpret_cast<uintptr_t>(arrays) & 15u) == 0) && ...)" in flt


# ------------------------------------------------------------------------------------------------------------------------------
# GPU cases
# ------------------------------------------------------------------------------------------------------------------------------
class Placed:
    """`src` copied into parent[off : off + n] of a NaN-filled parent of n + pad doubles (pad = 4: two doubles on either side of the
    view at offset 2, one and three at offset 1)"""

    def __init__(self, src, off, pad=4):
        import torch
        flat = src.reshape(-1)
        self.n, self.off = flat.numel(), off
        assert 1 <= off <= pad - 2                                    # never flush with the parent
        self.parent = torch.full((self.n + pad,), float("nan"), dtype=torch.float64, device="cuda")
        assert self.parent.data_ptr() % 16 == 0
        self.v = self.parent[off:off + self.n]
        self.v.copy_(flat)
        self.before = flat.clone()
        assert self.v.data_ptr() % 16 == 8 * (off & 1)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.v.data_ptr())

    def padding_intact(self):
        import torch
        bits = torch.cat([self.parent[:self.off], self.parent[self.off + self.n:]]).view(torch.int64)
        return bool((bits == NAN_BITS).all())

    def check_written(self):
        import torch
        assert self.padding_intact(), "written outside the view"
        assert bool(torch.isfinite(self.v).all())

    def check_read_only(self):
        import torch
        assert self.padding_intact() and torch.equal(self.v, self.before), "a read-only buffer changed"


def _nan_like(src, off, pad=4):
    import torch
    return Placed(torch.full_like(src, float("nan")), off, pad)


def _api():
    from ndr_amd import _lib
    from ndr_amd.pyVoxelFEM import _stream
    return _lib.load(), _lib.check, _stream()


def _set(t, key, value):
    lib, check, _ = _api()
    check(lib.vfem_sim_set_option(t._h, key, value))


@functools.lru_cache(maxsize=None)
def _problem(gi):
    """grid gi on both sides, level 0 only; u has its constrained components zeroed as a sweep's input must"""
    import torch
    from oracle import vfem_oracle as vo
    ne, bc = GRIDS[gi]
    rho = seeded_density(ne, 88, "proxy")
    o, t = make_oracle(ne, DOM, bc, rho), make_hip(ne, DOM, bc, rho)
    omg = vo.OracleMG(o, 0, nthreads=4)
    omg.update_element_stiffness()
    tmg = t.multigridSolver(0)
    rng = np.random.default_rng(5 + gi)
    u, b = rng.standard_normal((o.num_nodes, 3)), rng.standard_normal((o.num_nodes, 3))
    omg.enforce_dirichlet(0, u, True)
    return dict(ne=ne, o=o, t=t, omg=omg, tmg=tmg, u=u, b=b, ud=torch.as_tensor(u, device="cuda"), bd=torch.as_tensor(b, device="cuda"),
                fixed=o.dmask.astype(bool))


@functools.lru_cache(maxsize=None)
def _oracle_ops(gi):
    p = _problem(gi)
    return p["o"].apply_k(p["u"]), p["omg"].residual(0, p["u"].copy(), p["b"])


@functools.lru_cache(maxsize=None)
def _oracle_sweeps(gi, fwd):
    """u after 1, 2, 3 sweeps in one direction"""
    p = _problem(gi)
    us, res = p["u"].copy(), []
    for _ in range(3):
        p["omg"].smoothing(0, us, p["b"], bool(fwd))
        res.append(us.copy())
    return res


def _ops(p, u, b, out, which):
    lib, check, s = _api()
    if which == "sim_apply":
        check(lib.vfem_sim_apply_k(p["t"]._h, u, out, 0, s))
    elif which == "mg_apply":
        check(lib.vfem_mg_apply_k(p["tmg"]._h, 0, u, out, s))
    else:
        check(lib.vfem_mg_residual(p["tmg"]._h, 0, u, b, out, s))


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_apply_and_residual_on_offset_buffers(gi):
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    p = _problem(gi)
    _set(p["t"], DMA_LX, 0)
    ref_apply, ref_res = _oracle_ops(gi)
    worst, worst_al = {}, 0.0
    for which in ("sim_apply", "mg_apply", "residual"):
        aligned, uc, bc = torch.full_like(p["ud"], float("nan")), p["ud"].clone(), p["bd"].clone()
        _ops(p, _ptr(uc), _ptr(bc), _ptr(aligned), which)
        assert torch.equal(uc, p["ud"]) and torch.equal(bc, p["bd"])
        ref = ref_res if which == "residual" else ref_apply
        assert relerr(aligned.cpu().numpy(), ref) < TOL_OP, which
        for uo in OFFSETS:
            for oo in OFFSETS:
                u, b, out = Placed(p["ud"], uo), Placed(p["bd"], 1), _nan_like(p["ud"], oo)
                _ops(p, u.ptr, b.ptr, out.ptr, which)
                out.check_written()
                u.check_read_only()
                b.check_read_only()
                got = out.v.view_as(aligned)
                worst[which] = max(worst.get(which, 0.0), relerr(got.cpu().numpy(), ref))
                worst_al = max(worst_al, float((got - aligned).abs().max()))
                assert worst[which] < TOL_OP, (which, uo, oo)
                assert torch.equal(got, aligned), (which, uo, oo)
    record_deltas("buffer_alignment_apply_%d" % gi, {"grid": list(p["ne"]), "relerr_vs_oracle": worst, "vs_aligned": worst_al})


@pytest.mark.gpu
@pytest.mark.parametrize("gi", [0, 1])
def test_line_exclusive_tiling_on_offset_results(gi):
    """VFEM_OPT_DMA_LX = 2: the first emitted column of a row in doubles mod 16 (`srow`) follows the address of the result"""
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    lib, check, s = _api()
    p = _problem(gi)
    t = p["t"]
    _set(t, DMA_LX, 0)
    aligned, uc = torch.full_like(p["ud"], float("nan")), p["ud"].clone()
    check(lib.vfem_sim_apply_k(t._h, _ptr(uc), _ptr(aligned), 0, s))
    _set(t, DMA_LX, 2)
    try:
        for uo in OFFSETS:
            for oo in (1, 6, 15):
                u, out = Placed(p["ud"], uo), _nan_like(p["ud"], oo, pad=18)
                check(lib.vfem_sim_apply_k(t._h, u.ptr, out.ptr, 0, s))
                out.check_written()
                u.check_read_only()
                assert torch.equal(out.v.view_as(aligned), aligned), (uo, oo)
                r, b = _nan_like(p["ud"], oo, pad=18), Placed(p["bd"], 1)
                check(lib.vfem_mg_residual(p["tmg"]._h, 0, u.ptr, b.ptr, r.ptr, s))
                r.check_written()
                assert relerr(r.v.view_as(aligned).cpu().numpy(), _oracle_ops(gi)[1]) < TOL_OP, (uo, oo)
    finally:
        _set(t, DMA_LX, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_plane_ranges_of_an_odd_field(gi):
    import torch
    lib, check, s = _api()
    p = _problem(gi)
    _set(p["t"], DMA_LX, 0)
    NX = p["ne"][0] + 1
    u = Placed(p["ud"], 1)
    full = _nan_like(p["ud"], 2)
    check(lib.vfem_sim_apply_k(p["t"]._h, u.ptr, full.ptr, 0, s))
    full.check_written()
    fv = full.v.view(NX, -1)
    assert relerr(fv.cpu().numpy().reshape(-1, 3), _oracle_ops(gi)[0]) < TOL_OP
    for lo, hi in ((0, 0), (1, NX - 2), (NX - 1, NX - 1)):
        for oo in OFFSETS:
            out = _nan_like(p["ud"], oo)
            check(lib.vfem_sim_apply_k_planes(p["t"]._h, u.ptr, out.ptr, lo, hi, s))
            assert out.padding_intact()
            ov = out.v.view(NX, -1)
            assert torch.equal(ov[lo:hi + 1], fv[lo:hi + 1]), (lo, hi, oo)
            assert bool(torch.isnan(ov[:lo]).all()) and bool(torch.isnan(ov[hi + 1:]).all()), (lo, hi, oo)
    u.check_read_only()


def _sweep_checks(p, gi, march, tag):
    """vfem_mg_smooth_sweeps on offset buffers, both directions, 1 to 3 sweeps: oracle, constrained components, aligned clones"""
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    lib, check, s = _api()
    _set(p["t"], GS_MARCH, march)
    worst, worst_al = 0.0, 0.0
    try:
        # (mg_smooth_n falls back to the row kernels without a word where the level cannot march)
        assert lib.vfem_mg_can_smooth_planes(p["tmg"]._h, 0) == (1 if march == 2 else 0)
        for fwd, n in SWEEP_CASES:
            ref = _oracle_sweeps(gi, fwd)[n - 1]
            al, bc = p["ud"].clone(), p["bd"].clone()
            check(lib.vfem_mg_smooth_sweeps(p["tmg"]._h, 0, _ptr(al), _ptr(bc), fwd, n, s))
            for uo in OFFSETS:
                u, b = Placed(p["ud"], uo), Placed(p["bd"], 1)
                check(lib.vfem_mg_smooth_sweeps(p["tmg"]._h, 0, u.ptr, b.ptr, fwd, n, s))
                u.check_written()
                b.check_read_only()
                got = u.v.view_as(al)
                g = got.cpu().numpy()
                worst = max(worst, relerr(g, ref))
                worst_al = max(worst_al, float((got - al).abs().max() / al.abs().max()))
                assert relerr(g, ref) < TOL_SWEEP, (fwd, n, uo)
                assert np.array_equal(g[p["fixed"]], p["u"][p["fixed"]]), (fwd, n, uo)
                assert torch.equal(got, al), (fwd, n, uo)
    finally:
        _set(p["t"], GS_MARCH, 1)
    record_deltas("buffer_alignment_%s_%d" % (tag, gi), {"grid": list(p["ne"]), "relerr_vs_oracle": worst, "vs_aligned": worst_al})


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_marching_sweeps_on_offset_buffers(gi):
    """every sweep count mixes the parities of uR and uO (the scratch vector is even); the result must equal the sweeps on aligned clones bit for bit"""
    _sweep_checks(_problem(gi), gi, 2, "march")


@pytest.mark.gpu
def test_row_kernel_sweeps_on_offset_buffers():
    _sweep_checks(_problem(0), 0, 0, "rows")


@pytest.mark.gpu
@pytest.mark.parametrize("gi", range(len(GRIDS)))
def test_marching_colour_groups_and_plane_ranges_on_offset_buffers(gi):
    """vfem_mg_smooth_colors group by group and vfem_mg_smooth_group_planes (uR = uO = u): a forward then a backward sweep made
    of half sweeps; the planes of one colour group do not depend on each other, so a group done in two plane ranges is the group"""
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    lib, check, s = _api()
    p = _problem(gi)
    h, NX = p["tmg"]._h, p["ne"][0] + 1
    ref_f = _oracle_sweeps(gi, 1)[0]
    ref_fb = ref_f.copy()
    p["omg"].smoothing(0, ref_fb, p["b"], False)
    _set(p["t"], GS_MARCH, 2)
    try:
        assert lib.vfem_mg_can_smooth_planes(h, 0) == 1
        al = p["ud"].clone()
        for fwd in (1, 0):
            for first in (0, 4):
                check(lib.vfem_mg_smooth_colors(h, 0, _ptr(al), _ptr(p["bd"]), fwd, first, 4, s))
        for uo in OFFSETS:
            u, b = Placed(p["ud"], uo), Placed(p["bd"], 1)
            w = Placed(p["ud"], uo)                                  # the same sweeps, each group in two plane ranges
            for fwd, ref in ((1, ref_f), (0, ref_fb)):
                for first in (0, 4):
                    check(lib.vfem_mg_smooth_colors(h, 0, u.ptr, b.ptr, fwd, first, 4, s))
                    for lo, hi in ((0, 2), (3, NX - 1)):
                        check(lib.vfem_mg_smooth_group_planes(h, 0, w.ptr, b.ptr, fwd, first // 4, lo, hi, s))
                u.check_written()
                w.check_written()
                g = u.v.view_as(al).cpu().numpy()
                assert relerr(g, ref) < TOL_SWEEP, (uo, fwd)
                assert np.array_equal(g[p["fixed"]], p["u"][p["fixed"]]), (uo, fwd)
                assert torch.equal(w.v, u.v), (uo, fwd)
            b.check_read_only()
            assert torch.equal(u.v.view_as(al), al), uo
    finally:
        _set(p["t"], GS_MARCH, 1)


@functools.lru_cache(maxsize=None)
def _pcg_problem(ne, levels):
    from oracle import vfem_oracle as vo
    rho = seeded_density(ne, 88, "proxy")
    o, t = make_oracle(ne, DOM, BC_CANTILEVER, rho), make_hip(ne, DOM, BC_CANTILEVER, rho)
    _set(t, GS_MARCH, 2)
    f = o.build_load_vector()
    omg = vo.OracleMG(o, levels, nthreads=4)
    uo = omg.pcg(np.zeros_like(f), f, 100, 1e-6, 1, 2, True)
    return o, t, t.multigridSolver(levels), f, uo, omg.last_iters


def _pcg(mg, x, b):
    from ndr_amd import _lib
    lib, check, s = _api()
    its, rel = ctypes.c_int(0), ctypes.c_double(0.0)
    check(lib.vfem_mg_pcg(mg._h, x, b, 100, 1e-6, 1, 2, 1, _lib.RESIDUAL_CB(), None, ctypes.byref(its), ctypes.byref(rel), s))
    return its.value


@pytest.mark.gpu
@pytest.mark.parametrize("ne,levels", PCG_GRIDS)
def test_pcg_on_offset_buffers(ne, levels):
    """an odd b: ||b||^2 by k_dot_partial<false>; an odd x: the initial residual of an odd field, k_pcg_step_dot<false>; iteration
    count and iterate equal the aligned run bit for bit (kernels_vec.hip: the partition and the order of a sum do not depend on the
    alignment), and the oracle as in test_pcg_with_marching_sweeps_matches_oracle"""
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    o, t, mg, f, uo, iters = _pcg_problem(ne, levels)
    fd = torch.as_tensor(f, device="cuda")
    xa = torch.zeros_like(fd)
    fc = fd.clone()
    its_a = _pcg(mg, _ptr(xa), _ptr(fc))
    assert its_a == iters
    co, worst_al = float(np.sum(f * uo)), 0.0
    for xo, bo in PCG_OFFSETS:
        x, b = Placed(torch.zeros_like(fd), xo), Placed(fd, bo)
        its = _pcg(mg, x.ptr, b.ptr)
        x.check_written()
        b.check_read_only()
        worst_al = max(worst_al, float((x.v.view_as(xa) - xa).abs().max()))
        assert its == its_a == iters, (xo, bo)
        assert torch.equal(x.v.view_as(xa), xa), (xo, bo)
        ug = x.v.view_as(xa).cpu().numpy()
        assert abs(float(np.sum(f * ug)) - co) < 1e-8 * abs(co), (xo, bo)
        assert relerr(ug, uo) < 1e-6, (xo, bo)
    record_deltas("buffer_alignment_pcg_%dx%dx%d" % ne, {"iterations": its_a, "relerr_u_vs_oracle": relerr(xa.cpu().numpy(), uo), "vs_aligned": worst_al})


@pytest.mark.gpu
@pytest.mark.parametrize("gi", [0, 3])                       # 3 nn odd / even
def test_compliance_of_offset_buffers(gi):
    lib, check, s = _api()
    from ndr_amd.pyVoxelFEM import _ptr
    p = _problem(gi)

    def value(fp, up):
        v = ctypes.c_double(0.0)
        check(lib.vfem_compliance(p["t"]._h, fp, up, ctypes.byref(v), s))
        return v.value

    ref = value(_ptr(p["bd"]), _ptr(p["ud"]))
    assert abs(ref - 0.5 * float(np.sum(p["b"] * p["u"]))) < 1e-12 * float(np.sum(np.abs(p["b"] * p["u"])))
    worst_al = 0.0
    for fo, uo in ((1, 2), (2, 1), (1, 1), (2, 2)):
        f, u = Placed(p["bd"], fo), Placed(p["ud"], uo)
        got = value(f.ptr, u.ptr)
        worst_al = max(worst_al, abs(got - ref))
        assert got == ref, (fo, uo)
        f.check_read_only()
        u.check_read_only()
    record_deltas("buffer_alignment_compliance_%d" % gi, {"grid": list(p["ne"]), "vs_aligned": worst_al,
                                                          "relerr_vs_numpy": abs(ref - 0.5 * float(np.sum(p["b"] * p["u"]))) / abs(ref)})


# ---- LangelaarFilter --------------------------------------------------------------------------------------------------------
def _filter(dims):
    from ndr_amd import pyVoxelFEM as pv
    f = pv.LangelaarFilter()
    f._set_grid(dims)
    return f


@functools.lru_cache(maxsize=None)
def _langelaar_ref(dims):
    n = int(np.prod(dims))
    x, g = np.random.default_rng(17).uniform(0.0, 1.0, n), np.random.default_rng(18).standard_normal(n)
    out, smax = lc.apply(x, dims)
    return x, g, out, smax, lc.backprop(g, x, dims, out, smax)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [(33, 17, 10), (64, 64, 64), (160, 80)])
def test_langelaar_on_offset_buffers(dims):
    """an even layer axis and arrays 8 bytes off the 16-byte grid: the launchers take the scalar runs (before the fix this
    test would have issued 16-byte accesses at 8-byte addresses: it exists for the fixed code only)"""
    import torch
    x, g, out_ref, smax_ref, grad_ref = _langelaar_ref(dims)
    xd, gd = torch.as_tensor(x, device="cuda"), torch.as_tensor(g, device="cuda")
    fa = _filter(dims)
    out_a = fa.apply_dev(xd.clone())
    grad_a = fa.backprop_dev(gd.clone(), xd.clone())
    assert np.abs(out_a.cpu().numpy() - out_ref).max() <= 1e-12
    assert np.abs(grad_a.cpu().numpy() - grad_ref).max() <= 1e-10 * np.abs(grad_ref).max()
    f = _filter(dims)
    xp = Placed(xd, 1)
    out = f.apply_dev(xp.v)
    xp.check_read_only()
    assert bool(torch.isfinite(out).all())
    assert np.abs(out.cpu().numpy() - out_ref).max() <= 1e-12
    assert np.abs(f._smax.cpu().numpy() - smax_ref).max() <= 1e-12
    assert torch.equal(out, out_a) and torch.equal(f._smax, fa._smax)
    for go, xo in ((1, 2), (2, 1)):
        gp, xp = Placed(gd, go), Placed(xd, xo)
        grad = f.backprop_dev(gp.v, xp.v)
        gp.check_read_only()
        xp.check_read_only()
        assert bool(torch.isfinite(grad).all())
        assert np.abs(grad.cpu().numpy() - grad_ref).max() <= 1e-10 * np.abs(grad_ref).max(), (go, xo)
        assert torch.equal(grad, grad_a), (go, xo)
    record_deltas("buffer_alignment_langelaar_" + "x".join(str(d) for d in dims),
                  {"forward_abs": float(np.abs(out.cpu().numpy() - out_ref).max()),
                   "backward_rel": float(np.abs(grad.cpu().numpy() - grad_ref).max() / np.abs(grad_ref).max()),
                   "vs_aligned": max(float((out - out_a).abs().max()), float((grad - grad_a).abs().max()))})
    # the arrays the marches write, through the C entry points: out / smax / grad off the grid, the inputs on it
    lib, check, s = _api()
    from ndr_amd.pyVoxelFEM import _ptr
    nl = f._nl()
    for oo, so in ((1, 2), (2, 1)):
        o_, s_, gr = _nan_like(xd, oo), _nan_like(xd, so), _nan_like(xd, oo)
        check(lib.vfem_langelaar_apply(nl, f._EPS, f._P, f._Q, _ptr(xd), o_.ptr, s_.ptr, s))
        o_.check_written()
        s_.check_written()
        assert torch.equal(o_.v, out_a) and torch.equal(s_.v, fa._smax), (oo, so)
        work = torch.empty(2 * nl[0] * nl[1], dtype=torch.float64, device="cuda")
        check(lib.vfem_langelaar_backprop(nl, f._EPS, f._P, f._Q, _ptr(gd), _ptr(xd), o_.ptr, s_.ptr, _ptr(work), gr.ptr, s))
        gr.check_written()
        assert o_.padding_intact() and s_.padding_intact()
        assert torch.equal(gr.v, grad_a), (oo, so)


@pytest.mark.gpu
def test_langelaar_2d_grid_wider_than_one_workgroup():
    """1100 columns against the 1008 core columns of a Region<1> workgroup (aligned buffers)"""
    dims = (1100, 20)
    x, g, out_ref, smax_ref, grad_ref = _langelaar_ref(dims)
    f = _filter(dims)
    out = f.apply(x)
    assert np.all(np.isfinite(out))
    assert np.abs(out - out_ref).max() <= 1e-12
    assert np.abs(f._smax.cpu().numpy() - smax_ref).max() <= 1e-12
    got = f.backprop(g, x)
    assert np.all(np.isfinite(got))
    assert np.abs(got - grad_ref).max() <= 1e-10 * np.abs(grad_ref).max()
