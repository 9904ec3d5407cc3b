"""The balanced schedule of the LDS-DMA apply (kernels_apply_dma.hip: k_apply_dma_sched) against the grid launch it replaces.

With VFEM_OPT_DMA_CHUNKS = 0, VFEM_OPT_DMA_STRIP = 1 and VFEM_OPT_DMA_LX = 0 (the defaults) the apply, the level-0 residual and the
plane-range apply run as one block per CU that marches a list of segments (tile column x plane range) derived from its id: block b is
slot b / 8 of team b % 8, team t owns slab t % nslab of the planes, the 8 / nslab teams of a slab split its tile columns, and the
C mod S columns a team has left after its whole rounds of S columns are cut in x into S pieces.  Any other value of the three options
takes the old launch of one block per tile and x-chunk; VFEM_OPT_DMA_CHUNKS = 8 is that launch with the default tiling.

A march restarts its carry and fold from the plane below its first output plane, so where it is cut in x changes no sum, and the tile
of a node column is the same under both launches: every assertion here is bitwise (torch.equal).

What the grids reach, with S = 32 slots per team (256 CUs); NX planes -> nslab as the launcher picks it (>= 64: 8, >= 16: 4, else 1):
  (40, 400, 70)   41 planes, nslab 4 (slabs of 10, 10, 10, 11), two teams per slab; 37 main + 9 strip columns = 46 per slab, 23 per
                  team: fewer than S, so every column is remainder, 23 L plane-steps in pieces of 8 that cross column ends; both
                  tile shapes.  (The issue's table expects a whole round here; with the slab's columns split over two teams of 32
                  slots there is none -- the last two grids below have one.)
  (9, 70, 64)     10 planes, nslab 1, 8 teams share 7 + 2 = 9 columns (1 or 2 each): pieces of 1 plane, most slots idle
  (5, 13, 78)     6 planes, nslab 1, 2 x 2 main columns and no strip (the 16 node columns left over are one too many for it): four
                  teams have one column in pieces of 1 plane, four have none at all
  (70, 96, 126)   71 planes, nslab 8 with slabs of 8 and 9 planes; 18 main + 3 strip columns (a strip of one node column)
  (3, 400, 448)   4 planes, nslab 1; 259 main + 9 strip = 268 columns, 33 or 34 per team: one whole round, then 1 or 2 columns of
                  4 planes in pieces of 1
  (63, 120, 196)  64 planes, nslab 8 (slabs of 8); 33 main + 3 strip = 36 columns per team: one whole round, 4 x 8 plane-steps left
"""
import ctypes
import functools
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from helpers import BC_CANTILEVER, make_hip, seeded_density  # noqa: E402

DMA_CHUNKS = 7            # VFEM_OPT_DMA_CHUNKS
DOM = ([0, 0, 0], [2, 1, 1])
CASE1 = (40, 400, 70)
GRIDS = [CASE1, (9, 70, 64), (5, 13, 78), (70, 96, 126), (3, 400, 448), (63, 120, 196)]
NAN_BITS = 0x7FF8000000000000


def _api():
    from ndr_amd import _lib
    from ndr_amd.pyVoxelFEM import _stream
    return _lib.load(), _lib.check, _stream()


def _schedule(t, old):
    lib, check, _ = _api()
    check(lib.vfem_sim_set_option(t._h, DMA_CHUNKS, 8 if old else 0))


@functools.lru_cache(maxsize=None)
def _problem(ne):
    """simulator (cantilever mask, seeded densities), a seeded u and b, and K u by the old launch -- computed once, never written again"""
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    lib, check, s = _api()
    # the cantilever's point load needs a node at y = z = 1/2 (an even ny and nz); only the residual case, on CASE1, uses the mask
    t = make_hip(ne, DOM, BC_CANTILEVER if ne == CASE1 else None, seeded_density(ne, 88, "proxy"))
    g = torch.Generator(device="cuda").manual_seed(1234 + sum(ne))
    u = torch.randn((t.numNodes(), 3), dtype=torch.float64, device="cuda", generator=g)
    b = torch.randn((t.numNodes(), 3), dtype=torch.float64, device="cuda", generator=g)
    old = torch.full_like(u, float("nan"))
    _schedule(t, True)
    try:
        check(lib.vfem_sim_apply_k(t._h, _ptr(u), _ptr(old), 0, s))
    finally:
        _schedule(t, False)
    assert bool(torch.isfinite(old).all()) and float(old.abs().max()) > 0.0
    return dict(ne=ne, t=t, u=u, b=b, old=old)


@pytest.mark.gpu
@pytest.mark.parametrize("ne", GRIDS, ids=lambda ne: "%dx%dx%d" % ne)
def test_apply_is_bitwise_the_old_launch(ne):
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    lib, check, s = _api()
    p = _problem(ne)
    new = torch.full_like(p["u"], float("nan"))
    check(lib.vfem_sim_apply_k(p["t"]._h, _ptr(p["u"]), _ptr(new), 0, s))
    assert torch.equal(new, p["old"])


@pytest.mark.gpu
def test_plane_ranges():
    """a single interior plane, the first, the last, and an odd interior range (33 planes: nslab 4, slabs of 8, 8, 8, 9)"""
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    lib, check, s = _api()
    p = _problem(CASE1)
    NX = CASE1[0] + 1
    full = p["old"].view(NX, -1)
    for lo, hi in ((17, 17), (0, 0), (NX - 1, NX - 1), (3, 35)):
        out = torch.full_like(p["u"], float("nan"))
        check(lib.vfem_sim_apply_k_planes(p["t"]._h, _ptr(p["u"]), _ptr(out), lo, hi, s))
        ov = out.view(NX, -1)
        assert torch.equal(ov[lo:hi + 1], full[lo:hi + 1]), (lo, hi)
        assert bool(torch.isnan(ov[:lo]).all()) and bool(torch.isnan(ov[hi + 1:]).all()), (lo, hi)


@pytest.mark.gpu
def test_residual_at_level_0():
    """vfem_mg_residual = b - K u, 0 at the cantilever's fixed components; the subtraction is the kernel's own single operation"""
    import torch
    from ndr_amd.pyVoxelFEM import _ptr
    lib, check, s = _api()
    p = _problem(CASE1)
    tmg = p["t"].multigridSolver(0)
    fixed = torch.as_tensor(p["t"].dirichletMask, device="cuda").view_as(p["u"])
    assert 0 < int(fixed.sum()) < fixed.numel()
    want = torch.where(fixed, torch.zeros_like(p["u"]), p["b"] - p["old"])
    got = torch.full_like(p["u"], float("nan"))
    check(lib.vfem_mg_residual(tmg._h, 0, _ptr(p["u"]), _ptr(p["b"]), _ptr(got), s))
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_views_8_bytes_off_a_16_byte_line():
    """u and the result as views parent[1 : 1 + n] of NaN-filled parents (two spare doubles behind, one in front); the guards stay NaN"""
    import torch
    lib, check, s = _api()
    p = _problem(CASE1)
    n = p["u"].numel()
    for uo, oo in ((1, 1), (1, 2), (2, 1)):
        up = torch.full((n + 4,), float("nan"), dtype=torch.float64, device="cuda")
        op = torch.full((n + 4,), float("nan"), dtype=torch.float64, device="cuda")
        uv, ov = up[uo:uo + n], op[oo:oo + n]
        uv.copy_(p["u"].reshape(-1))
        assert uv.data_ptr() % 16 == 8 * (uo & 1) and ov.data_ptr() % 16 == 8 * (oo & 1)
        check(lib.vfem_sim_apply_k(p["t"]._h, ctypes.c_void_p(uv.data_ptr()), ctypes.c_void_p(ov.data_ptr()), 0, s))
        assert torch.equal(ov.view_as(p["old"]), p["old"]), (uo, oo)
        guards = torch.cat([op[:oo], op[oo + n:], up[:uo], up[uo + n:]]).view(torch.int64)
        assert bool((guards == NAN_BITS).all()), (uo, oo)
        assert torch.equal(uv, p["u"].reshape(-1)), (uo, oo)
