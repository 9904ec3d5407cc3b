"""-m gpu: the box filter on an x-slab (vfem_box_filter_slab) equals the matching slice of the whole-grid filter (vfem_box_filter) bit
for bit, apply and transpose, for slabs at either end, inside and over the whole grid; and every inconsistent call is refused."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _whole(lib, grid, r, x, transpose):
    out = torch.empty_like(x)
    status = lib.vfem_box_filter((ctypes.c_int64 * 3)(*grid), r, _p(x), _p(out), transpose, _s())
    assert status == 0
    return out


def _slab(lib, grid, r, x, lo, hi, transpose):
    """owned layers [lo, hi) with r ghost layers on each side that has neighbours; returns the owned layers' output"""
    nx, layer = grid[0], grid[1] * grid[2]
    a, b = max(lo - r, 0), min(hi + r, nx)
    local = x.view(nx, layer)[a:b].reshape(-1).clone()
    out = torch.full(((hi - lo) * layer,), float("nan"), dtype=torch.float64, device="cuda")
    n = (ctypes.c_int64 * 3)(b - a, grid[1], grid[2])
    status = lib.vfem_box_filter_slab(n, a, nx, lo - a, hi - lo, r, _p(local), _p(out), transpose, _s())
    assert status == 0, lib.vfem_last_error()
    return out


@pytest.mark.parametrize("grid", [(13, 7, 9), (40, 16, 16)])
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_slab_filter_equals_the_whole_grid_slice_bitwise(grid, r):
    from ndr_amd import _lib
    lib = _lib.load()
    g = torch.Generator(device="cuda").manual_seed(5 + r)
    n = grid[0] * grid[1] * grid[2]
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    layer = grid[1] * grid[2]
    nx = grid[0]
    slabs = [(0, 4), (nx - 5, nx), (4, 9), (5, 6), (0, nx)]        # low end, high end, interior, one layer, whole grid
    for transpose in (0, 1):
        whole = _whole(lib, grid, r, x, transpose).view(nx, layer)
        for lo, hi in slabs:
            got = _slab(lib, grid, r, x, lo, hi, transpose)
            assert torch.equal(got, whole[lo:hi].reshape(-1)), (grid, r, transpose, lo, hi)


def test_slab_filter_refuses_inconsistent_calls():
    from ndr_amd import _lib
    lib = _lib.load()
    grid = (13, 7, 9)
    layer = grid[1] * grid[2]
    src = torch.zeros(13 * layer, dtype=torch.float64, device="cuda")
    dst = torch.zeros(13 * layer, dtype=torch.float64, device="cuda")

    def call(nl0, x_first, nxg, out_first, out_layers, r, ny=grid[1], nz=grid[2]):
        return lib.vfem_box_filter_slab((ctypes.c_int64 * 3)(nl0, ny, nz), x_first, nxg, out_first, out_layers, r, _p(src), _p(dst),
                                        0, _s())

    assert call(6, 3, 13, 1, 4, 1) == 0                 # layers 3..8 local, 4..7 written with one ghost layer each side
    torch.cuda.synchronize()
    assert call(6, 3, 13, 1, 4, 2) != 0                 # radius 2: layer 2 (in the grid) is not local
    assert call(6, 3, 13, 0, 4, 1) != 0                 # writing the first local layer needs layer 2
    assert call(6, 3, 13, 2, 4, 1) != 0                 # writing the last local layer needs layer 9
    assert call(6, 0, 13, 0, 5, 1) == 0                 # at the low end the grid boundary clips the neighbourhood
    assert call(6, 7, 13, 1, 5, 1) == 0                 # ... and at the high end
    torch.cuda.synchronize()
    assert call(6, 3, 13, 1, 4, -1) != 0                # negative radius
    assert call(6, 10, 13, 1, 4, 1) != 0                # local layers past the global grid
    assert call(6, -1, 13, 1, 4, 1) != 0                # local layers before it
    assert call(6, 3, 13, 1, 6, 1) != 0                 # output layers past the local layers
    assert call(6, 3, 13, -1, 4, 1) != 0                # output layers before them
    assert call(6, 3, 13, 1, -2, 1) != 0                # negative output count
    assert call(0, 3, 13, 0, 0, 1) != 0                 # empty slab
    assert call(6, 3, 13, 1, 4, 1, ny=0) != 0           # empty cross-section
    assert call(6, 3, 13, 1, 4, 2) != 0 and b"ghost" in lib.vfem_last_error()
