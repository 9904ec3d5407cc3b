"""The MLP kernels (kernels_mlp.hip, kernels_mlp_x3.hip, kernels_mlp_bwd.hip, host side mlp.hip) against the float64 restatement
of networks.MLP in tests/mlp_ref64.py, at the sizes the golden fixtures (<= 256 voxels, widths 32 .. 256 and 512) do not reach:
several pipeline stages and 16 / 32 / 128 voxel slices of the weight-gradient kernel, partial second tiles of its 256 x 256 output
tile, hidden widths and embedding sizes that are no power of two, two chunks with accumulation, the block edges, and the grid entry
points on grids whose fp32 coordinates are exact.

Gradients are taken with a positive g_out that the reference zeroes on voxels with a hidden unit within 2e-5 of its ReLU kink
(mlp_ref64.py says why); the share of such voxels is asserted to stay below 8 %."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mlp_ref64  # noqa: E402
from test_mlp import TOL_F16, TOL_F32, TOL_GRAD  # noqa: E402

MAX_MASKED = 0.08
# every dW / db in relative L2 against the float64 reference: max(TOL_GRAD, 4 e32), e32 the error of the reference's own float32
# run on the same inputs (4: another summation order and the dropped lo x lo products).
# Measured maxima on an MI355X ("Shapes beyond the fixtures"): first-layer dW 1.15e-6 (case D), hidden dW
# 5.0e-7, output-layer dW 5.4e-7, hidden db 2.1e-7, output db 1.0e-7; grid entry points 8.0e-7; e32 between 1e-8 and 3.6e-6 (case C,
# 2^20 voxels), so the kernels sit at about 1 x e32 on the first layer and the bound is TOL_GRAD itself nearly everywhere.
# Forward: fp32 mode 2.2e-6 (the reference's float32 run: 2.4e-6), fp16 mode 7.5e-4.
E32_FACTOR = 4.0
TOL_TERMS1 = 2e-3        # set_backward_terms(1), the bound of test_hip_mlp_gradients_match_reference_autograd

# id: (es, nn, layers, sigma, sigmoid, voxels, seed).  What each reaches: see DESIGN.md section 3.5
CASES = {
    "A": (96, 288, 4, 3.0, False, 4097, 101),
    "B": (160, 480, 3, 4.0, True, 2049, 102),
    "C": (32, 32, 3, 1.0, True, (1 << 20) + 777, 103),
    "D": (1024, 512, 4, 4.0, False, 1025, 104),
    "E": (64, 96, 2, 2.0, False, 16385, 105),
    "F": (128, 352, 5, 2.0, True, 8191, 106),
    "G": (160, 512, 3, 2.0, False, 16384, 107),
    "H1": (64, 64, 3, 2.5, True, 1, 108),
    "H63": (64, 64, 3, 2.5, True, 63, 108),
    "H64": (64, 64, 3, 2.5, True, 64, 108),
    "H65": (64, 64, 3, 2.5, True, 65, 108),
    "H257": (64, 64, 3, 2.5, True, 257, 108),
}
GRIDS = {"g33": (33, 17, 9), "g65": (65, 1, 33)}          # n - 1 a power of two: lo + i step is exact in fp32; g65 has gstep = 0
GRID_CASES = [("A", "g33"), ("A", "g65"), ("B", "g33"), ("B", "g65"), ("D", "g65")]
_deltas = {}


def _weights(case):
    from helpers import seeded_mlp_weights
    es, nn_, nl, sigma, sig, nvox, seed = CASES[case]
    return seeded_mlp_weights(es, nn_, nl, sigma, seed)


def _reference_on(case, coords):
    """float64 forward on all voxels, float64 and float32 gradients with the masked positive g_out; e32 per tensor"""
    import torch
    es, nn_, nl, sigma, sig, _, seed = CASES[case]
    B, Ws, bs = _weights(case)
    nvox = coords.shape[0]
    g = np.random.default_rng(seed + 7000).uniform(0.5, 1.5, size=nvox).astype(np.float32)
    r64 = mlp_ref64.run(coords, B, Ws, bs, sig, g_out=g, mask_below=mlp_ref64.DELTA)
    gm = r64["g_out"].astype(np.float32)
    masked = float((gm == 0).mean())
    r32 = mlp_ref64.run(coords, B, Ws, bs, sig, g_out=gm, dtype=torch.float32)
    e32 = [mlp_ref64.rel_l2(a, b) for a, b in zip(r32["gW"] + r32["gb"], r64["gW"] + r64["gb"])]
    return {"coords": coords, "out": r64["out"], "g_out": gm, "masked": masked, "grads": r64["gW"] + r64["gb"], "e32": e32,
            "fwd32": float(np.abs(r32["out"] - r64["out"]).max())}


@functools.lru_cache(maxsize=None)
def reference(case):
    """explicit coordinates, uniform in [0, 1]^3"""
    nvox, seed = CASES[case][5], CASES[case][6]
    coords = np.random.default_rng(seed + 5000 + nvox).uniform(0.0, 1.0, size=(nvox, 3)).astype(np.float32)
    return _reference_on(case, coords)


@functools.lru_cache(maxsize=None)
def grid_reference(case, grid):
    from oracle import vfem_oracle as vo
    return _reference_on(case, vo.get_mgrid(GRIDS[grid]).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def grid_range_reference(case, grid):
    """the voxels [first, first + count) of the grid: starts and ends inside a 64-voxel block"""
    from oracle import vfem_oracle as vo
    first, count = grid_range(grid)
    return _reference_on(case, vo.get_mgrid(GRIDS[grid]).reshape(-1, 3)[first:first + count])


def grid_range(grid):
    plane = GRIDS[grid][1] * GRIDS[grid][2]
    return plane * 3 + 13, plane * 20 + 5           # g33: 17 9 3 + 13 and 17 9 20 + 5


def _model(case):
    import torch
    from ndr_amd.mlp import MLP
    es, nn_, nl, sigma, sig, _, _ = CASES[case]
    m = MLP(3, 1, nn_, nl, es, sigma, output_act=torch.nn.Sigmoid() if sig else None)
    m.load_arrays(*_weights(case))
    return m


def _check_gradients(tag, ref, gw, gb):
    """every dW, db of the kernels against the float64 reference; records the errors beside the reference's own float32 error"""
    from helpers import record_deltas
    assert ref["masked"] <= MAX_MASKED and (ref["g_out"] != 0).any(), ref["masked"]
    errs = [mlp_ref64.rel_l2(t.cpu().numpy(), r) for t, r in zip(gw + gb, ref["grads"])]
    nl = len(gw)
    names = ["dW%d" % i for i in range(nl)] + ["db%d" % i for i in range(nl)]
    _deltas[tag] = {"masked_share": ref["masked"], "kernel": dict(zip(names, errs)), "ref_float32": dict(zip(names, ref["e32"]))}
    record_deltas("mlp_shapes", _deltas)
    print(tag, _deltas[tag])
    for name, e, e32 in zip(names, errs, ref["e32"]):
        assert e <= max(TOL_GRAD, E32_FACTOR * e32), (tag, name, e, e32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_matches_fp64_reference(case):
    """precision "fp32" (split operands) and "fp16" through the explicit-coordinate entry point, every voxel"""
    import torch
    from helpers import record_deltas
    ref = reference(case)
    m = _model(case)
    x = torch.from_numpy(ref["coords"]).cuda()
    err = {}
    for precision in ("fp32", "fp16"):
        m.precision = precision
        got = m.forward(x).cpu().numpy().reshape(-1)
        assert got.shape == ref["out"].shape
        err[precision] = float(np.abs(got - ref["out"]).max())
    err["ref_float32"] = ref["fwd32"]
    _deltas["forward_" + case] = err
    record_deltas("mlp_shapes", _deltas)
    print(case, err)
    assert err["fp32"] <= TOL_F32, err
    assert err["fp16"] <= TOL_F16, err


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_gradients_match_fp64_reference(case):
    import torch
    ref = reference(case)
    m = _model(case)
    x, g = torch.from_numpy(ref["coords"]).cuda(), torch.from_numpy(ref["g_out"]).cuda()
    gw, gb = m.backward(x, g)
    _check_gradients("backward_" + case, ref, gw, gb)
    if case in ("A", "B"):
        m.set_backward_terms(1)
        gw, gb = m.backward(x, g)
        nl = len(gw)
        for i in range(nl):
            e = mlp_ref64.rel_l2(gw[i].cpu().numpy(), ref["grads"][i])
            assert e <= TOL_TERMS1, (case, i, e)


@pytest.mark.gpu
@pytest.mark.parametrize("case,grid", GRID_CASES)
def test_grid_entry_points_match_fp64_reference(case, grid):
    """forward_grid / backward_grid and the voxel-range entry points against the reference on oracle.get_mgrid's coordinates, at the
    bounds of the explicit-coordinate entry points; the float64 copy; the kept first layer (cases A, B, D)"""
    import torch
    from helpers import record_deltas
    side = GRIDS[grid]
    ref = grid_reference(case, grid)
    m = _model(case)
    nvox = int(np.prod(side))
    o64 = torch.empty(nvox, dtype=torch.float64, device="cuda")
    out = m.forward_grid(side, out_f64=o64).reshape(-1)
    assert torch.equal(o64, out.double())
    err = {"grid": float(np.abs(out.cpu().numpy() - ref["out"]).max())}
    g = torch.from_numpy(ref["g_out"]).cuda()
    gw, gb = m.backward_grid(side, g)
    _check_gradients("backward_grid_%s_%s" % (case, grid), ref, gw, gb)
    recomputed = [t.clone() for t in gw + gb]
    # the kept first layer: forward, then backward of the same grid -- bit for bit the recomputed gradients
    m.set_keep_first_layer(True)
    assert torch.equal(m.forward_grid(side).reshape(-1), out)
    kw, kb = m.backward_grid(side, g)
    for a, b in zip(kw + kb, recomputed):
        assert torch.equal(a, b)
    m.set_keep_first_layer(False)
    # a voxel range that starts and ends inside a 64-voxel block
    first, count = grid_range(grid)
    assert first % 64 and (first + count) % 64 and first + count < nvox
    rref = grid_range_reference(case, grid)
    o64 = torch.empty(count, dtype=torch.float64, device="cuda")
    part = m.forward_grid_range(side, first, count, out_f64=o64)
    assert torch.equal(o64, part.double())
    err["range"] = float(np.abs(part.cpu().numpy() - rref["out"]).max())
    gr = torch.from_numpy(rref["g_out"]).cuda()
    rw, rb = m.backward_grid_range(side, first, count, gr)
    _check_gradients("backward_grid_range_%s_%s" % (case, grid), rref, rw, rb)
    recomputed = [t.clone() for t in rw + rb]
    m.set_keep_first_layer(True)
    assert torch.equal(m.forward_grid_range(side, first, count), part)
    kw, kb = m.backward_grid_range(side, first, count, gr)
    for a, b in zip(kw + kb, recomputed):
        assert torch.equal(a, b)
    _deltas["forward_grid_%s_%s" % (case, grid)] = err
    record_deltas("mlp_shapes", _deltas)
    print(case, grid, err)
    assert max(err.values()) <= TOL_F32, err


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, (1 << 20) + 3])
def test_fused_adam_block_edges(n):
    """three vfem_adam_step updates against torch.optim.Adam on float64 CPU parameters"""
    import torch
    from ndr_amd import _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    ref = torch.nn.Parameter(p0.double())
    opt = torch.optim.Adam([ref], lr=3e-3, betas=(0.9, 0.99), eps=1e-8)
    p = p0.clone().cuda()
    mm, vv = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 4):
        g = torch.randn(n, generator=gen) * (1.0 + step)
        ref.grad = g.double()
        opt.step()
        gd = g.cuda()
        _lib.check(lib.vfem_adam_step(n, ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(gd.data_ptr()), ctypes.c_void_p(mm.data_ptr()),
                                      ctypes.c_void_p(vv.data_ptr()), 3e-3, 0.9, 0.99, 1e-8, step, None))
    torch.cuda.synchronize()
    assert float((p.cpu().double() - ref.detach()).abs().max()) < 2e-6
