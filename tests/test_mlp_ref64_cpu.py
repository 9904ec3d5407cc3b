"""tests/mlp_ref64.py (the float64 restatement of networks.MLP that the GPU shape tests compare the kernels with) against the
numbers the modelled project itself produced: the forward outputs and the torch.autograd gradients of the five golden fixtures."""
import numpy as np
import pytest

import mlp_ref64
from test_mlp import FIXTURES, FULL, TOL_GRAD, _load, _load_full

# measured with this formulation: forward <= 3.7e-6 (fixtures are fp32, their own rounding), gradients <= 1.5e-6
TOL_FWD = 2e-5          # the oracle's bound (test_oracle_reproduces_reference_mlp)


@pytest.mark.parametrize("path", FIXTURES)
def test_ref64_reproduces_reference_fixture(path):
    z, es, nn_, nl, sig, Ws, bs = _load(path)
    r = mlp_ref64.run(z["coords"], z["B"], Ws, bs, sig, g_out=z["gout"])
    assert np.abs(r["out"] - z["out"].reshape(-1)).max() < TOL_FWD
    for i in range(nl):
        ew, eb = mlp_ref64.rel_l2(r["gW"][i], z["gW%d" % i]), mlp_ref64.rel_l2(r["gb"][i], z["gb%d" % i])
        assert ew < TOL_GRAD and eb < TOL_GRAD, (i, ew, eb)


def test_ref64_reproduces_reference_full_size_fixture():
    z, es, nn_, nl, B, Ws, bs = _load_full()
    r = mlp_ref64.run(z["coords"], B, Ws, bs, False, g_out=z["gout"])
    assert np.abs(r["out"] - z["out"].reshape(-1)).max() < TOL_FWD
    assert np.abs(mlp_ref64.run(z["coords"], B, Ws, bs, True)["out"] - z["out_sig"].reshape(-1)).max() < TOL_FWD
    stride = int(z["row_stride"][0])
    for i in range(nl):
        w = r["gW"][i][::stride] if r["gW"][i].shape[0] > 1 else r["gW"][i]
        ew, eb = mlp_ref64.rel_l2(w, z["gW%d" % i]), mlp_ref64.rel_l2(r["gb"][i], z["gb%d" % i])
        assert ew < TOL_GRAD and eb < TOL_GRAD, (i, ew, eb)


def test_float32_variant_and_mask():
    """dtype=float32 runs the same code in the fixtures' own precision; mask_below zeroes g_out exactly on the voxels whose
    smallest hidden |pre-activation| is below it, and those voxels then contribute nothing"""
    import torch
    z, es, nn_, nl, sig, Ws, bs = _load(FIXTURES[0])
    g = np.abs(z["gout"]).reshape(-1) + 0.5
    r32 = mlp_ref64.run(z["coords"], z["B"], Ws, bs, sig, g_out=g, dtype=torch.float32)
    r64 = mlp_ref64.run(z["coords"], z["B"], Ws, bs, sig, g_out=g)
    assert r32["out"].dtype == np.float32 and r64["out"].dtype == np.float64
    assert np.abs(r32["out"] - r64["out"]).max() < TOL_FWD
    cut = float(np.median(r64["min_pre"]))
    m = mlp_ref64.run(z["coords"], z["B"], Ws, bs, sig, g_out=g, mask_below=cut)
    gone = r64["min_pre"] < cut
    assert 0 < gone.sum() < gone.size
    assert np.array_equal(m["g_out"], np.where(gone, 0.0, g))
    by_hand = mlp_ref64.run(z["coords"], z["B"], Ws, bs, sig, g_out=np.where(gone, 0.0, g).astype(np.float32))
    for a, b in zip(m["gW"] + m["gb"], by_hand["gW"] + by_hand["gb"]):
        assert np.array_equal(a, b)
