"""bench.py's plain run: the headline line and --dump-outputs only; every side measurement is behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import ROOT

BENCH = os.path.join(ROOT, "bench.py")
SIDE_KEYS = ("roofline", "spmv_other_grids", "cg_mg", "mlp_forward", "degree2_cg_mg", "degree2_spmv", "rank_proxy", "cpu_baseline")


def test_rank_proxy_needs_full():
    r = subprocess.run([sys.executable, BENCH, "--rank-proxy", "8"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stderr
    assert "--full" in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    import torch
    from helpers import make_hip
    ne, steps, warmup = (32, 16, 16), 3, 2
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--grid", *map(str, ne), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["unit"] == "GVoxel/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["metric"].startswith("matrix-free SpMV GVoxel/s (Q1 fp64, 32x16x16)")
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (steps, warmup, 1)
    assert line["value"] == pytest.approx(np.prod(ne) / (line["ms_per_step"] * 1e-3) / 1e9, rel=1e-9)
    assert not [k for k in SIDE_KEYS if k in line]
    assert line["dumped_outputs"]["arrays"] == {"Ku": [int(np.prod(np.array(ne) + 1)), 3]}

    # the dumped Ku is K(rho) u of bench.py's seeded inputs
    tps = make_hip(ne, ([0, 0, 0], [1, 1, 1]), None, None, v0=0.5)
    g = torch.Generator(device="cuda").manual_seed(88)
    tps.setElementDensities(torch.rand(tps.numElements(), dtype=torch.float64, device="cuda", generator=g))
    u = torch.randn((tps.numNodes(), 3), dtype=torch.float64, device="cuda", generator=g)
    ref = tps.applyK(u)
    ku = np.load(os.path.join(str(tmp_path), "Ku.npy"))
    assert np.abs(ku - ref).max() <= 1e-12 * np.abs(ref).max()
