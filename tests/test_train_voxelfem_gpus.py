"""training/train_voxelfem.py --gpus N: the ground-truth loop over N slab ranks started by the driver itself (-m gpu: two ranks sharing
the one GPU, a gloo rehearsal) writes the outputs of the one-GPU run and the same compliance history; configurations without a
distributed form are argparse errors raised before any GPU work (CPU)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "training", "train_voxelfem.py")


def _driver(args, out, timeout):
    return subprocess.run([sys.executable, SCRIPT] + args + ["--out", out], cwd=ROOT, capture_output=True, text=True, timeout=timeout)


@pytest.mark.gpu
def test_two_ranks_reproduce_the_one_gpu_history(tmp_path):
    common = ["--grid", "[32, 16, 16]", "--prob", "problems/3d/cantilever_flexion.json", "--v0", "0.5", "--mgl", "3", "--iter", "3"]
    hist = {}
    for gpus in (1, 2):
        out = str(tmp_path / ("logs%d" % gpus))
        p = _driver(["--jid", "g%d" % gpus, "--gpus", str(gpus)] + common, out, 600)
        assert p.returncode == 0, p.stderr[-4000:]
        loss = os.path.join(out, "loss", "gt", "g%d" % gpus)
        (name,) = os.listdir(loss)
        with open(os.path.join(loss, name)) as fh:
            hist[gpus] = json.load(fh)
        assert any(f.endswith(".vtr") for f in os.listdir(os.path.join(out, "densities", "gt", "g%d" % gpus)))
        assert "Total Steps: 2" in p.stderr
    assert len(hist[2]["compliance"]) == 3
    for key in ("final", "binary"):
        assert abs(hist[2][key] - hist[1][key]) <= 1e-8 * abs(hist[1][key]), (hist[1], hist[2])
    for a, b in zip(hist[2]["compliance"], hist[1]["compliance"]):
        assert abs(a - b) <= 1e-8 * abs(b), (hist[1], hist[2])


@pytest.mark.parametrize("args", [
    ["--prob", "problems/3d/cantilever_flexion.json", "--grid", "[32, 16, 16]", "--mgl", "0"],
    ["--prob", "problems/2d/mbb_beam.json", "--grid", "[64, 32]", "--mgl", "2"],
])
def test_configurations_without_a_distributed_form_are_refused_before_gpu_work(tmp_path, args):
    out = str(tmp_path / "logs")
    p = _driver(["--gpus", "2", "--iter", "1"] + args, out, 120)
    assert p.returncode == 2 and "--gpus 2" in p.stderr, p.stderr
    assert not os.path.exists(out)


def test_the_distributed_loop_refuses_what_it_cannot_decompose():
    sys.path.insert(0, ROOT)
    from ndr_amd.distributed_design import DistributedDesignLoop
    mat = os.path.join(ROOT, "VoxelFEM", "examples", "materials", "B9Creator.material")
    bc = os.path.join(ROOT, "bcs", "3d", "cantilever_flexion.bc")
    with pytest.raises(RuntimeError, match="3-D"):
        DistributedDesignLoop(mat, bc, [1, 1], [[0, 0], [2, 1]], [32, 16], 3, 0.5, 2)
    with pytest.raises(RuntimeError, match="degree"):
        DistributedDesignLoop(mat, bc, [2, 2, 2], [[0, 0, 0], [2, 1, 1]], [32, 16, 16], 3, 0.5, 2)
    with pytest.raises(RuntimeError, match="multigrid"):
        DistributedDesignLoop(mat, bc, [1, 1, 1], [[0, 0, 0], [2, 1, 1]], [32, 16, 16], 3, 0.5, 2, use_multigrid=False)
