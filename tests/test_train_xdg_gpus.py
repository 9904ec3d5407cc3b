"""training/train_xdg.py --gpus N and --checkpoint: the neural design loop over N slab ranks started by the driver itself (-m gpu: two
ranks sharing the one GPU, a gloo rehearsal) follows the one-GPU loss history and writes the one-GPU run's files; a run resumed from
a checkpoint continues where the full run went; the fused Adam state interchanges with torch.optim.Adam's; configurations without a
distributed form are argparse errors raised before any GPU work (CPU)."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "training", "train_xdg.py")
COMMON = ["--prob", "problems/3d/bridge.json", "--es", "64", "--nn", "64", "--nl", "4", "--sigma", "2", "--lr", "3e-3"]


def _driver(args, out, timeout=600, env=None):
    return subprocess.run([sys.executable, SCRIPT] + args + ["--out", out], cwd=ROOT, capture_output=True, text=True,
                          timeout=timeout, env=env)


_RUNS = {}


def _run(tmp_factory, gpus, args, jid="x"):
    """(loss history, files written, stderr) of one driver run; runs shared by several tests are made once"""
    key = (gpus, tuple(args))
    if key not in _RUNS:
        out = str(tmp_factory.mktemp("logs%d" % gpus))
        p = _driver(["--jid", jid, "--gpus", str(gpus)] + COMMON + list(args), out)
        assert p.returncode == 0, p.stderr[-4000:]
        wdir = os.path.join(out, "weights", "ff", jid)
        with open(os.path.join(wdir, jid + "_loss.json")) as fh:
            hist = json.load(fh)
        files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
        _RUNS[key] = (hist, files, p.stderr, wdir)
    return _RUNS[key]


def _assert_close(dist_hist, one_hist, first=2e-5, later=1e-4):
    assert len(dist_hist) == len(one_hist), (dist_hist, one_hist)
    for k, (a, b) in enumerate(zip(dist_hist, one_hist)):
        assert abs(a - b) <= (first if k == 0 else later) * abs(b), (k, dist_hist, one_hist)


@pytest.mark.gpu
@pytest.mark.parametrize("vcs", ["constrained_sigmoid", "maxed_barrier"])
def test_two_ranks_follow_the_one_gpu_history(tmp_path_factory, vcs):
    args = ["--grid", "[32, 16, 16]", "--mgl", "3", "--iter", "4", "--vcs", vcs]
    one, files1, _, _ = _run(tmp_path_factory, 1, args)
    two, files2, err, _ = _run(tmp_path_factory, 2, args)
    _assert_close(two, one)
    assert files2 == files1, (files1, files2)                  # rank 0 alone wrote, and wrote what one GPU writes
    assert err.count("Total Steps: 4,") == 1, err[-3000:]      # progress lines of rank 0 only
    assert "Step split over 2 ranks" in err


@pytest.mark.gpu
@pytest.mark.parametrize("mgl,path", [("3", "sharded"), ("1", "gathered")])
def test_both_density_paths_follow_the_one_gpu_history(tmp_path_factory, mgl, path):
    """[32, 16, 16] over two ranks: three levels leave two distributed ones (set_local_densities), one level none (the gather)"""
    args = ["--grid", "[32, 16, 16]", "--mgl", mgl, "--iter", "4", "--vcs", "constrained_sigmoid"]
    one = _run(tmp_path_factory, 1, args)[0]
    two, _, err, _ = _run(tmp_path_factory, 2, args)
    assert "Densities to the solver: " + path in err, err[-3000:]
    _assert_close(two, one)


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [1, 2])
def test_a_resumed_run_continues_the_full_run(tmp_path_factory, gpus):
    grid = ["--grid", "[32, 16, 16]", "--mgl", "3", "--vcs", "constrained_sigmoid"]
    full, files, _, _ = _run(tmp_path_factory, gpus, grid + ["--iter", "4", "--cs", "2"])
    assert [f for f in files if f.endswith(".pt")] == [os.path.join("weights", "ff", "x", "x_iter%d.pt" % k) for k in (2, 4)]
    _, _, _, wdir = _run(tmp_path_factory, gpus, grid + ["--iter", "2"])
    ckpt = os.path.join(wdir, "x_iter2.pt")
    resumed, rfiles, err, _ = _run(tmp_path_factory, gpus, grid + ["--iter", "4", "--checkpoint", ckpt])
    assert len(resumed) == 2 and "Total Steps: 3, Resolution Steps: 2" in err, err[-3000:]
    assert "x_iter1.pt" not in " ".join(rfiles)
    for a, b in zip(resumed, full[2:]):
        assert abs(a - b) <= 1e-3 * abs(b), (resumed, full)

    # what the driver loads is what was saved, bit for bit
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "training"))
    import train_xdg
    from ndr_amd.mlp import TrainableMLP
    saved = torch.load(ckpt, map_location="cuda")
    assert saved["step"] == 2 and saved["scale"] == 2.0
    net = TrainableMLP(3, 1, 64, 4, 64, 2.0)
    assert train_xdg.load_checkpoint(net, ckpt) == 2
    assert torch.equal(net.B, saved["B"])
    for k, v in net.state_dict().items():
        assert torch.equal(v, saved["model_state_dict"][k]), k
    mine, theirs = net.optimizer_state_dict(), saved["optim_state_dict"]
    assert sorted(mine["state"]) == sorted(theirs["state"]) == list(range(len(list(net.parameters()))))
    for i, st in theirs["state"].items():
        assert float(mine["state"][i]["step"]) == float(st["step"]) == 2.0
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(mine["state"][i][key], st[key]), (i, key)
    assert mine["param_groups"] == theirs["param_groups"]


def _toy_loss(net, target):
    d = net.forward_grid()
    return ((d - target) ** 2).mean()


@pytest.mark.gpu
def test_adam_state_interchanges_with_torch_adam(tmp_path):
    """the reference's checkpoint (torch.optim.Adam state) continues in the fused adam_step, and the fused state in torch.optim.Adam,
    with the next step as torch.optim.Adam takes it (the bound of the fused-Adam kernel test)"""
    from ndr_amd.mlp import TrainableMLP
    torch.manual_seed(3)
    side, hyper = (8, 8, 8), dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8)
    target = torch.rand(8 * 8 * 8, device="cuda")

    def make():
        net = TrainableMLP(3, 1, 64, 4, 64, 2.0)
        net.set_grid(side)
        return net

    def copy_weights(dst, src):
        dst.load_state_dict(src.state_dict())
        dst.B = src.B.clone()

    def max_diff(a, b):
        return max(float((p - q).detach().abs().max()) for p, q in zip(a.parameters(), b.parameters()))

    # reference -> fused
    ref = make()
    opt = torch.optim.Adam(ref.parameters(), **hyper)
    for _ in range(3):
        opt.zero_grad()
        _toy_loss(ref, target).backward()
        opt.step()
    path = str(tmp_path / "ref.pt")
    torch.save({"scale": ref.scale, "B": ref.B, "model_state_dict": ref.state_dict(), "step": 3,
                "optim_state_dict": opt.state_dict()}, path)
    d = torch.load(path, map_location="cuda")
    fused = make()
    fused.load_state_dict(d["model_state_dict"])
    fused.B = d["B"]
    fused.load_optimizer_state_dict(d["optim_state_dict"])
    assert fused._adam_t == 3
    opt.zero_grad()
    _toy_loss(ref, target).backward()
    for p, q in zip(fused.parameters(), ref.parameters()):
        p.grad = q.grad.clone()
    opt.step()
    fused.adam_step(**hyper)
    assert max_diff(fused, ref) < 2e-6

    # fused -> reference
    src = make()
    for _ in range(3):
        src.zero_grad()
        _toy_loss(src, target).backward()
        src.adam_step(**hyper)
    sd = src.optimizer_state_dict()
    assert sd["param_groups"][0]["lr"] == hyper["lr"] and tuple(sd["param_groups"][0]["betas"]) == hyper["betas"]
    path = str(tmp_path / "fused.pt")
    torch.save({"optim_state_dict": sd}, path)
    dst = make()
    copy_weights(dst, src)
    opt = torch.optim.Adam(dst.parameters(), **hyper)
    opt.load_state_dict(torch.load(path, map_location="cuda")["optim_state_dict"])
    src.zero_grad()
    _toy_loss(src, target).backward()
    for p, q in zip(dst.parameters(), src.parameters()):
        p.grad = q.grad.clone()
    src.adam_step(**hyper)
    opt.step()
    assert max_diff(dst, src) < 2e-6

    # state the fused update cannot continue is refused
    for change, what in ((lambda s: s["param_groups"][0].update(weight_decay=1e-4), "weight"),
                         (lambda s: s["param_groups"][0].update(amsgrad=True), "amsgrad"),
                         (lambda s: s["state"][0].update(exp_avg=torch.zeros(3)), "shape")):
        bad = torch.load(path, map_location="cuda")["optim_state_dict"]
        change(bad)
        with pytest.raises(ValueError, match=what):
            make().load_optimizer_state_dict(bad)


# ---- CPU: refusals before any GPU work ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [
    ["--gpus", "0", "--grid", "[32, 16, 16]"],
    ["--gpus", "2", "--prob", "problems/2d/mbb_beam.json", "--grid", "[64, 32]"],
    ["--gpus", "2", "--grid", "[32, 16, 16]", "--mgl", "0"],
    ["--gpus", "2", "--grid", "[33, 16, 16]"],
    ["--gpus", "8", "--grid", "[8, 16, 16]"],
    ["--gpus", "2", "--grid", "[32, 16, 16]", "--checkpoint", "no/such/checkpoint.pt"],
    ["--gpus", "1", "--grid", "[32, 16, 16]", "--checkpoint", "no/such/checkpoint.pt"],
])
def test_configurations_without_a_distributed_form_are_refused_before_gpu_work(tmp_path, args):
    out = str(tmp_path / "logs")
    prob = ["--prob", "problems/3d/bridge.json"] if "--prob" not in args else []
    p = _driver(["--iter", "1", "--sigma", "2"] + prob + args, out, 120)
    assert p.returncode == 2 and "error: --" in p.stderr, p.stderr
    assert not os.path.exists(out)


def test_degree_two_is_refused_before_gpu_work(tmp_path):
    with open(os.path.join(ROOT, "problems", "3d", "bridge.json")) as fh:
        cfg = json.load(fh)
    cfg["orderFEM"] = [2, 2, 2]
    for key in ("MATERIAL_PATH", "BC_PATH"):
        cfg[key] = os.path.join(ROOT, cfg[key])
    prob = tmp_path / "bridge_q2.json"
    prob.write_text(json.dumps(cfg))
    out = str(tmp_path / "logs")
    p = _driver(["--gpus", "2", "--iter", "1", "--sigma", "2", "--prob", str(prob), "--grid", "[32, 16, 16]"], out, 120)
    assert p.returncode == 2 and "--gpus 2 runs 3-D degree-[1, 1, 1]" in p.stderr, p.stderr
    assert not os.path.exists(out)


def test_a_rank_count_other_than_the_launchers_is_refused(tmp_path):
    out = str(tmp_path / "logs")
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = _driver(["--gpus", "2", "--iter", "1", "--sigma", "2", "--prob", "problems/3d/bridge.json", "--grid", "[32, 16, 16]"], out, 120,
                env=env)
    assert p.returncode == 2 and "does not match WORLD_SIZE 3" in p.stderr, p.stderr
    assert not os.path.exists(out)


# ---- CPU: the soft satisfiers on a field held in parts ------------------------------------------------------------------------------
def _soft_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ndr_amd import fem

    def allsum(t):
        t = t.detach().clone()
        dist.all_reduce(t)
        return t

    field = torch.rand(2 * 1000, generator=torch.Generator().manual_seed(5), dtype=torch.float32) * 0.9
    out = {}
    for mode in ("add_mean", "one_sided_max", "maxed_barrier", "thresholded_barrier"):
        x = field[rank * 1000:(rank + 1) * 1000].clone().requires_grad_(True)
        pen = fem.satisfy_volume_constraint(x, 0.3, compliance_loss=torch.tensor(7.0), constant=10.0, mode=mode,
                                            allsum=allsum)
        pen.backward()
        out[mode] = (pen.item(), x.grad.clone())
    q.put((rank, out))
    dist.destroy_process_group()


def test_soft_satisfiers_over_two_ranks_equal_the_whole_field():
    """the volume penalty of a field held by two ranks (one all-reduce of the local sum) and its gradient on each rank's part are
    those of the whole field; without allsum the function is the one-field form"""
    import torch.multiprocessing as mp
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import collect_from_ranks, free_port
    from ndr_amd import fem
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_soft_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(collect_from_ranks(q, procs))
    field = torch.rand(2 * 1000, generator=torch.Generator().manual_seed(5), dtype=torch.float32) * 0.9
    for mode in ("add_mean", "one_sided_max", "maxed_barrier", "thresholded_barrier"):
        x = field.clone().requires_grad_(True)
        pen = fem.satisfy_volume_constraint(x, 0.3, compliance_loss=torch.tensor(7.0), constant=10.0, mode=mode)
        pen.backward()
        for rank in (0, 1):
            value, grad = res[rank][mode]
            assert abs(value - pen.item()) <= 1e-6 * abs(pen.item()), (mode, value, pen.item())
            ref = x.grad[rank * 1000:(rank + 1) * 1000]
            assert torch.allclose(grad, ref, rtol=1e-5, atol=1e-12), (mode, float((grad - ref).abs().max()))
