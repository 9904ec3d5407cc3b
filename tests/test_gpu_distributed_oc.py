"""-m gpu: the ground-truth OC design loop over x-slab ranks (ndr_amd.distributed_design.DistributedDesignLoop; ranks sharing the
one GPU, gloo) walks the same optimisation as the single-process fem.DesignLoop: same PCG iterations, the same bisection (probe
count, multiplier), the same compliance, densities and thresholded compliance; and the design update exchanges a fixed number of
element-layer messages per step, whatever the number of probes."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
STEPS = 5


def _single(bc, corners, ne, levels, radius, beta):
    """fem.DesignLoop as fem.ground_truth_topopt drives it (seed, then OC steps with one persistent optimiser), recording what
    DesignLoop.run does not expose: PCG iterations, probes and the multiplier of every step"""
    from helpers import MATERIAL
    from ndr_amd import fem, pyVoxelFEM as pv
    loop = fem.DesignLoop(MATERIAL, bc, [1, 1, 1], corners, list(ne), 3, 0.5, levels)
    loop.problem.filters[0].radius = radius
    loop.problem.filters[1].beta = beta
    probes = [0]
    evaluate = loop.problem.evaluateOCConstraintAtVars_dev

    def counted(x):
        probes[0] += 1
        return evaluate(x)

    loop.problem.evaluateOCConstraintAtVars_dev = counted
    loop.seed()
    its, lams, nprobe, hist = [loop.objective.mg.last_iterations], [], [], []
    oc = pv.OCOptimizer(loop.problem)
    for _ in range(STEPS):
        hist.append(loop.compliance())
        probes[0] = 0
        oc.step()
        nprobe.append(probes[0])
        lams.append(0.5 * (oc._lmin + oc._lmax))         # the accepted multiplier is the midpoint of the kept bracket
        its.append(loop.objective.mg.last_iterations)
    rho = loop.tps.getDensities()
    return dict(hist=hist, its=its, lams=lams, probes=nprobe, rho=rho, thr=loop.thresholded_compliance())


def _worker(rank, world, port, ne, levels, bc, corners, radius, beta, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from helpers import MATERIAL
    from ndr_amd.distributed_design import DistributedDesignLoop
    loop = DistributedDesignLoop(MATERIAL, bc, [1, 1, 1], corners, list(ne), 3, 0.5, levels)
    loop.radius, loop.beta = radius, beta
    loop.seed()
    msgs = []
    for _ in range(STEPS):
        m0 = loop.messages
        loop.run(1)
        msgs.append(loop.messages - m0)
    rho = loop.gather_densities(0)
    owned = loop.owned_densities().cpu().numpy()
    first, count = loop.ds.owned_element_range()
    thr = loop.thresholded_compliance()
    loop.radius = 10 ** 6
    try:
        loop.seed()
        refused = None
    except RuntimeError as e:
        refused = str(e)
    out = dict(rank=rank, hist=list(loop.history), its=loop.pcg_iterations[1:2 + STEPS], lams=list(loop.lambdas),
               probes=list(loop.probes), msgs=msgs, owned=owned, first=first, count=count, thr=thr, refused=refused,
               neighbours=(rank > 0) + (rank < world - 1))
    if rank == 0:
        out["rho"] = rho
        out["single"] = _single(bc, corners, ne, levels, radius, beta)
    q.put(out)
    dist.destroy_process_group()


def _run(world, target, args):
    from helpers import collect_from_ranks, free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + args + (q,)) for r in range(world)]
    for p in procs:
        p.start()
    return sorted(collect_from_ranks(q, procs, timeout=600), key=lambda r: r["rank"])


CANTILEVER = ("bcs/3d/cantilever_flexion.bc", [[0, 0, 0], [2, 1, 1]])
BRIDGE = ("bcs/3d/bridge.bc", [[0, 0, 0], [2, 1, 1]])


@pytest.mark.parametrize("world,ne,levels,problem,radius,beta", [
    (2, (32, 16, 16), 3, CANTILEVER, 1, 1.0),
    (2, (32, 16, 16), 3, BRIDGE, 1, 1.0),
    (3, (48, 16, 16), 3, CANTILEVER, 1, 1.0),
    (3, (48, 16, 16), 3, BRIDGE, 2, 4.0),
])
def test_distributed_oc_loop_walks_the_single_process_optimisation(world, ne, levels, problem, radius, beta):
    bc, corners = os.path.join(ROOT, problem[0]), problem[1]
    res = _run(world, _worker, (ne, levels, bc, corners, radius, beta))
    s = res[0]["single"]
    assert len(s["hist"]) == STEPS and s["hist"][-1] < s["hist"][0]
    for r in res:
        assert r["its"] == s["its"], (r["its"], s["its"])
        assert r["probes"] == s["probes"], (r["probes"], s["probes"])
        for a, b in zip(r["lams"], s["lams"]):
            assert abs(a - b) <= 1e-12 * abs(b), (r["lams"], s["lams"])
        for a, b in zip(r["hist"], s["hist"]):
            assert abs(a - b) <= 1e-8 * abs(b), (r["hist"], s["hist"])
        assert abs(r["thr"] - s["thr"]) <= 1e-8 * abs(s["thr"]), (r["thr"], s["thr"])
        assert np.abs(r["owned"] - s["rho"][r["first"]:r["first"] + r["count"]]).max() <= 1e-8
        # the design update's element-layer messages: the same every step (they do not grow with the probes), at most three
        # exchanges per neighbour
        assert len(set(r["msgs"])) == 1 and r["msgs"][0] <= 3 * r["neighbours"], (r["msgs"], r["probes"])
        assert r["refused"] is not None and "radius" in r["refused"]
    rho = res[0]["rho"]
    assert rho.shape == s["rho"].shape and np.abs(rho - s["rho"]).max() <= 1e-8
    assert abs(1.0 - rho.mean() / 0.5) <= 1e-6 * (1 + 1e-6)          # final volume within the bisection's ctol


def _refusal_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from helpers import BC_CANTILEVER, MATERIAL
    from ndr_amd.distributed_design import DistributedDesignLoop
    try:          # one multigrid level: no level below the distributed one holds element matrices, so densities cannot be sharded
        DistributedDesignLoop(MATERIAL, BC_CANTILEVER, [1, 1, 1], [[0, 0, 0], [2, 1, 1]], [32, 16, 16], 3, 0.5, 1)
        msg = None
    except RuntimeError as e:
        msg = str(e)
    q.put(dict(rank=rank, msg=msg))
    dist.destroy_process_group()


def test_slabs_that_cannot_take_sharded_densities_are_refused_with_the_solvers_message():
    for r in _run(2, _refusal_worker, ()):
        assert r["msg"] is not None and "sharded densities" in r["msg"], r
