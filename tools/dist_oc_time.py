"""Wall time per OC step of the distributed design loop (ndr_amd.distributed_design) split into solve, design update and
communication, next to fem.DesignLoop on the same grid.  With fewer devices than ranks the ranks share a device and
torch.distributed runs on gloo: a rehearsal of the code path, not a scaling measurement.
    python tools/dist_oc_time.py --ranks 2 --grid 128 64 64 --mgl 3 --steps 5 --warmup 2"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MATERIAL = os.path.join(ROOT, "VoxelFEM", "examples", "materials", "B9Creator.material")
BC = os.path.join(ROOT, "bcs", "3d", "cantilever_flexion.bc")
DOMAIN = [[0, 0, 0], [2, 1, 1]]


def _rank(rank, world, port, args, q):
    import torch
    import torch.distributed as dist
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "WORLD_SIZE": str(world)})
    torch.cuda.set_device(rank % torch.cuda.device_count())
    from ndr_amd import distributed, distributed_design
    distributed.init_process_group_from_env()
    loop = distributed_design.DistributedDesignLoop(MATERIAL, BC, [1, 1, 1], DOMAIN, args.grid, 3, 0.5, args.mgl)
    loop.seed()
    for _ in range(args.warmup):
        loop.step()
    for k in loop.timers:
        loop.timers[k] = 0.0
    dist.barrier()
    torch.cuda.synchronize()
    clock = time.perf_counter()
    for _ in range(args.steps):
        loop.step()
    torch.cuda.synchronize()
    total = time.perf_counter() - clock
    q.put(dict(rank=rank, backend=dist.get_backend(), step_ms=1e3 * total / args.steps,
               **{k + "_ms": 1e3 * v / args.steps for k, v in loop.timers.items()},
               pcg_iterations=loop.pcg_iterations[-args.steps:], probes=loop.probes[-args.steps:]))
    dist.destroy_process_group()


def _single(args):
    import torch
    from ndr_amd import fem, pyVoxelFEM as pv
    loop = fem.DesignLoop(MATERIAL, BC, [1, 1, 1], DOMAIN, args.grid, 3, 0.5, args.mgl)
    solve = [0.0]
    update = loop.objective.updateCache

    def timed(x):
        torch.cuda.synchronize()
        t = time.perf_counter()
        update(x)
        torch.cuda.synchronize()
        solve[0] += time.perf_counter() - t

    loop.objective.updateCache = timed
    loop.seed()
    oc = pv.OCOptimizer(loop.problem)
    for _ in range(args.warmup):
        oc.step()
    solve[0] = 0.0
    torch.cuda.synchronize()
    clock = time.perf_counter()
    for _ in range(args.steps):
        oc.step()
    torch.cuda.synchronize()
    total = time.perf_counter() - clock
    return dict(step_ms=1e3 * total / args.steps, solve_ms=1e3 * solve[0] / args.steps,
                update_ms=1e3 * (total - solve[0]) / args.steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--grid", type=int, nargs=3, default=[128, 64, 64])
    ap.add_argument("--mgl", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--single", action="store_true", help="in this process: fem.DesignLoop on the same grid")
    args = ap.parse_args()
    if args.single:
        print(json.dumps(dict(mode="DesignLoop", grid=args.grid, **_single(args))))
        return
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, args.ranks, port, args, q)) for r in range(args.ranks)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=1800) for _ in procs], key=lambda r: r["rank"])
    for p in procs:
        p.join()
    for r in res:
        print(json.dumps(dict(mode="DistributedDesignLoop", ranks=args.ranks, grid=args.grid, **r)))


if __name__ == "__main__":
    main()
