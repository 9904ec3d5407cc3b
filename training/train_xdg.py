#!/usr/bin/env python3
"""Neural density field (Fourier-feature MLP) trained against the compliance solve on the MI355X path: the command line of the
reference's training/train_xdg.py for the flags that matter to the hot path (--jid --grid --prob --v0 --mgl --vcs --es --nn --nl
--lr --iter --cs --sigma --checkpoint; run from the repository root).  Every step: MLP logits -> volume-constraint satisfier ->
compliance through the multigrid-PCG solve (autograd node with the device sensitivities) -> backward through the MLP -> Adam.
    python training/train_xdg.py --jid demo --grid "[64, 32, 32]" --prob problems/3d/bridge.json --v0 0.4 --mgl 3 --sigma 3 --iter 50
The filters of the reference's closure (kornia Gaussian smoothing etc.) are out of scope and not applied.
--gpus N > 1 runs the same loop over N x-slab ranks (ndr_amd.distributed_xdg; 3-D, degree 1, multigrid): without a launcher this
process starts N fresh rank processes and never touches the GPU itself; under torch.distributed.run the environment is used.
Rank 0 writes the outputs.  --checkpoint resumes from a checkpoint of this driver or of the reference (utils.save_weights)."""
import argparse
import ast
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--jid', default='run')
    ap.add_argument('--grid', help='grid dimensions as a list, e.g. "[64, 32, 32]" (default: the problem file\'s)')
    ap.add_argument('--prob', required=True)
    ap.add_argument('--v0', help='volume fraction (default: the problem file\'s)')
    ap.add_argument('--mgl', default=2)
    ap.add_argument('--vcs', default='constrained_sigmoid', help='volume-constraint satisfier (fem.satisfy_volume_constraint modes)')
    ap.add_argument('--es', default=1024, help='Fourier features (embedding size)')
    ap.add_argument('--nn', default=512, help='neurons per hidden layer')
    ap.add_argument('--nl', default=4, help='layers')
    ap.add_argument('--lr', default=3e-4)
    ap.add_argument('--iter', default=5000)
    ap.add_argument('--cs', default=100, help='a weight checkpoint every iter/cs steps')
    ap.add_argument('--sigma', required=True, help='scale of the Fourier-feature Gaussian')
    ap.add_argument('--out', default='logs')
    ap.add_argument('--mlp_precision', default='fp32', choices=['fp16', 'fp32'],
                    help='fp32: the reference network\'s precision (fused kernel with split fp16 operands); fp16: plain fp16 operands, 3x faster')
    ap.add_argument('--gpus', type=int, default=1, help='ranks of the x-slab decomposition (3-D degree-1 multigrid problems; 1: one GPU)')
    ap.add_argument('--checkpoint', help='checkpoint to resume from (weights, B, scale; step and Adam state when present)')
    args = ap.parse_args(argv)

    with open(args.prob) as fh:
        cfg = json.load(fh)
    grid = tuple(ast.literal_eval(args.grid)) if args.grid else tuple(cfg['gridDimensions'])
    v0 = float(args.v0) if args.v0 is not None else cfg['maxVolume'][0]
    if args.checkpoint is not None and not os.path.isfile(args.checkpoint):
        ap.error('--checkpoint {}: no such file'.format(args.checkpoint))
    if args.gpus < 1:
        ap.error('--gpus must be at least 1')
    if args.gpus > 1:
        _refuse_undecomposable(ap, args, cfg, grid)
        if 'WORLD_SIZE' not in os.environ:
            from ndr_amd.distributed import launch_ranks
            launch_ranks(args.gpus, main, list(sys.argv[1:] if argv is None else argv))
            with open(os.path.join(args.out, 'weights', 'ff', str(args.jid), '{}_loss.json'.format(args.jid))) as fh:
                return json.load(fh)              # what rank 0 wrote
        if int(os.environ['WORLD_SIZE']) != args.gpus:
            ap.error('--gpus {} does not match WORLD_SIZE {}'.format(args.gpus, os.environ['WORLD_SIZE']))
        return _train_ranks(args, cfg, grid, v0)
    from ndr_amd import fem, pyVoxelFEM

    torch.manual_seed(cfg.get('seed', 88))
    hard = fem.type_of_volume_constaint_satisfier(args.vcs)
    tps = fem.initializeTensorProductSimulator(cfg['orderFEM'], cfg['domainCorners'], list(grid), v0, 1, 1e-4, 3,
                                               cfg['MATERIAL_PATH'], cfg['BC_PATH'])          # train_xdg forces SIMP exponent 3
    objective = pyVoxelFEM.MultigridComplianceObjective(tps.multigridSolver(int(args.mgl)))
    for name, value in fem.DesignLoop.SOLVER.items():
        setattr(objective, name, value)
    top = pyVoxelFEM.TopologyOptimizationProblem(tps, objective, [pyVoxelFEM.TotalVolumeConstraint(v0)], [])
    net = _network(args, hard)
    net.set_grid(grid)
    fem.homogeneous_init(net, v0)
    first = 0 if args.checkpoint is None else load_checkpoint(net, args.checkpoint)
    max_volume = torch.tensor(v0, device="cuda")
    steps, every = int(args.iter), _every(args)
    wdir = os.path.join(args.out, 'weights', 'ff', str(args.jid))
    os.makedirs(wdir, exist_ok=True)
    history, start = [], time.perf_counter()
    for step in range(first, steps):
        net.zero_grad()
        density = net.forward_grid().view(grid)
        if hard:
            density = fem.satisfy_volume_constraint(density, max_volume, mode=args.vcs)
        else:
            density = torch.clamp(density, 0.0, 1.0)
        loss = fem.VoxelFEMFunction.apply(density.flatten(), top)
        if not hard:
            loss = loss + fem.satisfy_volume_constraint(density, max_volume, compliance_loss=loss.detach(), scaler_mode='clip',
                                                        constant=1500, mode=args.vcs)
        loss.backward()
        net.adam_step(lr=float(args.lr))
        history.append(float(loss.detach()))
        _progress(step, history[-1])
        if (step + 1) % every == 0 or step + 1 == steps:
            save_checkpoint(net, step + 1, os.path.join(wdir, '{}_iter{}.pt'.format(args.jid, step + 1)))
    with open(os.path.join(wdir, '{}_loss.json'.format(args.jid)), 'w') as fh:
        json.dump(history, fh)
    sys.stderr.write('\nOverall runtime: {}\n'.format(time.perf_counter() - start))
    return history


def _network(args, hard):
    from ndr_amd.mlp import TrainableMLP
    net = TrainableMLP(3, 1, int(args.nn), int(args.nl), int(args.es), float(args.sigma),
                       output_act=None if hard else torch.nn.Sigmoid())
    net.kernel.precision = args.mlp_precision
    return net


def _every(args):
    return max(1, int(args.iter) // max(1, int(args.cs)))


def _progress(step, loss):
    sys.stderr.write('Total Steps: {:d}, Resolution Steps: {:d}, Compliance loss {:.6f}\n'.format(step + 1, step, loss))


def save_checkpoint(net, step, path):
    """utils.save_weights with a step (the reference's intermediate checkpoints): weights, B, scale, step, Adam state"""
    torch.save({'model_state_dict': net.state_dict(), 'B': net.B, 'step': step, 'scale': net.scale,
                'optim_state_dict': net.optimizer_state_dict()}, path)


def load_checkpoint(net, path):
    """utils.load_weights: weights, B and scale, and when the checkpoint has them the step and the Adam state; returns the step
    to continue from (0 without one)"""
    d = torch.load(path, map_location=torch.device('cuda', torch.cuda.current_device()))
    net.load_state_dict(d['model_state_dict'])
    net.B = d['B'].to(device=net.B.device, dtype=net.B.dtype)
    if 'scale' in d:
        net.scale = d['scale']
    if 'step' not in d:
        return 0
    if 'optim_state_dict' in d:
        net.load_optimizer_state_dict(d['optim_state_dict'])
    return int(d['step'])


def _refuse_undecomposable(ap, args, cfg, grid):
    """configurations without a distributed form: argparse errors, raised before any GPU work or output"""
    from ndr_amd.distributed import SlabPartition, auto_dist_levels, DistributedMGSolver
    levels = int(args.mgl)
    if levels < 1:
        ap.error('--gpus {} needs the multigrid objective (--mgl >= 1): the direct solve has no distributed form'.format(args.gpus))
    if len(grid) != 3 or list(cfg['orderFEM']) != [1, 1, 1]:
        ap.error('--gpus {} runs 3-D degree-[1, 1, 1] problems only (grid {}, orderFEM {})'.format(args.gpus, list(grid), cfg['orderFEM']))
    ld = auto_dist_levels(int(grid[0]), args.gpus, levels, DistributedMGSolver.MIN_LAYERS)
    try:
        SlabPartition(grid, args.gpus, 0, align=2 ** (ld + 1))
        if ld + 1 > levels:
            raise RuntimeError('needs at least one replicated multigrid level below the distributed ones')
    except RuntimeError as e:
        ap.error('--gpus {}: the x extent {} cannot be split into slabs ({})'.format(args.gpus, grid[0], e))


def _train_ranks(args, cfg, grid, v0):
    """this process is one rank (environment of torch.distributed.run or of distributed.launch_ranks): the loop of main on the slabs;
    rank 0 prints and writes what the one-GPU run writes"""
    import torch.distributed as dist
    from ndr_amd import distributed, fem
    from ndr_amd.distributed_xdg import DistributedXdgLoop
    torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count())
    distributed.init_process_group_from_env()       # nccl with a device per rank, gloo when the ranks share a device (rehearsal)
    try:
        rank = dist.get_rank()
        log = sys.stderr if rank == 0 else None
        torch.manual_seed(cfg.get('seed', 88))
        hard = fem.type_of_volume_constaint_satisfier(args.vcs)
        loop = DistributedXdgLoop(cfg['MATERIAL_PATH'], cfg['BC_PATH'], cfg['orderFEM'], cfg['domainCorners'], grid, v0, int(args.mgl),
                                  vcs=args.vcs, log=log)
        net = _network(args, hard)
        fem.homogeneous_init(net, v0)
        loop.attach(net)                             # parameters and B of rank 0 on every rank
        first = 0
        if args.checkpoint is not None:
            first = load_checkpoint(net, args.checkpoint)
            loop.broadcast_parameters()
        steps, every = int(args.iter), _every(args)
        wdir = os.path.join(args.out, 'weights', 'ff', str(args.jid))
        if rank == 0:
            os.makedirs(wdir, exist_ok=True)
        history, start = [], time.perf_counter()
        for step in range(first, steps):
            history.append(loop.step(args.lr))
            if rank == 0:
                _progress(step, history[-1])
            if (step + 1) % every == 0 or step + 1 == steps:
                loop.check_parameters()
                if rank == 0:
                    save_checkpoint(net, step + 1, os.path.join(wdir, '{}_iter{}.pt'.format(args.jid, step + 1)))
        if rank == 0:
            with open(os.path.join(wdir, '{}_loss.json'.format(args.jid)), 'w') as fh:
                json.dump(history, fh)
            split = loop.split()
            sys.stderr.write('Step split over {} ranks (s/step): {}; PCG iterations {}\n'.format(
                loop.world, ', '.join('{} {:.4f}'.format(k, v) for k, v in split.items()), [s['pcg_iterations'] for s in loop.steps]))
            sys.stderr.write('\nOverall runtime: {}\n'.format(time.perf_counter() - start))
        dist.barrier()
    finally:
        dist.destroy_process_group()
    return history


if __name__ == '__main__':
    main()
