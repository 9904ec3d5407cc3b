"""The neural design loop of training/train_xdg.py over the x-slab ranks of `distributed.DistributedMGSolver` ("The neural
design loop over the ranks").

Every rank evaluates the Fourier-feature MLP on the voxels of its owned element layers only (`TrainableMLP.set_grid(...,
voxel_range=...)`) and holds the same parameters.  One step:

  forward    vfem_mlp_forward_grid_range on the owned voxels
  satisfier  hard modes: the bisection of sigmoid_with_constrained_mean with one scalar all-reduce per probe (at most 128);
             soft modes: clamp, then the volume penalty on the mean of the whole field (one all-reduce of the local sum)
  solve      densities to the slab solver (set_local_densities: one message per neighbour, or an all-gather of the field when the
             hierarchy is too shallow to shard), warm-started PCG, compliance_gradient of the owned elements
  backward   vfem_mlp_backward_grid_range, then ONE all-reduce of the parameter gradients (TrainableMLP._all_reduce)
  adam       vfem_adam_step on every rank: the same update of the same summed gradient keeps the parameters equal

The loss is the whole field's on every rank.  Degree 1, 3-D, multigrid only."""
import time

import torch

from . import fem
from .distributed import SlabLoop
from .slab_comm import MAX, SUM


class _SlabCompliance(torch.autograd.Function):
    """fem.VoxelFEMFunction with the owned densities of a rank: value 2 J of the whole field, gradient the owned sensitivities"""

    @staticmethod
    def forward(ctx, density_owned, loop):
        loop._set_densities(density_owned.detach().to(torch.float64))
        loop._solve(loop.SOLVER["tol"])
        # as in the reference's autograd node the value is 2 J but the gradient is that of J (fem.py:122-126)
        ctx.save_for_backward(loop.ds.compliance_gradient(loop._u).to(torch.float32))
        return density_owned.new_tensor(2.0 * loop.ds.compliance(loop._f, loop._u))

    @staticmethod
    def backward(ctx, grad_output):
        (g,) = ctx.saved_tensors
        return g * grad_output, None


class DistributedXdgLoop(SlabLoop):
    """train_xdg's loop on the slab ranks (one instance per rank; all ranks call every method in the same order).

    Solver as the one-GPU driver sets it up (E0 = 1, Emin = 1e-4, SIMP exponent 3, fem.DesignLoop.SOLVER, 100 PCG iterations at
    most), and started as MultigridComplianceObjective starts: one solve from zero at the uniform volume fraction with tol 1e-5;
    every later solve warm-starts from the previous displacements.  `attach(net)` takes the network (a TrainableMLP built as the
    one-GPU driver builds it), broadcasts its parameters and B from rank 0 and restricts it to the owned voxels.

    `sharded` says how the densities reach the solver, decided once here: set_local_densities when the hierarchy allows it
    (T >= MIN_SHARDED_T), otherwise the gather of the whole field + set_global_densities.  `steps` keeps, per step, the loss, the
    PCG iterations and the wall time of the five parts (TIMERS)."""

    TIMERS = ("forward", "satisfier", "solve", "backward", "adam")

    def __init__(self, material, bcs, order, corners, grid, volume_fraction, mg_levels, vcs="constrained_sigmoid", dist_levels=None,
                 log=None):
        self.hard = fem.type_of_volume_constaint_satisfier(vcs)      # (an unknown satisfier is refused before the solver is built)
        self.vcs = vcs
        super().__init__(material, bcs, order, corners, grid, 3.0, mg_levels, dist_levels=dist_levels)   # train_xdg forces the SIMP exponent to 3
        self.v = float(volume_fraction)
        ds = self.ds
        self.first, self.count = ds.owned_element_range()
        self.sharded = ds.T >= ds.MIN_SHARDED_T
        if log is not None and self.rank == 0:
            log.write("Densities to the solver: {} ({} ranks, {} distributed levels)\n".format(
                "sharded (set_local_densities)" if self.sharded else "gathered (all-gather + set_global_densities)",
                self.world, ds.Ld + 1))
        self.net = None
        self.steps = []
        self._max_volume = torch.tensor(self.v, device=self.dev)
        self._first_solve(torch.full((self.count,), self.v, dtype=torch.float64, device=self.dev))

    # ---- collectives --------------------------------------------------------------------------------
    def _allsum(self, t):
        return self.comm.all_reduce(t.detach().clone(), SUM)

    def _allmax(self, t):
        return self.comm.all_reduce(t.detach().clone(), MAX)

    def broadcast_parameters(self, src=0):
        """parameters and B of rank `src` to every rank (at the start and after a checkpoint is loaded)"""
        for t in [self.net.B] + list(self.net.parameters()):
            self.comm.broadcast(t.data, src)

    def check_parameters(self):
        """raise unless every rank holds the same parameters: one all-reduce (MAX) of [sum, sum of squares] and their negatives"""
        with torch.no_grad():
            s = sum(float(p.double().sum()) for p in self.net.parameters())
            q = sum(float(p.double().square().sum()) for p in self.net.parameters())
        agreed = self.comm.all_reduce(torch.tensor([s, q, -s, -q], dtype=torch.float64, device=self.dev), MAX)
        most, least = agreed[:2].tolist(), (-agreed[2:]).tolist()
        if most != least:
            raise RuntimeError("DistributedXdgLoop: the ranks' parameters differ (checksums: max %r, min %r)" % (most, least))

    # ---- network ------------------------------------------------------------------------------------
    def attach(self, net):
        self.net = net
        net.set_grid(self.ne, voxel_range=(self.first, self.count))
        self.broadcast_parameters()
        return self

    # ---- solve --------------------------------------------------------------------------------------
    def _set_densities(self, owned):
        if self.sharded:
            self.ds.set_local_densities(owned)
        else:
            self.ds.set_global_densities(self.comm.all_gather_slabs(owned, [n * self.layer for n in self.ds.part.layers()]))

    # ---- one step -----------------------------------------------------------------------------------
    def loss(self, lap=lambda name: None):
        """the closure of train_xdg without the optimiser step: the loss tensor (the whole field's, the same on every rank; call
        .backward() on it).  `lap(name)` is called as each part (TIMERS) ends."""
        logits = self.net.forward_grid()
        lap("forward")
        if self.hard:
            density = fem.satisfy_volume_constraint(logits, self._max_volume, mode=self.vcs, allsum=self._allsum, allmax=self._allmax)
        else:
            density = torch.clamp(logits, 0.0, 1.0)
        self.last_density = density.detach()
        lap("satisfier")
        loss = _SlabCompliance.apply(density, self)
        lap("solve")
        if not self.hard:
            loss = loss + fem.satisfy_volume_constraint(density, self._max_volume, compliance_loss=loss.detach(), scaler_mode='clip',
                                                        constant=1500, mode=self.vcs, allsum=self._allsum)
            lap("satisfier")
        return loss

    def step(self, lr):
        """one step of train_xdg's loop; returns the loss"""
        t = dict.fromkeys(self.TIMERS, 0.0)
        torch.cuda.synchronize()
        clock = [time.perf_counter()]

        def lap(name):
            torch.cuda.synchronize()
            now = time.perf_counter()
            t[name] += now - clock[0]
            clock[0] = now

        self.net.zero_grad()
        loss = self.loss(lap)
        loss.backward()
        lap("backward")
        self.net.adam_step(lr=float(lr))
        lap("adam")
        value = float(loss.detach())
        self.steps.append(dict(t, loss=value, pcg_iterations=self.ds.last_iterations))
        return value

    def split(self):
        """mean seconds per step of each part over the steps run so far"""
        n = max(1, len(self.steps))
        return {k: sum(s[k] for s in self.steps) / n for k in self.TIMERS}
