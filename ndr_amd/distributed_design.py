"""The ground-truth OC design loop (fem.DesignLoop) over the x-slab ranks of `distributed.DistributedMGSolver` ("The OC design
loop over the ranks").

Every rank holds the design variables of its owned element layers; no rank ever holds the whole field.  The compliance solve is
the slab solver with sharded densities (`set_local_densities`), warm-started as in DesignLoop.  The design update -- smoothing
filter (box, radius r), projection filter (tanh, beta), volume constraint and the optimality-criterion bisection -- runs on the
owned layers plus r ghost layers towards each neighbour:

  gradient   compliance_gradient (owned) -> projection backprop (owned) -> ONE exchange of r ghost layers (objective and
             constraint chains batched) -> slab box transpose (owned); the counts c_i come from the global extents, so r ghost
             layers of the input suffice
  inputs     ONE batched exchange of the ghost layers of x0, dJ, dc
  probe      candidate on owned + ghost layers (the ghost candidates equal the neighbours' owned ones bit for bit: same inputs, same
             elementwise kernel) -> slab box apply (owned) -> projection -> sum over the owned layers -> ONE scalar all-reduce.
             No probe exchanges element layers, and every branch is taken on all-reduced values, so all ranks walk the same bisection
  accept     the accepted candidate (ghosts included) through the filters, locally, then set_local_densities (its own exchange)

so a step sends three element-layer messages per neighbour whatever the number of probes.  Degree 1, 3-D, multigrid only."""
import ctypes
import time

import numpy as np
import torch

from . import _lib
from .distributed import SlabLoop
from .pyVoxelFEM import _ptr, _stream


class DistributedDesignLoop(SlabLoop):
    """fem.DesignLoop on the slab ranks (one instance per rank, all ranks call every method in the same order).

    The constructor takes DesignLoop's arguments plus `dist_levels` (distributed multigrid levels, default: the solver's automatic
    choice) and `group` (torch.distributed group).  `radius` (smoothing filter) and `beta` (projection filter) default to 1 and 1
    as in DesignLoop's filter chain and may be changed before `seed`."""

    def __init__(self, material, bcs, order, corners, grid, simp_exponent, volume_fraction, mg_levels, use_multigrid=True,
                 dist_levels=None, group=None):
        super().__init__(material, bcs, order, corners, grid, simp_exponent, mg_levels, use_multigrid, dist_levels, group)
        self.order = list(order)
        self.v = float(volume_fraction)
        self.radius, self.beta = 1, 1.0
        self.N = self.ne[0] * self.layer
        self.x0, self.x1 = self.ds.part.x0, self.ds.part.x1
        self.own = self.x1 - self.x0
        self.lib = _lib.load()
        self.history = []
        self.adaptive_filtering = None
        self.messages = 0               # element-layer messages this rank sent (one per neighbour and exchange)
        self.lambdas, self.probes, self.pcg_iterations = [], [], []
        self.timers = {"solve": 0.0, "update": 0.0, "comm": 0.0}
        self._lmin, self._lmax = 1.0, 2.0
        self._check_radius()
        self._phys = torch.full((self.own * self.layer,), self.v, dtype=torch.float64, device=self.dev)
        self._vars = None
        self._first_solve(self._phys)

    # ---- geometry -----------------------------------------------------------------------------------
    def _check_radius(self):
        r = int(self.radius)
        if r < 0:
            raise RuntimeError("DistributedDesignLoop: negative filter radius %d" % r)
        thinnest = min(self.ds.part.layers())
        if self.world > 1 and r > thinnest:
            raise RuntimeError("DistributedDesignLoop: filter radius %d exceeds the %d owned element layers of the thinnest slab; "
                               "use fewer ranks or a smaller radius" % (r, thinnest))
        return r

    def _ghosts(self):
        r = int(self.radius)
        return (r if self.rank > 0 else 0), (r if self.rank < self.world - 1 else 0)

    # ---- element-layer exchange ------------------------------------------------------------------------
    def _exchange(self, fields):
        """fill the ghost layers of the extended arrays `fields` (each [(gl + own + gr) * layer]) from the neighbours' owned layers:
        one message per neighbour and direction for all fields together"""
        gl, gr = self._ghosts()
        if self.world == 1 or (gl == 0 and gr == 0):
            return
        clock = time.perf_counter()
        views = [f.view(-1, self.layer) for f in fields]
        pairs, slots = [], []
        for peer, send_first, count, recv_first in ((self.rank - 1, gl, gl, 0), (self.rank + 1, gl + self.own - gr, gr, gl + self.own)):
            if count:
                sb = torch.cat([v[send_first:send_first + count] for v in views])
                pairs.append((peer, sb, torch.empty_like(sb)))
                slots.append((recv_first, count))
        self.comm.finish(self.comm.start(pairs))
        for (_, _, rb), (first, count) in zip(pairs, slots):
            for v, part in zip(views, rb.view(len(views), count, self.layer)):
                v[first:first + count].copy_(part)
        self.messages += len(pairs)
        self.timers["comm"] += time.perf_counter() - clock

    def _extend(self, owned):
        gl, gr = self._ghosts()
        ext = torch.empty(((gl + self.own + gr) * self.layer,), dtype=torch.float64, device=self.dev)
        ext[gl * self.layer:(gl + self.own) * self.layer].copy_(owned)
        return ext

    def _allreduce(self, value):
        if self.world == 1:
            return value
        clock = time.perf_counter()
        t = self.comm.all_reduce(torch.tensor([value], dtype=torch.float64))
        self.timers["comm"] += time.perf_counter() - clock
        return float(t[0])

    # ---- device kernels ----------------------------------------------------------------------------
    def _box(self, ext, transpose):
        """slab box filter of the extended array `ext` (owned + ghost layers), owned layers out"""
        gl, gr = self._ghosts()
        out = torch.empty((self.own * self.layer,), dtype=torch.float64, device=self.dev)
        n = (ctypes.c_int64 * 3)(gl + self.own + gr, self.ne[1], self.ne[2])
        _lib.check(self.lib.vfem_box_filter_slab(n, self.x0 - gl, self.ne[0], gl, self.own, int(self.radius), _ptr(ext),
                                                 _ptr(out), int(transpose), _stream()))
        return out

    def _projection(self, x):
        out = torch.empty_like(x)
        _lib.check(self.lib.vfem_projection(x.numel(), float(self.beta), _ptr(x), _ptr(out), _stream()))
        return out

    def _projection_backprop(self, g, x):
        out = torch.empty_like(g)
        _lib.check(self.lib.vfem_projection_backprop(g.numel(), float(self.beta), _ptr(g), _ptr(x), _ptr(out), _stream()))
        return out

    def _sum(self, x):
        """global sum of the owned values `x`: local device reduction, one scalar all-reduce"""
        m = ctypes.c_double(0.0)
        _lib.check(self.lib.vfem_mean(x.numel(), _ptr(x), ctypes.byref(m), _stream()))
        return self._allreduce(m.value * x.numel())

    def _volume_constraint(self, phys):
        """TotalVolumeConstraint 1 - mean/v of the whole field, from the owned physical densities"""
        return 1.0 - (self._sum(phys) / self.N) / self.v

    # ---- problem -----------------------------------------------------------------------------------
    def _set_densities(self, phys):
        clock = time.perf_counter()
        super()._set_densities(phys)
        self.messages += (self.rank > 0) + (self.rank < self.world - 1)
        self.timers["comm"] += time.perf_counter() - clock

    def _solve(self, tol):
        torch.cuda.synchronize()
        clock = time.perf_counter()
        super()._solve(tol)
        self.pcg_iterations.append(self.ds.last_iterations)
        torch.cuda.synchronize()
        self.timers["solve"] += time.perf_counter() - clock

    def _set_vars_ext(self, ext):
        """TopologyOptimizationProblem.setVars with the extended design (owned + valid ghost layers): filters, densities, solve"""
        gl, _ = self._ghosts()
        x = ext[gl * self.layer:(gl + self.own) * self.layer]
        if self._vars is not None:
            d = x - self._vars
            if self._allreduce(float((d * d).sum())) ** 0.5 < 1e-16:
                return False                                          # Problem.hh:50-51, on the global norm
        self._vars = x.clone()
        self._filtered = self._box(ext, 0)
        self._phys = self._projection(self._filtered)
        self._set_densities(self._phys)
        self._solve(self.SOLVER["tol"])
        return True

    def set_vars(self, x_owned):
        """design variables of the owned layers (flat, float64); ghost layers come from the neighbours"""
        ext = self._extend(x_owned.to(device=self.dev, dtype=torch.float64).reshape(-1))
        self._exchange([ext])
        return self._set_vars_ext(ext)

    def seed(self, design=None):
        """start from `design` (the whole grid's or the owned layers' design variables; array or tensor) or from the current
        physical densities"""
        self._check_radius()
        if design is None:
            x = self._phys
        else:
            x = torch.as_tensor(np.asarray(design.detach().cpu() if isinstance(design, torch.Tensor) else design, dtype=np.float64))
            x = x.reshape(-1)
            if x.numel() == self.N:
                x = x[self.x0 * self.layer:self.x1 * self.layer]
            elif x.numel() != self.own * self.layer:
                raise RuntimeError("seed: %d values match neither the grid (%d) nor the owned layers (%d)"
                                   % (x.numel(), self.N, self.own * self.layer))
        self.set_vars(x.to(self.dev))

    def objective(self):
        """J = 1/2 f.u (global)"""
        return self.ds.compliance(self._f, self._u)

    def compliance(self):
        return 2.0 * self.objective()

    def owned_densities(self):
        """physical densities of the owned layers (flat device tensor)"""
        return self._phys

    def gather_densities(self, dst=0):
        """physical densities of the whole grid as a numpy array [nx * ny * nz] on rank `dst` (None on the others)"""
        whole = self.comm.gather_slabs(self._phys, [n * self.layer for n in self.ds.part.layers()], dst)
        return None if whole is None else whole.cpu().numpy()

    # ---- optimality criterion ----------------------------------------------------------------------
    def _gradients(self):
        """dJ and dc of the owned design variables (TopologyOptimizationProblem.evaluateObjectiveGradient_device /
        evaluateConstraintsJacobian_device through the two filters)"""
        gl, _ = self._ghosts()
        g = self.ds.compliance_gradient(self._u)
        gp = self._extend(self._projection_backprop(g, self._filtered))
        c = torch.full((self.own * self.layer,), -1.0 / (self.v * self.N), dtype=torch.float64, device=self.dev)
        cp = self._extend(self._projection_backprop(c, self._filtered))
        self._exchange([gp, cp])
        return self._box(gp, 1), self._box(cp, 1)

    def step(self, m=0.2, ctol=1e-6):
        """OCOptimizer.step with the bracket kept across steps"""
        if self._vars is None:
            raise RuntimeError("Must call seed first!")
        torch.cuda.synchronize()
        clock = time.perf_counter()
        comm0, solve0 = self.timers["comm"], self.timers["solve"]
        dJ, dc = self._gradients()
        x0, dJe, dce = self._extend(self._vars), self._extend(dJ), self._extend(dc)
        self._exchange([x0, dJe, dce])
        cand = torch.empty_like(x0)
        probes = [0]

        def stepped(lam):
            _lib.check(self.lib.vfem_oc_candidate(x0.numel(), _ptr(x0), _ptr(dJe), _ptr(dce), float(lam), float(m),
                                                  _ptr(cand), _stream()))
            return cand

        def ceval(lam):
            probes[0] += 1
            return self._volume_constraint(self._projection(self._box(stepped(lam), 0)))

        while ceval(self._lmin) > 0:
            self._lmax = self._lmin
            self._lmin /= 2
        while ceval(self._lmax) < 0:
            self._lmin = self._lmax
            self._lmax *= 2
        mid = 0.5 * (self._lmin + self._lmax)
        vol = ceval(mid)
        while abs(vol) > ctol:
            if vol < 0:
                self._lmin = mid
            if vol > 0:
                self._lmax = mid
            mid = 0.5 * (self._lmin + self._lmax)
            vol = ceval(mid)
        self._set_vars_ext(stepped(mid).clone())
        self.lambdas.append(mid)
        self.probes.append(probes[0])
        obj, con = self.objective(), self._volume_constraint(self._phys)
        if self.rank == 0:
            print("objective, constraint, lambda estimate: %g\t%g\t%g" % (obj, con, mid))
        torch.cuda.synchronize()
        self.timers["update"] += (time.perf_counter() - clock) - (self.timers["comm"] - comm0) - (self.timers["solve"] - solve0)

    def run(self, steps, log=None):
        """DesignLoop.run: `steps` OC steps, compliance recorded before each; rank 0 writes the progress lines to `log`"""
        clock = time.perf_counter()
        for k in range(steps):
            c = self.compliance()
            self.history.append(c)
            if log is not None and self.rank == 0:
                log.write('Total Steps: {:d}, Runtime: {:.1f}, Compliance loss {:.6f}\n'.format(k, time.perf_counter() - clock, c))
            clock = time.perf_counter()
            self.step()
        return self.history

    def thresholded_compliance(self):
        """compliance of the design rounded to {0, 1} at 0.5; the design is restored as DesignLoop does (vars = physical densities)"""
        x = self._phys.clone()
        self.set_vars((x > 0.5).to(torch.float64))
        c = self.compliance()
        self.set_vars(x)
        return c
