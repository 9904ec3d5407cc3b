"""The messages and collectives of the x-slab ranks, and the only place that knows the backend.

"nccl" (RCCL over xGMI, one device per rank) moves device buffers; "gloo" (CPU tests, ranks that share a device) moves host
buffers.  `SlabComm` sends a tensor as it is where the backend reaches it and through a copy on the other side where it does not
(a device tensor under gloo, a host scalar under nccl), so callers never ask which backend runs.  With one rank nothing is sent.
As a rank proxy (`proxy=(world, rank)`, tools/rank_proxy.py: ONE rank of `world` alone in its process) no peer exists: a
neighbour message becomes a device copy of the same bytes, reductions stay local, a gather repeats the rank's own block.
"""
import torch
import torch.distributed as dist

SUM, MAX = dist.ReduceOp.SUM, dist.ReduceOp.MAX


class SlabComm:
    def __init__(self, group=None, proxy=None):
        self.group = group
        self.proxy = proxy is not None
        if self.proxy:
            self.world, self.rank = int(proxy[0]), int(proxy[1])
        elif dist.is_available() and dist.is_initialized():
            self.world, self.rank = dist.get_world_size(group), dist.get_rank(group)
        else:
            self.world, self.rank = 1, 0
        self.alone = self.world == 1 or self.proxy                       # nothing leaves this process
        self.host = not self.alone and dist.get_backend(group) == "gloo"   # messages travel through host memory

    def _wire(self, t):
        """`t` itself where the backend reaches it, else a copy on the side it does"""
        t = t.contiguous()
        return t.cpu() if self.host else t.cuda()

    def _in_place(self, collective, t):
        h = self._wire(t)
        collective(h)
        if h is not t:
            t.copy_(h)
        return t

    def all_reduce(self, t, op=SUM):
        """in place on `t`"""
        return t if self.alone else self._in_place(lambda h: dist.all_reduce(h, op=op, group=self.group), t)

    def broadcast(self, t, src=0):
        """in place on `t`"""
        return t if self.alone else self._in_place(lambda h: dist.broadcast(h, src, group=self.group), t)

    def _gather(self, mine, counts, dst):
        """flat slabs of `counts[r]` values per rank (they differ by at most one aligned block) through equal-size buffers --
        RCCL's gathers want one size"""
        if self.world == 1:
            return mine
        if self.proxy:
            return torch.cat([(mine if c <= mine.numel() else mine.repeat(2))[:c] for c in counts])
        send = torch.zeros(max(counts), dtype=mine.dtype, device="cpu" if self.host else mine.device)
        send[:mine.numel()].copy_(mine)
        bufs = [torch.empty_like(send) for _ in counts] if dst in (None, self.rank) else None
        if dst is None:
            dist.all_gather(bufs, send, group=self.group)
        else:
            dist.gather(send, bufs, dst=dst, group=self.group)
        return None if bufs is None else torch.cat([b[:c] for b, c in zip(bufs, counts)]).to(mine.device)

    def all_gather_slabs(self, mine, counts):
        """the ranks' slabs concatenated in rank order, on every rank"""
        return self._gather(mine, counts, None)

    def gather_slabs(self, mine, counts, dst=0):
        """the ranks' slabs concatenated in rank order on rank `dst`, None on the others"""
        return self._gather(mine, counts, dst)

    def start(self, pairs):
        """Begin the exchange with the x-neighbours: `pairs` holds up to two (peer, send_tensor, recv_view), ONE message each way
        per entry, all posted as one batch of non-blocking sends / receives.  Returns the handle for `finish`; the transfers run
        while the caller launches work that touches neither tensor.  A contiguous `recv_view` the backend reaches is received
        into directly; any other is filled in `finish`."""
        if self.proxy:
            for _, send, recv in pairs:
                recv.copy_(send)
            return None
        ops, copies = [], []
        for peer, send, recv in pairs:
            sb = self._wire(send)
            rb = recv if recv.is_contiguous() and recv.is_cuda != self.host else torch.empty_like(sb)
            ops.append(dist.P2POp(dist.isend, sb, peer, self.group))
            ops.append(dist.P2POp(dist.irecv, rb, peer, self.group))
            if rb is not recv:
                copies.append((recv, rb))
        return (dist.batch_isend_irecv(ops), copies) if ops else None

    def finish(self, handle):
        """wait for the transfers of `start`; afterwards every recv_view holds the neighbour's data"""
        if handle is None:
            return
        works, copies = handle
        for w in works:
            w.wait()
        for recv, rb in copies:
            recv.copy_(rb)
