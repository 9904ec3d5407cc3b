"""networks.MLP restated in a few lines of CPU torch for the tests, in float64 (or, with dtype=torch.float32, in the precision
the modelled project runs it at: the yardstick for what rounding alone costs).  Written from the formulas:
  forward    f = [sin(2 pi x B^T), cos(2 pi x B^T)];  h_0 = relu(W_0 f + b_0);  h_i = relu(W_i h_{i-1} + b_i);
             out = W_last h + b_last, optionally through a sigmoid
  backward   torch.autograd of L = sum_v g_out[v] out[v]
The float32 inputs (coordinates, B, weights, g_out) are promoted to `dtype` once and never rounded back.  Voxels are
evaluated in batches (the parameter gradients accumulate over them), so 2^20 voxels of a 2048-feature network fit in memory.

Next to the outputs it returns, per voxel, the smallest |pre-activation| over all hidden units: a unit within rounding of zero
flips its ReLU between two precisions, after which the two gradients differ by that unit's whole contribution -- no summation
error, and nothing a tolerance should be sized for.  `mask_below` zeroes g_out on such voxels (they are still evaluated, and
contribute nothing in any implementation), which keeps a float64 gradient a meaningful reference for a float32 one."""
import os

import numpy as np
import torch

DELTA = 2e-5          # about ten times the fp32 rounding of an O(1) pre-activation summed over up to 2048 terms


def cpu_threads():
    """threads for the CPU reference: what the environment grants (OMP_NUM_THREADS, else the affinity mask), at most 16"""
    n = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return max(1, min(16, n if n > 0 else len(os.sched_getaffinity(0))))


def _batch(width):
    return max(1024, (1 << 24) // int(width))          # <= 128 MB per float64 activation matrix


def run(coords, B, Ws, bs, sigmoid=False, g_out=None, dtype=torch.float64, mask_below=None):
    """coords [..., 3], B [es, 3], Ws / bs: the Linear layers in order (torch layout [out, in]), all float32 arrays.
    Returns a dict: out [nvox], min_pre [nvox] (smallest hidden |pre-activation|), and -- when g_out [nvox] is given --
    g_out as used, gW, gb (lists in layer order).  mask_below: g_out is zeroed where min_pre < mask_below before it is used."""
    threads = torch.get_num_threads()
    torch.set_num_threads(cpu_threads())
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dtype)
        x = t(coords).reshape(-1, 3)
        nvox, nl = x.shape[0], len(Ws)
        Bt = t(B)
        W = [t(w).reshape(np.asarray(w).shape[0] if np.asarray(w).ndim == 2 else 1, -1) for w in Ws]
        b = [t(v).reshape(-1) for v in bs]
        want_grad = g_out is not None
        if want_grad:
            g = t(g_out).reshape(-1).clone()
            assert g.numel() == nvox
            for p in W + b:
                p.requires_grad_(True)
        out, min_pre = torch.empty(nvox, dtype=dtype), torch.empty(nvox, dtype=dtype)
        two_pi = torch.tensor(2.0 * np.pi, dtype=dtype)
        step = _batch(max(2 * Bt.shape[0], W[0].shape[0]))
        for v0 in range(0, nvox, step):
            v1 = min(nvox, v0 + step)
            with torch.set_grad_enabled(want_grad):
                proj = (two_pi * x[v0:v1]) @ Bt.T
                h = torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1)
                lo = torch.full((v1 - v0,), float("inf"), dtype=dtype)
                for i in range(nl):
                    h = h @ W[i].T + b[i]
                    if i < nl - 1:
                        lo = torch.minimum(lo, h.detach().abs().min(dim=1).values)
                        h = torch.relu(h)
                o = h.reshape(-1)
                if sigmoid:
                    o = torch.sigmoid(o)
                out[v0:v1], min_pre[v0:v1] = o.detach(), lo
                if want_grad:
                    if mask_below is not None:
                        g[v0:v1] = torch.where(lo < mask_below, torch.zeros_like(lo), g[v0:v1])
                    (g[v0:v1] * o).sum().backward()
        res = {"out": out.numpy(), "min_pre": min_pre.numpy()}
        if want_grad:
            res["g_out"] = g.numpy()
            res["gW"] = [p.grad.numpy() for p in W]
            res["gb"] = [p.grad.numpy() for p in b]
        return res
    finally:
        torch.set_num_threads(threads)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
