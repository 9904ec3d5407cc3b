"""float64 numpy restatements of the design-update operations for the tests, written from the formulas and not from the
kernels' loop structure:
  smoothing   A x:   out_i = (1/c_i) sum_{k in N(i)} x_k,  N(i) the (2r+1)^d box around i clipped to the grid, c_i = |N(i)|
              A^T g: out_k = sum_{i in N(k)} g_i / c_i
  projection  P(x) = (tanh(b/2) + tanh(b (x - 1/2))) / (2 tanh(b/2)),  P'(x) = b (1 - tanh^2(b (x - 1/2))) / (2 tanh(b/2))
  OC step     clip(x0 sqrt(dJ / (dc lam)), max(x0 - m, 0), min(x0 + m, 1)) in the reference's order of max / min
The clipped box is a product of per-axis intervals, so A is the tensor product of 1-D row-normalised box filters: each is a
sum of 2r+1 shifted slices along one axis, scaled by the per-axis count.  No prefix sums: their cancellation at 10^7
elements would swamp the round-off these references are compared at."""
import numpy as np


def _axis_box(x, axis, r, transpose):
    n = x.shape[axis]
    out = np.zeros_like(x)
    idx = np.arange(n)
    cnt = (np.minimum(idx + r, n - 1) - np.maximum(idx - r, 0) + 1).astype(np.float64)
    shape = [1] * x.ndim
    shape[axis] = n
    cnt = cnt.reshape(shape)
    src = x / cnt if transpose else x
    for s in range(-min(r, n - 1), min(r, n - 1) + 1):
        # out[i] += src[i + s] for every i with 0 <= i + s < n
        dst = [slice(None)] * x.ndim
        sl = [slice(None)] * x.ndim
        dst[axis] = slice(max(0, -s), n - max(0, s))
        sl[axis] = slice(max(0, s), n - max(0, -s))
        out[tuple(dst)] += src[tuple(sl)]
    return out if transpose else out / cnt


def box_filter(x, grid, r, transpose=False):
    """A x (transpose=False) or A^T x on the row-major grid `grid` (2 or 3 extents); x is flat"""
    grid = tuple(int(v) for v in grid)
    y = np.asarray(x, dtype=np.float64).reshape(grid)
    for axis in range(len(grid)):
        y = _axis_box(y, axis, int(r), transpose)
    return y.reshape(-1)


def projection(x, beta):
    th = np.tanh(0.5 * beta)
    return 0.5 * (th + np.tanh(beta * (np.asarray(x, dtype=np.float64) - 0.5))) / th


def projection_backprop(g, x, beta):
    th = np.tanh(0.5 * beta)
    t = np.tanh(beta * (np.asarray(x, dtype=np.float64) - 0.5))
    return np.asarray(g, dtype=np.float64) * 0.5 * beta * (1.0 - t * t) / th


def oc_candidate(x0, dJ, dc, lam, m):
    """the reference's expression (OptimalityCriterion.hh:47-50); NaN where dJ / (dc lam) < 0, as np.maximum propagates it"""
    with np.errstate(invalid="ignore", divide="ignore"):
        v = x0 * np.sqrt(dJ / (dc * lam))
    return np.minimum(np.minimum(np.maximum(np.maximum(v, x0 - m), 0.0), x0 + m), 1.0)


def oc_candidate_nan_free(x0, dJ, dc, lam, m):
    """the device's chosen semantics: where the square root is not real, the lower edge max(x0 - m, 0) of the move window"""
    v = oc_candidate(x0, dJ, dc, lam, m)
    return np.where(np.isnan(v), np.minimum(np.maximum(x0 - m, 0.0), np.minimum(x0 + m, 1.0)), v)
