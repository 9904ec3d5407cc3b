"""numpy restatement of the LangelaarFilter (overhang filter) for the tests, vectorised per layer.

The layer axis is the last grid axis; 2-D grids (nx, ny) are handled as (nx, 1, ny).  Written from the formulas:
  smin(a, b)   = (a + b - sqrt((a - b)^2 + eps) + sqrt(eps)) / 2
  forward      layer 0: out = in, smax = 1;  k >= 1: S = sum_support out^P, smax = S^(1/Q), out = smin(in, smax)
  backward     lambda(p) = g(p) + P out(p)^(P-1) / Q  sum_{q above p} lambda(q) dsmin_dx2(vars(q), smax(q)) S(q)^(1/Q-1),
               grad = lambda dsmin_dx1(vars, smax)
The support of an element on layer k is the element below it plus its in-bounds side neighbours on layer k-1.  A support
with S below the smallest normal double contributes 0 to the adjoint (the limit of 0 * inf)."""
import numpy as np

EPS, P, Q = 1e-4, 40.0, 40.0 - 1.58


def grid3(dims):
    d = tuple(int(v) for v in dims)
    return d if len(d) == 3 else (d[0], 1, d[1])


def cross(a):
    """a plane (nx, ny) summed over each element and its in-bounds +-1 neighbours in both axes (a symmetric stencil, so
    it is also its own transpose: the gather over the elements a plane element supports)."""
    s = a.copy()
    s[1:] += a[:-1]
    s[:-1] += a[1:]
    s[:, 1:] += a[:, :-1]
    s[:, :-1] += a[:, 1:]
    return s


def smin(a, b):
    return 0.5 * (a + b - np.sqrt((a - b) ** 2 + EPS) + np.sqrt(EPS))


def dsmin_dx1(a, b):
    return 0.5 * (1.0 - (a - b) / np.sqrt((a - b) ** 2 + EPS))


def dsmin_dx2(a, b):
    return 0.5 * (1.0 + (a - b) / np.sqrt((a - b) ** 2 + EPS))


def apply(x, dims):
    """returns (out, smax), both flat"""
    g = grid3(dims)
    x = np.asarray(x, dtype=np.float64).reshape(g)
    out, smax = np.empty(g), np.empty(g)
    out[..., 0], smax[..., 0] = x[..., 0], 1.0
    for k in range(1, g[2]):
        smax[..., k] = cross(out[..., k - 1] ** P) ** (1.0 / Q)
        out[..., k] = smin(x[..., k], smax[..., k])
    return out.reshape(-1), smax.reshape(-1)


def backprop(g_in, x, dims, out=None, smax=None):
    """gradient through the filter; out / smax are the caches of the apply being differentiated (default: apply(x))"""
    g3 = grid3(dims)
    if out is None:
        out, smax = apply(x, dims)
    gv = np.asarray(g_in, dtype=np.float64).reshape(g3)
    x, out, smax = (np.asarray(a, dtype=np.float64).reshape(g3) for a in (x, out, smax))
    lam = np.empty(g3)
    nz = g3[2]
    lam[..., nz - 1] = gv[..., nz - 1]
    for k in range(nz - 2, -1, -1):
        S = cross(out[..., k] ** P)                             # supports of layer k+1
        ok = S >= np.finfo(np.float64).tiny
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(ok, lam[..., k + 1] * dsmin_dx2(x[..., k + 1], smax[..., k + 1]) * S ** (1.0 / Q - 1.0), 0.0)
        lam[..., k] = gv[..., k] + P * out[..., k] ** (P - 1.0) / Q * cross(w)
    return (lam * dsmin_dx1(x, smax)).reshape(-1)
