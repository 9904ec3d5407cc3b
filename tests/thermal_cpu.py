"""Dense numpy restatement of steady heat conduction on a degree-1 voxel grid, written from the formulas and not from
the kernels: the element matrix by quadrature, dense assembly and solves, a Jacobi-PCG with the device's stopping rule, the two
objectives with their gradients, and element-wise versions of the apply, diagonal, source, gradient and flux sums that also run in
np.longdouble (the reference of the kernel tests).

Nodes and elements are numbered with the last axis fastest; local node a of an element has axis 0 as its most significant bit.
"""
import functools
import itertools

import numpy as np

CHECK = 8                   # the device's PCG reads its residual once every CHECK iterations


def num_nodes(ne):
    return int(np.prod(np.asarray(ne) + 1))


def num_elements(ne):
    return int(np.prod(ne))


def node_bits(N):
    return np.array([[(a >> (N - 1 - d)) & 1 for d in range(N)] for a in range(2 ** N)])


def element_nodes(ne):
    """[elements, 2^N]: the global node of every local node"""
    ne = np.asarray(ne)
    N = ne.size
    ecoord = np.stack(np.meshgrid(*[np.arange(n) for n in ne], indexing="ij"), axis=-1).reshape(-1, N)
    out = np.empty((ecoord.shape[0], 2 ** N), dtype=np.int64)
    for a, bits in enumerate(node_bits(N)):
        out[:, a] = np.ravel_multi_index(tuple((ecoord + bits).T), tuple(ne + 1))
    return out


def node_coordinates(ne, h):
    ne = np.asarray(ne)
    grids = np.meshgrid(*[np.arange(n + 1) * hd for n, hd in zip(ne, h)], indexing="ij")
    return np.stack(grids, axis=-1).reshape(-1, ne.size)


def conductivity_tensor(k, N):
    k = np.asarray(k, dtype=np.float64)
    return k * np.eye(N) if k.ndim == 0 else k.reshape(N, N)


def conductivity_matrix(k, h):
    """Kc0[a][b] = int grad N_a . k grad N_b dV by two Gauss points per axis (exact for the multilinear element)"""
    h = np.asarray(h, dtype=np.float64)
    N = h.size
    k = conductivity_tensor(k, N)
    bits = node_bits(N)
    pts = [0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0)]
    K = np.zeros((2 ** N, 2 ** N))
    for xi in itertools.product(pts, repeat=N):
        G = np.empty((2 ** N, N))
        for a in range(2 ** N):
            for d in range(N):
                v = (1.0 if bits[a, d] else -1.0) / h[d]
                for o in range(N):
                    if o != d:
                        v *= xi[o] if bits[a, o] else 1.0 - xi[o]
                G[a, d] = v
        K += (G @ k @ G.T) * np.prod(h) / 2 ** N
    return K


def kappa(rho, p=3.0, k_min=1e-3):
    return k_min + rho ** p * (1.0 - k_min)


def dkappa(rho, p=3.0, k_min=1e-3):
    return p * rho ** (p - 1.0) * (1.0 - k_min)


def band_width(ne):
    """the half-bandwidth of A: the sum of the node strides"""
    strides = np.cumprod(np.concatenate([[1], (np.asarray(ne)[::-1] + 1)[:-1]]))
    return int(strides.sum())


def band_offset(i, j, w):
    """where A[i][j], j <= i <= j + w, lies in the tile layout of vfem_band_spd_factor (include/vfem.h)"""
    bt = (w + 63) // 64
    return ((i // 64) * (bt + 2) + i // 64 - j // 64) * 4096 + (i % 64) * 64 + j % 64


def band_doubles(n, w):
    return (n + 63) // 64 * ((w + 63) // 64 + 2) * 4096


# ---- dense ----

def assemble(ne, Kc0, kap, fixed=None, dtype=np.float64):
    """A = P (sum_e kappa_e Kc0) P + (I - P), dense"""
    en = element_nodes(ne)
    n = num_nodes(ne)
    A = np.zeros((n, n), dtype=dtype)
    np.add.at(A, (en[:, :, None], en[:, None, :]), kap.astype(dtype)[:, None, None] * Kc0.astype(dtype)[None])
    if fixed is not None and fixed.any():
        A[fixed, :] = 0.0
        A[:, fixed] = 0.0
        A[fixed, fixed] = 1.0
    return A


def load(ne, h, fixed=None, nodal=None, volumetric=None):
    return source(ne, h, volumetric, fixed, nodal)


def solve(A, Q):
    return np.linalg.solve(A, Q)


def compliance(ne, h, k, rho, fixed, nodal=None, volumetric=None, p=3.0, k_min=1e-3):
    """(J, T, dJ/drho, Q) of the thermal compliance J = Q . T"""
    Kc0 = conductivity_matrix(k, h)
    Q = load(ne, h, fixed, nodal, volumetric)
    T = solve(assemble(ne, Kc0, kappa(rho, p, k_min), fixed), Q)
    g = gradient(ne, Kc0, dkappa(rho, p, k_min), [-1.0], T[None], T[None])
    return float(Q @ T), T, g, Q


def pnorm_temperature(ne, h, k, rho, fixed, P, nodal=None, volumetric=None, p=3.0, k_min=1e-3):
    """(J_P, T, dJ_P/drho, lambda) of J_P = (sum |T|^P)^(1/P), evaluated scaled by max |T|"""
    Kc0 = conductivity_matrix(k, h)
    Q = load(ne, h, fixed, nodal, volumetric)
    A = assemble(ne, Kc0, kappa(rho, p, k_min), fixed)
    T = solve(A, Q)
    top = np.abs(T).max()
    J = top * np.sum((np.abs(T) / top) ** P) ** (1.0 / P)
    a = (np.abs(T) / J) ** (P - 1.0) * np.sign(T)
    a[fixed] = 0.0
    lam = solve(A, a)
    g = gradient(ne, Kc0, dkappa(rho, p, k_min), [-1.0], lam[None], T[None])
    return float(J), T, g, lam


def pcg(A, b, x0=None, tol=1e-8, max_iter=2000):
    """Jacobi-preconditioned CG with the device's rule: it stops when the recurrence residual, looked at before the first iteration and
    then every CHECK iterations, has |r| / |b| <= tol.  Returns x and a dict: ``iterations`` (where it stopped), ``crossing`` (the first
    iteration whose recurrence residual met the tolerance), ``relres`` (recurrence), ``true_relres`` and ``gap`` = their difference."""
    x = np.zeros_like(b) if x0 is None else x0.copy()
    dinv = 1.0 / np.diag(A)
    r = b - A @ x
    bb, rr = float(b @ b), float(r @ r)
    it, crossing = 0, 0 if rr <= tol * tol * bb else None
    done = rr <= tol * tol * bb
    d, rz_old = None, None
    while not done and it < max_iter:
        it += 1
        z = dinv * r
        rz = float(r @ z)
        d = z if it == 1 else z + (rz / rz_old) * d
        Ad = A @ d
        alpha = rz / float(d @ Ad)
        x = x + alpha * d
        r = r - alpha * Ad
        rr, rz_old = float(r @ r), rz
        if crossing is None and rr <= tol * tol * bb:
            crossing = it
        if it % CHECK == 0 or it == max_iter:
            done = rr <= tol * tol * bb
    true = float(np.linalg.norm(b - A @ x) / np.sqrt(bb))
    rel = float(np.sqrt(rr / bb))
    return x, dict(iterations=it, crossing=crossing, converged=done, relres=rel, true_relres=true, gap=abs(true - rel))


# ---- the kernels' sums, element by element, in float64 or np.longdouble ----

def _free(x, fixed):
    return x if fixed is None else np.where(fixed, 0, x)


def apply(ne, Kc0, kap, fixed, X, dtype=np.float64):
    """Y_c = A X_c for the block X [columns, nodes]"""
    en = element_nodes(ne)
    Kc0, kap, X = Kc0.astype(dtype), kap.astype(dtype), np.atleast_2d(X).astype(dtype)
    Y = np.zeros_like(X)
    for c in range(X.shape[0]):
        xe = _free(X[c], fixed)[en]                                                 # [elements, npe]
        np.add.at(Y[c], en, kap[:, None] * np.einsum("ab,eb->ea", Kc0, xe))
        if fixed is not None:
            Y[c] = np.where(fixed, X[c], Y[c])
    return Y


def diagonal(ne, Kc0, kap, fixed, dtype=np.float64):
    en = element_nodes(ne)
    d = np.zeros(num_nodes(ne), dtype=dtype)
    np.add.at(d, en, kap.astype(dtype)[:, None] * np.diag(Kc0).astype(dtype)[None, :])
    return d if fixed is None else np.where(fixed, dtype(1), d)


def source(ne, h, q, fixed, f_in, dtype=np.float64):
    """Q = P (f_in + sum_e q_e vol / 2^N)"""
    en = element_nodes(ne)
    out = np.zeros(num_nodes(ne), dtype=dtype) if f_in is None else np.asarray(f_in).astype(dtype).copy()
    if q is not None:
        share = dtype(np.prod(np.asarray(h, dtype=dtype))) / dtype(2 ** len(ne))
        qq = np.broadcast_to(np.asarray(q, dtype=dtype), (num_elements(ne),))
        np.add.at(out, en, (qq * share)[:, None] * np.ones(en.shape[1], dtype=dtype)[None, :])
    return _free(out, fixed)


def gradient(ne, Kc0, dkap, c, A, B, dtype=np.float64):
    """g[e] = dkappa_e sum_i c_i a_ie^T Kc0 b_ie"""
    en = element_nodes(ne)
    Kc0, dkap, c = Kc0.astype(dtype), np.asarray(dkap).astype(dtype), np.asarray(c).astype(dtype)
    A, B = np.atleast_2d(A).astype(dtype), np.atleast_2d(B).astype(dtype)
    s = np.zeros(en.shape[0], dtype=dtype)
    for i in range(c.size):
        s += c[i] * np.einsum("ea,ab,eb->e", A[i][en], Kc0, B[i][en])
    return dkap * s


def flux(ne, h, k, kap, T, dtype=np.float64):
    """q_e = -kappa_e k grad T at the element centre, [elements, N]"""
    N = len(ne)
    en = element_nodes(ne)
    bits = node_bits(N)
    h, k = np.asarray(h, dtype=dtype), conductivity_tensor(k, N).astype(dtype)
    Te = np.asarray(T).astype(dtype)[en]
    sign = np.where(bits == 1, 1, -1).astype(dtype)                               # [npe, N]
    grad = (Te @ sign) / (dtype(2 ** (N - 1)) * h)[None, :]
    return -np.asarray(kap).astype(dtype)[:, None] * (grad @ k.T)


# ---- fixtures shared with the GPU tests ----

EDGES = {2: (0.5, 0.3), 3: (0.5, 0.3, 0.7)}
K_ANISO = {2: np.array([[1.4, 0.3], [0.3, 0.8]]), 3: np.array([[1.4, 0.3, -0.2], [0.3, 0.8, 0.1], [-0.2, 0.1, 1.1]])}


def face_mask(ne, axis=0, which=0, middle_third=False):
    """the nodes of the face `axis` = 0 (or its far side); middle_third: only those within the middle third along the other axes"""
    ne = np.asarray(ne)
    idx = np.stack(np.meshgrid(*[np.arange(n + 1) for n in ne], indexing="ij"), axis=-1).reshape(-1, ne.size)
    m = idx[:, axis] == (0 if which == 0 else ne[axis])
    if middle_third:
        for d in range(ne.size):
            if d != axis:
                m &= (3 * idx[:, d] >= ne[d]) & (3 * idx[:, d] <= 2 * ne[d])
    return m


@functools.lru_cache(maxsize=None)
def pcg_fixture(ne):
    """the PCG problem of the issue on the grid `ne` (unit voxels, unit conductivity): rho uniform in [0.05, 1], p = 3, k_min = 1e-3, a
    unit volumetric source, the sink on the middle third of the face x = 0"""
    N = len(ne)
    rng = np.random.default_rng(1600 + num_elements(ne))
    rho = rng.uniform(0.05, 1.0, size=num_elements(ne))
    h = (1.0,) * N
    fixed = face_mask(ne, 0, 0, middle_third=True)
    Kc0 = conductivity_matrix(1.0, h)
    A = assemble(ne, Kc0, kappa(rho), fixed)
    Q = load(ne, h, fixed, volumetric=1.0)
    return dict(ne=ne, h=h, rho=rho, fixed=fixed, Kc0=Kc0, A=A, Q=Q)


# what pcg() takes on the two fixtures at tol 1e-8: the first iteration whose recurrence residual meets the tolerance
# (tests/test_thermal_cpu.py recomputes and pins them; the device may stop one check interval later, see tests/test_gpu_thermal.py)
PCG_SHAPES = [(40, 37), (12, 10, 9)]
PCG_CROSSING = {(40, 37): 234, (12, 10, 9): 71}
# the largest recurrence-to-true residual gap at convergence over the two fixtures (2.3e-13 and 3.2e-16), and what the PCG solution
# differs from the dense one by relative to max |T| (4.3e-11 and 2.9e-10): measured by the same test, which pins them within a factor
# of three
PCG_GAP_MEASURED = 2.8e-13
PCG_SOLUTION_MEASURED = {(40, 37): 5.2e-11, (12, 10, 9): 3.5e-10}


def pcg_iteration_bound(ne):
    """the restatement's count rounded up to the check interval, plus one more interval: the device sums in another order, so the
    crossing may move by an iteration"""
    return (PCG_CROSSING[tuple(ne)] + CHECK - 1) // CHECK * CHECK + CHECK


@functools.lru_cache(maxsize=None)
def direct_fixture(ne):
    """a direct-solver problem: random densities, anisotropic conductivity, the sink on the face x = 0, a volumetric and a nodal source"""
    N = len(ne)
    rng = np.random.default_rng(1700 + num_elements(ne))
    fixed = face_mask(ne, 0, 0)
    return dict(ne=ne, h=EDGES[N], k=K_ANISO[N], rho=rng.uniform(0.05, 1.0, size=num_elements(ne)), fixed=fixed,
                nodal=rng.uniform(0.0, 1.0, size=num_nodes(ne)), volumetric=rng.uniform(0.5, 1.5, size=num_elements(ne)))


def slab_case(ne, q=1.3, k=0.7, rho=0.8):
    """a slab with a uniform source and the sink on the face x = 0: T = q / (kappa k) (L x - x^2 / 2) at the nodes.  Returns
    (T, exact, J)"""
    N = len(ne)
    h = EDGES[N]
    fixed = face_mask(ne, 0, 0)
    r = np.full(num_elements(ne), rho)
    J, T, _, _ = compliance(ne, h, k, r, fixed, volumetric=q)
    x = node_coordinates(ne, h)[:, 0]
    L = ne[0] * h[0]
    return T, q / (kappa(rho) * k) * (L * x - 0.5 * x * x), J


def layers_case(ne, flux_in=0.9, k=0.7):
    """layers in series along axis 0 under a uniform flux on the face x = L, the sink on x = 0: the far face stands at
    flux sum_i h / (kappa_i k).  Returns (T on the far face, exact)"""
    N = len(ne)
    h = EDGES[N]
    rng = np.random.default_rng(1800 + num_elements(ne))
    layer = rng.uniform(0.2, 1.0, size=ne[0])
    rho = np.repeat(layer, num_elements(ne) // ne[0])
    far = face_mask(ne, 0, 1)
    # the face load of a uniform flux: each face element gives a 2^(N-1)-th of flux x its area to its nodes
    area = np.prod(h[1:])
    idx = np.stack(np.meshgrid(*[np.arange(n + 1) for n in ne], indexing="ij"), axis=-1).reshape(-1, N)
    share = np.ones(num_nodes(ne))
    for d in range(1, N):
        share *= np.where((idx[:, d] == 0) | (idx[:, d] == ne[d]), 0.5, 1.0)
    nodal = np.where(far, flux_in * area * share, 0.0)
    _, T, _, _ = compliance(ne, h, k, rho, face_mask(ne, 0, 0), nodal=nodal)
    return T[far], flux_in * np.sum(h[0] / (kappa(layer) * k))


# the restatement's own errors on the analytic cases (tests/test_thermal_cpu.py measures and pins them within a factor of three); the
# device bounds are ten times these, or nodes x 2^-52 where the figure is no more than one rounding (tests/loadcases_cpu.free_c_bound)
SLAB_SHAPES = [(16, 6), (6, 4, 3)]
SLAB_MEASURED = {(16, 6): 1.7e-13, (6, 4, 3): 1.4e-14}
LAYERS_MEASURED = {(16, 6): 6.0e-13, (6, 4, 3): 1.6e-15}


def analytic_bound(measured, ne):
    return 10.0 * measured if measured > 2.0 ** -52 else num_nodes(ne) * 2.0 ** -52
