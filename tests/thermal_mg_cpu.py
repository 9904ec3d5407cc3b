"""numpy restatement of the multigrid-preconditioned CG of the scalar conduction operator, written from the method's
specification and not from the kernels, on top of tests/thermal_cpu.py.

    levels      level l + 1 exists while every extent of level l is even and at least 4 elements; half the elements per axis
    fixed       a coarse node is fixed exactly when the fine node it coincides with is
    P_l         F_l I_l F_{l+1}: I_l the N-linear interpolation (weights 1, 1/2, 1/4, 1/8), F_l the 0/1 diagonal of the free nodes
    operators   A'_0 = F_0 (sum_e kappa_e Kc0) F_0,  A'_{l+1} = P_l^T A'_l P_l,  A_l = A'_l + (I - F_l)
    sweep       the 2^N colours (parity of the node index per axis, axis 0 the most significant bit), ascending or descending;
                on every node of the colour x += (b - A_l x) / diag A_l
    V-cycle     from zero: `smoothing` ascending sweeps, the residual, b_{l+1} = P_l^T r_l, the cycle of level l + 1,
                x_l += P_l x_{l+1}, `smoothing` descending sweeps; the coarsest level is solved exactly
    PCG         z = V-cycle(r); stops when the recurrence residual has |r| / |b| <= tol, looked at every iteration

Operators are sparse in coordinate form (``Op``) so that everything also runs in np.longdouble (the floors of the device tests);
in float64 the Galerkin products go through scipy.sparse, in np.longdouble through a coordinate-form triple product.
"""
import functools

import numpy as np
import scipy.sparse as sp

import thermal_cpu as tc


class Op:
    """a sparse matrix in coordinate form, duplicates summed, of any dtype"""

    def __init__(self, shape, rows, cols, vals):
        self.shape = shape
        key = rows.astype(np.int64) * shape[1] + cols
        order = np.argsort(key, kind="stable")
        key, vals = key[order], vals[order]
        if key.size:
            starts = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
            key, vals = key[starts], np.add.reduceat(vals, starts)
        self.rows, self.cols, self.vals = key // shape[1], key % shape[1], vals
        self.dtype = vals.dtype

    @classmethod
    def from_scipy(cls, M):
        M = M.tocoo()
        return cls(M.shape, M.row.astype(np.int64), M.col.astype(np.int64), M.data.astype(np.float64))

    def scipy(self):
        return sp.csr_matrix((self.vals.astype(np.float64), (self.rows, self.cols)), shape=self.shape)

    def _sum(self, idx, terms, n):
        if self.dtype == np.float64:
            return np.bincount(idx, weights=terms, minlength=n)
        out = np.zeros(n, dtype=self.dtype)
        np.add.at(out, idx, terms)
        return out

    def matvec(self, x):
        return self._sum(self.rows, self.vals * x[self.cols], self.shape[0])

    def rmatvec(self, y):
        """the transpose times y"""
        return self._sum(self.cols, self.vals * y[self.rows], self.shape[1])

    def diagonal(self):
        d = np.zeros(self.shape[0], dtype=self.dtype)
        on = self.rows == self.cols
        d[self.rows[on]] = self.vals[on]
        return d

    def dense(self):
        M = np.zeros(self.shape, dtype=self.dtype)
        M[self.rows, self.cols] = self.vals
        return M

    def take_rows(self, sel):
        """the rows `sel` (ascending node indices) as an Op of len(sel) rows"""
        local = np.full(self.shape[0], -1, dtype=np.int64)
        local[sel] = np.arange(sel.size)
        keep = local[self.rows] >= 0
        return Op((sel.size, self.shape[1]), local[self.rows[keep]], self.cols[keep], self.vals[keep])


def level_extents(ne, max_coarsenings=-1):
    out = [tuple(int(n) for n in ne)]
    while (max_coarsenings < 0 or len(out) - 1 < max_coarsenings) and all(n % 2 == 0 and n >= 4 for n in out[-1]):
        out.append(tuple(n // 2 for n in out[-1]))
    return out


def node_index_grid(ne):
    """[nodes, N] integer coordinates, last axis fastest"""
    return np.stack(np.meshgrid(*[np.arange(n + 1) for n in ne], indexing="ij"), axis=-1).reshape(-1, len(ne))


def coarse_mask(ne_f, fixed_f):
    return np.ascontiguousarray(fixed_f.reshape([n + 1 for n in ne_f])[tuple(slice(None, None, 2) for _ in ne_f)]).reshape(-1)


def interpolation(ne_f, dtype=np.float64):
    """I_l as an Op [fine nodes, coarse nodes]: an even fine index 2 j takes coarse j, an odd one 2 j + 1 half of j and half of j + 1"""
    N = len(ne_f)
    ne_c = tuple(n // 2 for n in ne_f)
    idx = node_index_grid(ne_f)
    rows, cols, vals = [], [], []
    for m in range(2 ** N):
        bits = [(m >> (N - 1 - d)) & 1 for d in range(N)]
        w = np.ones(idx.shape[0], dtype=dtype)
        j = np.empty_like(idx)
        used = np.ones(idx.shape[0], dtype=bool)
        for d in range(N):
            odd = idx[:, d] % 2 == 1
            j[:, d] = idx[:, d] // 2 + bits[d]
            used &= odd | (bits[d] == 0)
            w = np.where(odd, w / 2, w)
        rows.append(np.flatnonzero(used))
        cols.append(np.ravel_multi_index(tuple(j[used].T), tuple(n + 1 for n in ne_c)))
        vals.append(w[used])
    return Op((tc.num_nodes(ne_f), tc.num_nodes(ne_c)), np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def prolongation(ne_f, fixed_f, fixed_c, dtype=np.float64):
    """P_l = F_l I_l F_{l+1}"""
    I = interpolation(ne_f, dtype)
    keep = ~fixed_f[I.rows] & ~fixed_c[I.cols]
    return Op(I.shape, I.rows[keep], I.cols[keep], I.vals[keep])


def fine_operator(ne, Kc0, kap, fixed, dtype=np.float64):
    """A'_0 = F_0 (sum_e kappa_e Kc0) F_0"""
    en = tc.element_nodes(ne)
    npe = en.shape[1]
    rows = np.repeat(en, npe, axis=1).reshape(-1)
    cols = np.tile(en, (1, npe)).reshape(-1)
    vals = (kap.astype(dtype)[:, None, None] * Kc0.astype(dtype)[None]).reshape(-1)
    keep = ~fixed[rows] & ~fixed[cols]
    n = tc.num_nodes(ne)
    return Op((n, n), rows[keep], cols[keep], vals[keep])


def galerkin(P, A):
    """P^T A P: scipy.sparse in float64, a coordinate-form triple product otherwise"""
    if A.dtype == np.float64:
        Ps = P.scipy()
        return Op.from_scipy((Ps.T @ A.scipy() @ Ps).tocoo())
    # the entries of P by fine row: at most `width` per row
    order = np.argsort(P.rows, kind="stable")
    pr, pc, pv = P.rows[order], P.cols[order], P.vals[order]
    count = np.bincount(pr, minlength=P.shape[0])
    width = int(count.max()) if count.size else 0
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    slot = np.arange(pr.size) - start[pr]
    C = np.zeros((P.shape[0], width), dtype=np.int64)
    W = np.zeros((P.shape[0], width), dtype=A.dtype)
    C[pr, slot], W[pr, slot] = pc, pv
    rows = np.repeat(C[A.rows], width, axis=1).reshape(-1)
    cols = np.tile(C[A.cols], (1, width)).reshape(-1)
    vals = (W[A.rows][:, :, None] * A.vals[:, None, None] * W[A.cols][:, None, :]).reshape(-1)
    keep = vals != 0
    return Op((P.shape[1], P.shape[1]), rows[keep], cols[keep], vals[keep])


def with_identity(Ap, fixed):
    """A_l = A'_l + (I - F_l)"""
    f = np.flatnonzero(fixed)
    return Op(Ap.shape, np.concatenate([Ap.rows, f]), np.concatenate([Ap.cols, f]), np.concatenate([Ap.vals, np.ones(f.size, dtype=Ap.dtype)]))


def colour_nodes(ne):
    """the node indices of the 2^N colours in ascending colour order"""
    N = len(ne)
    idx = node_index_grid(ne)
    colour = np.zeros(idx.shape[0], dtype=np.int64)
    for d in range(N):
        colour = 2 * colour + idx[:, d] % 2
    return [np.flatnonzero(colour == m) for m in range(2 ** N)]


class Hierarchy:
    """levels (elements per axis), masks, P_l, A'_l and A_l as Ops, the colour rows of A_l and the dense coarsest matrix"""

    def __init__(self, ne, Kc0, kap, fixed, max_coarsenings=-1, dtype=np.float64):
        self.dtype = dtype
        self.ne = level_extents(ne, max_coarsenings)
        self.fixed = [np.asarray(fixed, dtype=bool).reshape(-1)]
        for l in range(1, len(self.ne)):
            self.fixed.append(coarse_mask(self.ne[l - 1], self.fixed[-1]))
        self.P, self.Ap = [], [fine_operator(ne, Kc0, kap, self.fixed[0], dtype)]
        for l in range(1, len(self.ne)):
            self.P.append(prolongation(self.ne[l - 1], self.fixed[l - 1], self.fixed[l], dtype))
            self.Ap.append(galerkin(self.P[-1], self.Ap[-1]))
        self.A = [with_identity(Ap, f) for Ap, f in zip(self.Ap, self.fixed)]
        self.diag = [A.diagonal() for A in self.A]
        self.colours = [[(sel, A.take_rows(sel)) for sel in colour_nodes(e) if sel.size] for e, A in zip(self.ne, self.A)]
        self.coarsest = self.A[-1].dense().astype(np.float64)

    @property
    def last(self):
        return len(self.ne) - 1

    def sweep(self, l, x, b, forward=True):
        """one colour sweep of A_l x = b, in place on a copy"""
        x = x.astype(self.dtype).copy()
        for sel, rows in (self.colours[l] if forward else self.colours[l][::-1]):
            x[sel] = x[sel] + (b[sel] - rows.matvec(x)) / self.diag[l][sel]
        return x

    def restrict(self, l, r):
        return self.P[l].rmatvec(r.astype(self.dtype))

    def prolong_add(self, l, xc, xf):
        return xf.astype(self.dtype) + self.P[l].matvec(xc.astype(self.dtype))

    def solve_coarsest(self, b):
        """A_L^-1 b: float64 LAPACK, refined with residuals in the hierarchy's dtype"""
        x = np.linalg.solve(self.coarsest, b.astype(np.float64)).astype(self.dtype)
        if self.dtype != np.float64:
            for _ in range(3):
                x = x + np.linalg.solve(self.coarsest, (b - self.A[-1].matvec(x)).astype(np.float64)).astype(self.dtype)
        return x

    def vcycle(self, b, smoothing=1, l=0):
        b = b.astype(self.dtype)
        if l == self.last:
            return self.solve_coarsest(b)
        x = np.zeros_like(b)
        for _ in range(smoothing):
            x = self.sweep(l, x, b, True)
        r = b - self.A[l].matvec(x)
        x = self.prolong_add(l, self.vcycle(self.restrict(l, r), smoothing, l + 1), x)
        for _ in range(smoothing):
            x = self.sweep(l, x, b, False)
        return x

    def pcg(self, b, x0=None, tol=1e-8, max_iter=2000, smoothing=1):
        """CG preconditioned by one V-cycle, with the device's rule: it stops when the recurrence residual has |r| / |b| <= tol, looked
        at before the first and after every iteration.  Returns x and a dict as thermal_cpu.pcg does"""
        A = self.A[0]
        x = np.zeros_like(b) if x0 is None else x0.copy()
        r = b - A.matvec(x)
        bb, rr = float(b @ b), float(r @ r)
        if bb == 0.0:
            return np.zeros_like(b), dict(iterations=0, converged=True, relres=0.0, true_relres=0.0, gap=0.0)
        it, done = 0, rr <= tol * tol * bb
        d = rz_old = None
        while not done and it < max_iter:
            it += 1
            z = self.vcycle(r, smoothing)
            rz = float(r @ z)
            d = z if it == 1 else z + (rz / rz_old) * d
            Ad = A.matvec(d)
            alpha = rz / float(d @ Ad)
            x = x + alpha * d
            r = r - alpha * Ad
            rr, rz_old = float(r @ r), rz
            done = rr <= tol * tol * bb
        true = float(np.linalg.norm(b - A.matvec(x)) / np.sqrt(bb))
        rel = float(np.sqrt(rr / bb))
        return x, dict(iterations=it, converged=done, relres=rel, true_relres=true, gap=abs(true - rel))


def probing_vectors(ne, dtype=np.float64):
    """3^N vectors, each the sum of the unit vectors of the nodes with one residue of the index mod 3 per axis: a 3^N-point operator
    applied to one of them returns, at every node, the single coefficient that couples it to the one node of the set it reaches"""
    idx = node_index_grid(ne)
    N = len(ne)
    key = np.zeros(idx.shape[0], dtype=np.int64)
    for d in range(N):
        key = 3 * key + idx[:, d] % 3
    return [(key == s).astype(dtype) for s in range(3 ** N)]


# ---- fixtures shared with the GPU tests ----

def random_mask(ne, seed=0):
    """about 20 % of the nodes fixed at random"""
    return np.random.default_rng(4100 + seed + tc.num_elements(ne)).uniform(size=tc.num_nodes(ne)) < 0.2


@functools.lru_cache(maxsize=None)
def case(ne, mask="sink"):
    """random kappa from rho in [0.05, 1], the anisotropic conductivity and the edge lengths of thermal_cpu, and one of two masks: the
    middle-third sink on the face x = 0, or 20 % random fixed nodes"""
    N = len(ne)
    rng = np.random.default_rng(4000 + tc.num_elements(ne))
    kap = tc.kappa(rng.uniform(0.05, 1.0, size=tc.num_elements(ne)))
    fixed = tc.face_mask(ne, 0, 0, middle_third=True) if mask == "sink" else random_mask(ne)
    Kc0 = np.ascontiguousarray(tc.conductivity_matrix(tc.K_ANISO[N], tc.EDGES[N]))
    nn = tc.num_nodes(ne)
    return dict(ne=ne, N=N, Kc0=Kc0, kap=kap, fixed=fixed, X=rng.standard_normal(nn), B=rng.standard_normal(nn))


@functools.lru_cache(maxsize=None)
def case_hierarchy(ne, mask="sink", long=False):
    c = case(ne, mask)
    return Hierarchy(ne, c["Kc0"], c["kap"], c["fixed"], dtype=np.longdouble if long else np.float64)


@functools.lru_cache(maxsize=None)
def pcg_data(ne):
    """the data of thermal_cpu.pcg_fixture(ne) without its dense matrix, which the growth grids cannot hold (tests/test_thermal_mg_cpu.py
    checks that the two agree)"""
    N = len(ne)
    rho = np.random.default_rng(1600 + tc.num_elements(ne)).uniform(0.05, 1.0, size=tc.num_elements(ne))
    h = (1.0,) * N
    fixed = tc.face_mask(ne, 0, 0, middle_third=True)
    return dict(ne=ne, h=h, rho=rho, fixed=fixed, Kc0=tc.conductivity_matrix(1.0, h), Q=tc.load(ne, h, fixed, volumetric=1.0))


@functools.lru_cache(maxsize=None)
def pcg_hierarchy(ne):
    f = pcg_data(ne)
    return Hierarchy(ne, f["Kc0"], tc.kappa(f["rho"]), f["fixed"])


@functools.lru_cache(maxsize=None)
def pcg_solution(ne, smoothing=1):
    """(x, info) of the restatement's PCG on pcg_data(ne) at tol 1e-8"""
    return pcg_hierarchy(ne).pcg(pcg_data(ne)["Q"], tol=1e-8, smoothing=smoothing)


def direct_solve(H, b):
    """A_0^-1 b by a sparse LU factorisation: what the PCG solutions are compared with (the dense solve of thermal_cpu, affordable on
    the long grids)"""
    import scipy.sparse.linalg as spla
    return spla.spsolve(H.A[0].scipy().tocsc(), b)


@functools.lru_cache(maxsize=None)
def pcg_direct(ne):
    return direct_solve(pcg_hierarchy(ne), pcg_data(ne)["Q"])


# what Hierarchy.pcg takes on thermal_cpu.pcg_fixture at tol 1e-8 (tests/test_thermal_mg_cpu.py recomputes and pins them)
PCG_SHAPES = [(40, 36), (12, 264), (12, 8, 16), (4, 4, 136)]
PCG_COUNT = {1: {(40, 36): 23, (12, 264): 25, (12, 8, 16): 12, (4, 4, 136): 14},
             2: {(40, 36): 18, (12, 264): 20, (12, 8, 16): 9, (4, 4, 136): 11}}
GROWTH_COUNT = {(32, 32): 20, (64, 64): 23, (128, 128): 25, (16, 16, 16): 11, (32, 32, 32): 12}
