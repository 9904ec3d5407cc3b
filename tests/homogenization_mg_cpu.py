"""scipy restatement of the multigrid-preconditioned PCG for the periodic cell problems, built on homogenization_cpu.  Nothing
here comes from the library.

Levels: level 0 is the cell, level l + 1 has n_d / 2 periodic nodes per axis; a level is coarsened only while every n_d is even
and at least 4.  P is the periodic N-linear interpolation (x) I_N: fine index 2 j takes coarse j with weight 1, fine index
2 j + 1 takes coarse j and (j + 1) mod n_c with weight 1/2 each.  Restriction is P^T, unscaled.  A_0 is the unpinned periodic
matrix, A_{l+1} = P^T A_l P; the operator used on a level is A_l with the rows and columns of node 0 replaced by the identity
(``pinned``), and the transfers carry a zero at coarse node 0 (``Z P^T`` and ``P Z``, Z = identity without node 0).

Smoother: 2^N-colour block Gauss-Seidel, colour = parity of the node index along every axis with axis 0 as the most significant
bit, the N x N diagonal block inverted; ``smoothing`` sweeps in ascending colour order before the coarse correction and as many
in descending order after it.  The coarsest level is solved exactly (SuperLU, or an explicit inverse for comparison).  From a zero
initial guess the V-cycle is a symmetric positive definite operator."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import homogenization_cpu as hc


def level_dims(ne, levels=None):
    """per-level cell sizes: [[n_0, ..], [n_0 / 2, ..], ..]; ``levels`` caps the number of coarsenings"""
    dims = [[int(n) for n in ne]]
    while (levels is None or len(dims) - 1 < levels) and all(n % 2 == 0 and n >= 4 for n in dims[-1]):
        dims.append([n // 2 for n in dims[-1]])
    return dims


def prolongation_1d(nf):
    nc = nf // 2
    P = sp.lil_matrix((nf, nc))
    for j in range(nc):
        P[2 * j, j] += 1.0
        P[2 * j + 1, j] += 0.5
        P[2 * j + 1, (j + 1) % nc] += 0.5
    return P.tocsr()


def prolongation(nf, N):
    """P of one coarsening of the level with nf nodes per axis, acting on [node][component] vectors"""
    P = prolongation_1d(nf[0])
    for n in nf[1:]:
        P = sp.kron(P, prolongation_1d(n), format="csr")
    return sp.kron(P, sp.identity(N), format="csr")


def assemble_unpinned(ne, K0, E):
    N = len(ne)
    nd = N * int(np.prod(ne))
    dofs = hc._dofs(ne)
    ke = dofs.shape[1]
    rows = np.repeat(dofs, ke, axis=1).reshape(-1)
    cols = np.tile(dofs, (1, ke)).reshape(-1)
    vals = (np.asarray(E)[:, None, None] * K0[None]).reshape(-1)
    return sp.coo_matrix((vals, (rows, cols)), shape=(nd, nd)).tocsr()


def _keep(nd, N):
    keep = np.ones(nd)
    keep[:N] = 0.0
    return keep


def pinned(A, N):
    keep = _keep(A.shape[0], N)
    Z = sp.diags(keep)
    return (Z @ A @ Z + sp.diags(1.0 - keep)).tocsr()


def colours(n, N):
    """colour of every node of a level (parity per axis, axis 0 the most significant bit) as dof index lists, ascending"""
    idx = np.stack(np.meshgrid(*[np.arange(m) for m in n], indexing="ij"), -1).reshape(-1, N)
    col = np.zeros(len(idx), dtype=np.int64)
    for d in range(N):
        col = 2 * col + idx[:, d] % 2
    out = []
    for c in range(2 ** N):
        nodes = np.nonzero(col == c)[0]
        out.append((N * nodes[:, None] + np.arange(N)[None, :]).reshape(-1))
    return out


class Hierarchy:
    def __init__(self, ne, K0, E, levels=None, coarsest="splu"):
        self.N = N = len(ne)
        self.dims = level_dims(ne, levels)
        self.A = [assemble_unpinned(ne, K0, E)]          # unpinned Galerkin operators
        self.P = []                                        # P[l]: level l + 1 -> level l, zero column at coarse node 0
        for n in self.dims[:-1]:
            P = prolongation(n, N)
            self.A.append((P.T @ self.A[-1] @ P).tocsr())
            self.P.append((P @ sp.diags(_keep(P.shape[1], N))).tocsr())
        self.K = [pinned(A, N) for A in self.A]           # the operators used
        self.R = [P.T.tocsr() for P in self.P]
        self.colours = [colours(n, N) for n in self.dims]
        self.Dinv = [hc.block_jacobi(K, N) for K in self.K]
        Kc = self.K[-1]
        if coarsest == "splu":
            lu = spla.splu(Kc.tocsc())
            self.coarse_solve = lu.solve
        else:
            inv = np.linalg.inv(Kc.toarray())
            self.coarse_solve = lambda b: inv @ b

    def sweep(self, l, x, b, forward):
        """one block Gauss-Seidel sweep over all colours of level l, in place"""
        K, N = self.K[l], self.N
        order = self.colours[l] if forward else self.colours[l][::-1]
        for dofs in order:
            r = b[dofs] - K[dofs] @ x
            nodes = dofs[::N] // N
            x[dofs] += np.einsum("nab,nb->na", self.Dinv[l][nodes], r.reshape(-1, N)).reshape(-1)
        return x

    def vcycle(self, b, smoothing=1, l=0):
        if l == len(self.dims) - 1:
            return self.coarse_solve(b)
        x = np.zeros_like(b)
        for _ in range(smoothing):
            self.sweep(l, x, b, True)
        x += self.P[l] @ self.vcycle(self.R[l] @ (b - self.K[l] @ x), smoothing, l + 1)
        for _ in range(smoothing):
            self.sweep(l, x, b, False)
        return x


def pcg_columns(h, b, tol, smoothing=1, max_iter=10000):
    """multigrid PCG from x = 0 to |r| / |b| <= tol for every row of b; returns (x [S, nd], iterations [S])"""
    K = h.K[0]
    xs, its = [], []
    for bq in b:
        x = np.zeros_like(bq)
        bb = float(bq @ bq)
        it = 0
        if bb > 0.0:
            r = bq.copy()
            z = h.vcycle(r, smoothing)
            p = z.copy()
            rz = float(r @ z)
            while it < max_iter:
                Ap = K @ p
                alpha = rz / float(p @ Ap)
                x += alpha * p
                r -= alpha * Ap
                it += 1
                if float(r @ r) <= tol * tol * bb:
                    break
                z = h.vcycle(r, smoothing)
                rz_new = float(r @ z)
                p = z + (rz_new / rz) * p
                rz = rz_new
        xs.append(x)
        its.append(it)
    return np.stack(xs), its


def void_density(ne, radius=0.3, inside=0.0):
    """1 outside, ``inside`` within a centred sphere (disc) of the given radius on the unit cell, by element centres"""
    c = np.stack(np.meshgrid(*[(np.arange(n) + 0.5) / n for n in ne], indexing="ij"), -1)
    rho = np.ones(ne)
    rho[np.sum((c - 0.5) ** 2, axis=-1) < radius ** 2] = inside
    return rho


def void_problem(ne, Emin=1e-3):
    """the grid-independence cell: isotropic E = 1, nu = 0.3, gamma = 1, spherical (disc) void of radius 0.3 on the unit cell.
    Returns (K0, L, vol, E, b)"""
    N = len(ne)
    D = hc.isotropic_D(1.0, 0.3, N)
    K0, L, vol = hc.element_constants(D, [1.0 / n for n in ne])
    E, _ = hc.moduli(void_density(ne), 1.0, Emin, 1.0)
    return K0, L, vol, E, hc.rhs(ne, L, E)


def void_iterations(ne, tol=1e-10, smoothing=1, jacobi=False):
    """(multigrid PCG iterations, block-Jacobi PCG iterations or None) of the void cell"""
    K0, L, vol, E, b = void_problem(ne)
    h = Hierarchy(ne, K0, E)
    _, its = pcg_columns(h, b, tol, smoothing)
    return its, (hc.pcg_columns(h.K[0], b, len(ne), tol)[1] if jacobi else None)


# the small cells of the tests: (elements, voxel edge lengths, material, seed of the densities); random densities in [0.05, 1],
# gamma = 3, E_min = 1e-3, E_0 = 1
CELLS = {"12x8x16": ((12, 8, 16), (1.0, 0.8, 1.3), "aniso3", 51), "16x12": ((16, 12), (1.0, 0.7), "aniso2", 52),
         "8x4x12": ((8, 4, 12), (1.0, 1.0, 1.0), "iso3", 53), "5x3x7": ((5, 3, 7), (1.0, 0.9, 1.4), "iso3", 54)}


def cell_density(name):
    ne, _, _, seed = CELLS[name]
    return np.random.default_rng(seed).uniform(0.05, 1.0, size=ne)


def kind_D(kind):
    import material_ref as mr
    if kind == "aniso3":
        return mr.material_file_D(mr.ANISO_3D)
    if kind == "aniso2":
        return mr.material_file_D(mr.ANISO_2D)
    return hc.isotropic_D(1.0, 0.3, int(kind[-1]))              # "iso2" / "iso3"


def cell_D(name):
    return kind_D(CELLS[name][2])


def cell_reference(name):
    """the direct solution of a test cell (hc.homogenize) with the unpinned hierarchy's ingredients"""
    ne, h, _, _ = CELLS[name]
    return hc.homogenize(ne, h, cell_D(name), cell_density(name), 1.0, 1e-3, 3.0)


# The cells of tests/test_gpu_homogenization_blocks.py, the smallest on which the device's kernels run in several 256-thread
# workgroups and its two-stage reductions see more than 256 (512) partials: (elements, voxel edge lengths, material, seed); random
# densities in [0.05, 1], gamma = 3, E_min = 1e-3, E_0 = 1.  Too large for a direct solve in a test: only the pieces are used.
BLOCK_CELLS = {"2d-blocks": ((72, 64), (1.0, 0.7), "aniso2", 61), "3d-blocks": ((28, 24, 28), (1.0, 0.8, 1.3), "aniso3", 62),
               "2d-partials": ((320, 256), (1.0, 0.7), "aniso2", 63),
               "tensor-2d": ((520, 260), (1.0, 0.7), "aniso2", 64), "tensor-3d": ((52, 52, 52), (1.0, 0.8, 1.3), "aniso3", 65)}
# Laminates normal to x, isotropic E = 1, nu = 0.3, gamma = 1, E_min = 0, whose strain cases need very different numbers of
# block-Jacobi iterations: (elements, voxel edge length, density of the second half)
LAMINATES = {"lam-2d": ((48, 6), 1.0 / 48, 0.1), "lam-3d": ((64, 4, 4), 1.0 / 64, 0.5)}
# uniform cells of density 0.7 (a zero right-hand side up to rounding): (elements, voxel edge lengths, material)
UNIFORM_CELLS = {"6x4x8": ((6, 4, 8), (1.0, 0.8, 1.3), "aniso3"), "8x6": ((8, 6), (1.0, 0.7), "aniso2")}
THREADS = 256                                                    # the device's workgroup size (HOM_THREADS)


def block_cell(name):
    """(ne, h, D, rho, gamma, E_min) of a cell of BLOCK_CELLS, LAMINATES, UNIFORM_CELLS or of the singular cell ``void-2d``: 12 x 12 on
    the unit square, isotropic, gamma = 1, E_min = 0, density 1 except a 4 x 4 block of zeros, so that the nine nodes inside the block
    have no stiffness at all"""
    if name in BLOCK_CELLS:
        ne, h, kind, seed = BLOCK_CELLS[name]
        return ne, h, kind_D(kind), np.random.default_rng(seed).uniform(0.05, 1.0, size=ne), 3.0, 1e-3
    if name in LAMINATES:
        ne, edge, second = LAMINATES[name]
        rho = np.ones(ne)
        rho[ne[0] // 2:] = second
        return ne, (edge,) * len(ne), hc.isotropic_D(1.0, 0.3, len(ne)), rho, 1.0, 0.0
    if name in UNIFORM_CELLS:
        ne, h, kind = UNIFORM_CELLS[name]
        return ne, h, kind_D(kind), np.full(ne, 0.7), 3.0, 1e-3
    assert name == "void-2d"
    rho = np.ones((12, 12))
    rho[4:8, 4:8] = 0.0
    return (12, 12), (1.0 / 12,) * 2, hc.isotropic_D(1.0, 0.3, 2), rho, 1.0, 0.0


def block_problem(name):
    """dict with ne, N, D, K0, L, vol, E, dE, K (assembled, pinned) and b of ``block_cell(name)``: everything but a solve"""
    ne, h, D, rho, gamma, Emin = block_cell(name)
    K0, L, vol = hc.element_constants(D, h)
    E, dE = hc.moduli(rho, 1.0, Emin, gamma)
    return dict(ne=ne, N=len(ne), D=D, K0=K0, L=L, vol=vol, E=E, dE=dE, K=hc.assemble(ne, K0, E), b=hc.rhs(ne, L, E))


def workgroups(n):
    return -(-int(n) // THREADS)


if __name__ == "__main__":
    # python tests/homogenization_mg_cpu.py 16 16 16     -> the iteration counts of the void cell
    import sys
    ne = tuple(int(a) for a in sys.argv[1:]) or (16, 16, 16)
    print(ne, void_iterations(ne, jacobi=True))
