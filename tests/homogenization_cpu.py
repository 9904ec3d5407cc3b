"""numpy / scipy restatement of periodic homogenisation on a voxel cell, for the tests.  Nothing here comes from the library: the
element matrix K0 and the element loads L are integrated by 2-point Gauss quadrature from the flattened tensor D, the periodic
matrix is assembled through the node map and solved by SuperLU; the same block-Jacobi PCG as the device runs is here for
iteration counts.

Conventions: flattened strain order xx yy xy (2-D) / xx yy zz yz xz xy (3-D), D holds tensor components (a shear row carries no
factor 2), the unit strain e_q has 0.5 on both off-diagonal entries of a shear case, so C : e_q is row q of D.  Periodic node
(i_0, .., i_{N-1}) with the last axis fastest; element e owns the nodes (e_d + mu_d) mod ne_d, local node index with axis 0 as
the most significant bit, dof = N * node + component.  Node 0 is pinned.

    K_per w_q = - sum_e E_e L[:, q]                                                     (cell problems)
    Eh[q, r]  = 1/|Y| sum_e E_e (w_{q,e} . L[:, r] + vol D[q, r])                       (homogenised tensor, stress-like)
    G_e[q, r] = 1/|Y| (w_{q,e}^T K0 w_{r,e} + w_{q,e} . L[:, r] + L[:, q] . w_{r,e} + vol D[q, r]),  sum_e E_e G_e = Eh
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

PAIRS = {2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]}


def element_constants(D, h):
    """(K0 [ke, ke], L [ke, S], vol) of a box voxel with edge lengths h for the flattened tensor D"""
    D = np.asarray(D, dtype=np.float64)
    h = [float(v) for v in h]
    N = len(h)
    pairs = PAIRS[N]
    S, npe = len(pairs), 2 ** N
    mult = np.array([1.0 if i == j else 2.0 for i, j in pairs])
    loc = list(np.ndindex(*([2] * N)))
    gauss = (0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0))
    vol = float(np.prod(h))
    K0, L = np.zeros((N * npe, N * npe)), np.zeros((N * npe, S))
    for q in np.ndindex(*([2] * N)):
        x = [gauss[i] for i in q]
        grad = np.zeros((npe, N))
        for n, l in enumerate(loc):
            for d in range(N):
                v = 1.0
                for e in range(N):
                    if e == d:
                        v *= (1.0 if l[e] else -1.0) / h[e]
                    else:
                        v *= x[e] if l[e] else 1.0 - x[e]
                grad[n, d] = v
        B = np.zeros((S, N * npe))                   # tensor components of the strain of every dof
        for n in range(npe):
            for r, (i, j) in enumerate(pairs):
                if i == j:
                    B[r, N * n + i] = grad[n, i]
                else:
                    B[r, N * n + i] += 0.5 * grad[n, j]
                    B[r, N * n + j] += 0.5 * grad[n, i]
        MB = mult[:, None] * B                       # eps : sigma = sum_r mult_r eps_r sigma_r
        wgt = vol * 0.5 ** N
        K0 += wgt * MB.T @ D @ MB
        L += wgt * MB.T @ D
    return K0, L, vol


def element_nodes(ne):
    """[numElements, 2^N] periodic node indices"""
    ne = [int(n) for n in ne]
    N = len(ne)
    e = np.stack(np.meshgrid(*[np.arange(n) for n in ne], indexing="ij"), -1).reshape(-1, N)
    out = []
    for mu in np.ndindex(*([2] * N)):
        out.append(np.ravel_multi_index(tuple((e[:, d] + mu[d]) % ne[d] for d in range(N)), ne))
    return np.stack(out, axis=1)


def node_map(ne):
    """periodic node index of every node of the full (ne + 1) grid"""
    ne = [int(n) for n in ne]
    idx = np.stack(np.meshgrid(*[np.arange(n + 1) for n in ne], indexing="ij"), -1).reshape(-1, len(ne))
    return np.ravel_multi_index(tuple(idx[:, d] % ne[d] for d in range(len(ne))), ne)


def moduli(rho, E0, Emin, gamma):
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    return Emin + rho ** gamma * (E0 - Emin), gamma * rho ** (gamma - 1.0) * (E0 - Emin)


def _dofs(ne):
    N = len(ne)
    return (N * element_nodes(ne)[:, :, None] + np.arange(N)[None, None, :]).reshape(-1, N * 2 ** N)


def assemble(ne, K0, E):
    """the periodic stiffness matrix (csr) with the pin's rows and columns replaced by the identity"""
    N = len(ne)
    nd = N * int(np.prod(ne))
    dofs = _dofs(ne)
    ke = dofs.shape[1]
    rows = np.repeat(dofs, ke, axis=1).reshape(-1)
    cols = np.tile(dofs, (1, ke)).reshape(-1)
    vals = (np.asarray(E)[:, None, None] * K0[None]).reshape(-1)
    K = sp.coo_matrix((vals, (rows, cols)), shape=(nd, nd)).tocsr()         # duplicates (wrapped neighbours) are summed
    keep = np.ones(nd)
    keep[:N] = 0.0
    P = sp.diags(keep)
    return (P @ K @ P + sp.diags(1.0 - keep)).tocsr()


def rhs(ne, L, E):
    """[S, nd]: - sum_e E_e L[:, q] scattered to the periodic nodes, zero at the pin"""
    N = len(ne)
    nd = N * int(np.prod(ne))
    dofs = _dofs(ne)
    b = np.zeros((L.shape[1], nd))
    for q in range(L.shape[1]):
        np.add.at(b[q], dofs.reshape(-1), -(np.asarray(E)[:, None] * L[None, :, q]).reshape(-1))
    b[:, :N] = 0.0
    return b


def solve_direct(K, b):
    lu = spla.splu(K.tocsc())
    return np.stack([lu.solve(bq) for bq in b])


def block_jacobi(K, N):
    """inverses of the N x N node blocks, [nodes, N, N]"""
    nd = K.shape[0]
    blocks = np.zeros((nd // N, N, N))
    for a in range(N):
        for c in range(N):
            blocks[:, a, c] = np.asarray(K[np.arange(a, nd, N), np.arange(c, nd, N)]).reshape(-1)
    return np.linalg.inv(blocks)


def pcg_columns(K, b, N, tol, max_iter=100000):
    """block-Jacobi PCG from x = 0 to |r| / |b| <= tol for every row of b; returns (x [S, nd], iterations [S])"""
    Minv = block_jacobi(K, N)
    prec = lambda r: np.einsum("nab,nb->na", Minv, r.reshape(-1, N)).reshape(-1)
    xs, its = [], []
    for bq in b:
        x = np.zeros_like(bq)
        bb = float(bq @ bq)
        it = 0
        if bb > 0.0:
            r = bq.copy()
            z = prec(r)
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
                z = prec(r)
                rz_new = float(r @ z)
                p = z + (rz_new / rz) * p
                rz = rz_new
        xs.append(x)
        its.append(it)
    return np.stack(xs), its


def element_vectors(ne, W):
    """[S, numElements, ke] from W [S, nd]"""
    return np.asarray(W)[:, _dofs(ne)]


def tensor(ne, W, L, D, vol, E, cell_volume=None):
    cell = vol * int(np.prod(ne)) if not cell_volume else float(cell_volume)
    we = element_vectors(ne, W)
    E = np.asarray(E)
    return (np.einsum("e,qek,kr->qr", E, we, L) + E.sum() * vol * np.asarray(D)) / cell


def gradient(ne, W, K0, L, D, vol, cell_volume=None):
    """G [numElements, S, S] (without dE/drho): the upper triangle computed and mirrored"""
    cell = vol * int(np.prod(ne)) if not cell_volume else float(cell_volume)
    we = element_vectors(ne, W)
    G = np.einsum("qek,kl,rel->eqr", we, K0, we) + np.einsum("qek,kr->eqr", we, L) + np.einsum("kq,rek->eqr", L, we) + vol * np.asarray(D)[None]
    G = np.triu(G) + np.transpose(np.triu(G, 1), (0, 2, 1))
    return G / cell


def to_full(ne, W):
    """[S, nd] on the periodic grid -> [S, numNodes, N] on the full node grid"""
    N = len(ne)
    return np.asarray(W).reshape(len(W), -1, N)[:, node_map(ne)]


def homogenize(ne, h, D, rho, E0=1.0, Emin=0.0, gamma=1.0):
    """everything by the direct solve: dict with K0, L, vol, E, dE, K, b, W, Eh, G"""
    K0, L, vol = element_constants(D, h)
    E, dE = moduli(rho, E0, Emin, gamma)
    K = assemble(ne, K0, E)
    b = rhs(ne, L, E)
    W = solve_direct(K, b)
    return dict(K0=K0, L=L, vol=vol, E=E, dE=dE, K=K, b=b, W=W, Eh=tensor(ne, W, L, D, vol, E), G=gradient(ne, W, K0, L, D, vol))


def lame(E, nu):
    return nu * E / ((1.0 + nu) * (1.0 - 2.0 * nu)), E / (2.0 + 2.0 * nu)


def laminate_closed_form(phases, fractions):
    """flattened 6 x 6 tensor of a laminate of isotropic phases [(lambda, mu), ..] layered normal to x: harmonic means for
    C_xxxx, C_xyxy, C_xzxz, the arithmetic mean for C_yzyz, the standard mixed formulas for the rest (< > = volume average,
    M = lambda + 2 mu):
      C_xxxx = 1 / <1/M>,  C_xxyy = C_xxzz = <lambda/M> C_xxxx,
      C_yyyy = C_zzzz = <M - lambda^2/M> + <lambda/M>^2 C_xxxx,  C_yyzz = <lambda - lambda^2/M> + <lambda/M>^2 C_xxxx"""
    f = np.asarray(fractions, dtype=np.float64)
    lam = np.array([p[0] for p in phases])
    mu = np.array([p[1] for p in phases])
    M = lam + 2.0 * mu
    avg = lambda v: float(np.sum(f * v))
    cxx = 1.0 / avg(1.0 / M)
    D = np.zeros((6, 6))
    D[0, 0] = cxx
    D[0, 1] = D[1, 0] = D[0, 2] = D[2, 0] = avg(lam / M) * cxx
    D[1, 1] = D[2, 2] = avg(M - lam ** 2 / M) + avg(lam / M) ** 2 * cxx
    D[1, 2] = D[2, 1] = avg(lam - lam ** 2 / M) + avg(lam / M) ** 2 * cxx
    D[3, 3] = avg(mu)
    D[4, 4] = D[5, 5] = 1.0 / avg(1.0 / mu)
    return D


def isotropic_D(E, nu, N=3):
    lam, mu = lame(E, nu) if N == 3 else (nu * E / (1.0 - nu * nu), E / (2.0 + 2.0 * nu))
    S = len(PAIRS[N])
    D = np.zeros((S, S))
    D[:N, :N] = lam
    D[np.arange(N), np.arange(N)] = lam + 2.0 * mu
    D[np.arange(N, S), np.arange(N, S)] = mu
    return D


def rotation(axis, angle):
    """rotation matrix about ``axis`` (Rodrigues)"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * A + (1.0 - np.cos(angle)) * A @ A
