"""numpy / scipy fp64 restatement of the linearised buckling chain, for the tests.  Nothing here comes from the library: the
geometric element matrices are 2-point Gauss quadratures of stress_cpu.strain_matrix and the shape functions' gradients, K and K_G
are assembled by scipy on the full node grid, reduced to the free dofs and solved densely by ``scipy.linalg.eigh(K_G, K)``; the
iterative solve is modal_cpu.lobpcg on the same matrices with SuperLU's K^-1 as the preconditioner.

Conventions: those of stress_cpu (last axis fastest, local node index with axis 0 as the most significant bit, dof = N node + c).

    u = K^-1 f,   K_G,e[(n,a),(m,b)] = delta_ab mG_e sum_j u_ej T_j[n,m],   mG = rho^q E_0  (no E_min: void carries no stress)
    T_j[n,m] = int_e grad N_n^T (C : B_j(x)) grad N_m dV:  2^N N symmetric node matrices (the integrand has degree <= 3 per axis)
    K_G phi = nu K phi on the free dofs, phi^T K phi = 1, load factor lambda = -1 / nu for nu < 0, mu = 1 / lambda = -nu
    J = (sum_{i <= k} mu_i^P)^(1/P),  w_i = (mu_i / J)^(P-1)
    a = -sum_i w_i d(phi_i^T K_G phi_i)/du (0 at the fixed dofs),  K v = a
    dJ/drho_e = -sum_i w_i [dmG_e sum_j u_ej phi_ie^T T_j phi_ie - nu_i dE_e phi_ie^T K0 phi_ie] - dE_e v_e^T K0 u_e
"""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import homogenization_cpu as hc
import modal_cpu as mc
import stress_cpu as sc

E0, EMIN, GAMMA = 1.0, 1e-3, 3.0
NUM_MODES = 4
P_NORM = 8.0
# elements, edge lengths, (E, nu), load; densities uniform in [0.2, 1] from default_rng(0), the x = 0 face clamped
CASES = {"column2": ((16, 6), (0.125, 0.125), (1.0, 0.3), "column"),
         "column3": ((8, 4, 3), (0.25, 0.25, 0.25), (1.0, 0.3), "column"),
         "cantilever2": ((16, 12), (0.125, 0.125), (1.0, 0.3), "cantilever"),
         # (column3 with even extents: a multigrid hierarchy halves every axis, which 8 x 4 x 3 does not allow)
         "column3even": ((8, 4, 4), (0.25, 0.25, 0.25), (1.0, 0.3), "column")}


def shape_gradients(h, x):
    """grad N_n(x) [npe, N] at the point x of the unit cube scaled by h"""
    N = len(h)
    g = np.empty((2 ** N, N))
    for n, l in enumerate(np.ndindex(*([2] * N))):
        for d in range(N):
            v = 1.0
            for e in range(N):
                v *= ((1.0 if l[e] else -1.0) / h[e]) if e == d else (x[e] if l[e] else 1.0 - x[e])
            g[n, d] = v
    return g


def geometric_element_matrices(D, h):
    """T [ke, npe, npe]: K_G,e = mG_e sum_j u_ej T_j on the nodes, the identity across components"""
    D = np.asarray(D, dtype=np.float64)
    N = len(h)
    pairs = hc.PAIRS[N]
    npe = 2 ** N
    gauss = (0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0))
    T = np.zeros((N * npe, npe, npe))
    wgt = float(np.prod(h)) * 0.5 ** N
    for q in np.ndindex(*([2] * N)):
        x = [gauss[i] for i in q]
        g = shape_gradients(h, x)
        sig = D @ (sc.mult(N)[:, None] * sc.strain_matrix(h, x))          # [S, ke]: the stress of every unit dof
        for j in range(N * npe):
            s = np.zeros((N, N))
            for r, (a, b) in enumerate(pairs):
                s[a, b] = s[b, a] = sig[r, j]
            T[j] += wgt * g @ s @ g.T
    return T


def geometric_multiplier(rho, q=GAMMA, E0_=E0):
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    return rho ** q * E0_, q * rho ** (q - 1.0) * E0_


def element_nodes(ne):
    return sc.element_dofs(ne)[:, ::len(ne)] // len(ne)


def assemble_geometric(ne, T, mG, u):
    """K_G (csr) on the full node grid: kron(scalar node matrix, I_N)"""
    N = len(ne)
    ue = np.asarray(u, dtype=np.float64).reshape(-1)[sc.element_dofs(ne)]
    Ge = np.asarray(mG)[:, None, None] * np.einsum("ej,jnm->enm", ue, T)
    nodes = element_nodes(ne)
    npe = nodes.shape[1]
    rows, cols = np.repeat(nodes, npe, axis=1).reshape(-1), np.tile(nodes, (1, npe)).reshape(-1)
    nn = sc.num_nodes(ne)
    Gs = sp.coo_matrix((Ge.reshape(-1), (rows, cols)), shape=(nn, nn)).tocsr()
    return sp.kron(Gs, sp.identity(N), format="csr")


# ---- what the three kernels compute, in the number format asked for (the rounding floor of the formulas: longdouble against float64) ----

def kernel_apply(ne, T, mG, u, X, fixed=None, dtype=np.float64):
    """Y [cols, ndof] = P K_G(mG, u) P X, element by element"""
    N = len(ne)
    dofs, nodes = sc.element_dofs(ne), element_nodes(ne)
    T, mG, u = np.asarray(T, dtype=dtype), np.asarray(mG, dtype=dtype), np.asarray(u, dtype=dtype).reshape(-1)
    X = np.array(X, dtype=dtype).reshape(len(X), -1)
    keep = None if fixed is None else ~np.asarray(fixed, dtype=bool).reshape(-1)
    if keep is not None:
        X = X * keep
    Ge = mG[:, None, None] * np.einsum("ej,jnm->enm", u[dofs], T)
    Y = np.zeros_like(X)
    for c in range(len(X)):
        xe = X[c].reshape(-1, N)[nodes]                                    # [e, npe, N]
        ye = np.einsum("enm,emb->enb", Ge, xe)
        np.add.at(Y[c], dofs.reshape(-1), ye.reshape(-1))
    if keep is not None:
        Y = Y * keep
    return Y


def kernel_adjoint_load(ne, T, mG, Phi, coef, fixed=None, dtype=np.float64):
    """a [ndof] = sum_i coef_i d(phi_i^T K_G phi_i)/du, 0 at the fixed dofs; Phi [modes, ndof]"""
    N = len(ne)
    dofs, nodes = sc.element_dofs(ne), element_nodes(ne)
    T, mG = np.asarray(T, dtype=dtype), np.asarray(mG, dtype=dtype)
    a = np.zeros(sc.num_nodes(ne) * N, dtype=dtype)
    for i, c in enumerate(coef):
        pe = np.asarray(Phi[i], dtype=dtype).reshape(-1, N)[nodes]
        per = dtype(c) * mG[:, None] * np.einsum("enb,jnm,emb->ej", pe, T, pe)
        np.add.at(a, dofs.reshape(-1), per.reshape(-1))
    if fixed is not None:
        a[np.asarray(fixed, dtype=bool).reshape(-1)] = 0
    return a


def kernel_gradient(ne, T, K0, dmG, dE, u, v, Phi, cG, cK, dtype=np.float64):
    """g[e] = dmG_e sum_i cG_i sum_j u_ej phi_ie^T T_j phi_ie + dE_e (sum_i cK_i phi_ie^T K0 phi_ie - v_e^T K0 u_e)"""
    N = len(ne)
    dofs, nodes = sc.element_dofs(ne), element_nodes(ne)
    T, K0 = np.asarray(T, dtype=dtype), np.asarray(K0, dtype=dtype)
    dmG, dE = np.asarray(dmG, dtype=dtype), np.asarray(dE, dtype=dtype)
    ue, ve = np.asarray(u, dtype=dtype).reshape(-1)[dofs], np.asarray(v, dtype=dtype).reshape(-1)[dofs]
    sG, sK = np.zeros(len(dofs), dtype=dtype), -np.einsum("ek,kl,el->e", ve, K0, ue)
    for i in range(len(cG)):
        p = np.asarray(Phi[i], dtype=dtype).reshape(-1)
        pn, pe = p.reshape(-1, N)[nodes], p[dofs]
        sG = sG + dtype(cG[i]) * np.einsum("ej,enb,jnm,emb->e", ue, pn, T, pn)
        sK = sK + dtype(cK[i]) * np.einsum("ek,kl,el->e", pe, K0, pe)
    return dmG * sG + dE * sK


# ---- the fixtures ----

def end_load(ne, corner_half_weights=False):
    """[numNodes, N]: total 1 along -x over the nodes of the x = max face, spread evenly (or by the trapezoidal rule in 2-D)"""
    N = len(ne)
    nn = [int(n) + 1 for n in ne]
    f = np.zeros(nn + [N])
    w = np.ones(nn[1:])
    if corner_half_weights:
        assert N == 2
        w[0] = w[-1] = 0.5
    f[-1, ..., 0] = -w / w.sum()
    return f.reshape(-1, N)


def case(name):
    """(ne, h, D, rho, fixed [numNodes, N], f [numNodes, N])"""
    ne, h, (E, nu), load = CASES[name]
    rho = np.random.default_rng(0).uniform(0.2, 1.0, size=int(np.prod(ne)))
    fixed, f = sc.cantilever(ne)
    if load == "column":
        f = end_load(ne)
    return ne, h, hc.isotropic_D(E, nu, len(ne)), rho, fixed, f


def operators(ne, h, D, rho, fixed, f, q=GAMMA, solve=None):
    """dict with the element constants, the multipliers, the free dofs, K (csr, reduced), u, K_G (csr, reduced); ``solve(K, b)``
    replaces SuperLU for u and for the adjoint (stress_cpu.solve_cg with a tolerance: what an iterative solver leaves)"""
    K0 = hc.element_constants(D, h)[0]
    T = geometric_element_matrices(D, h)
    E, dE = hc.moduli(rho, E0, EMIN, GAMMA)
    mG, dmG = geometric_multiplier(rho, q)
    fixed = np.asarray(fixed, dtype=bool).reshape(-1)
    free = np.flatnonzero(~fixed)
    Kfull = sc.assemble(ne, K0, E, fixed)
    lu = spla.splu(Kfull.tocsc())
    solver = lu.solve if solve is None else (lambda b: solve(Kfull, b))
    u = solver(np.where(fixed, 0.0, np.asarray(f, dtype=np.float64).reshape(-1)))
    KG = assemble_geometric(ne, T, mG, u)[free][:, free].tocsr()
    return dict(ne=ne, K0=K0, T=T, dE=dE, mG=mG, dmG=dmG, fixed=fixed, free=free, Kfull=Kfull, lu=lu, solver=solver, K=Kfull[free][:, free].tocsr(),
                KG=KG, u=u, ndof=len(fixed))


def dense_modes(op, k):
    """(nu [k] ascending, Phi [ndof, k] K-orthonormal on the full grid, the whole spectrum)"""
    nu, V = scipy.linalg.eigh(op["KG"].toarray(), op["K"].toarray())
    Phi = np.zeros((op["ndof"], k))
    Phi[op["free"]] = V[:, :k]
    return nu[:k], Phi, nu


def lobpcg_modes(op, k, tol, X0, guard=2, max_iter=200):
    """modal_cpu.lobpcg on (K_G, K) with K^-1 as the preconditioner: (nu, Phi on the full grid, iterations, residuals)"""
    lu = spla.splu(op["K"].tocsc())
    nu, X, its, res = mc.lobpcg(op["KG"], op["K"], k, tol, X0, guard=guard, max_iter=max_iter, T=lu.solve)
    Phi = np.zeros((op["ndof"], k))
    Phi[op["free"]] = X
    return nu, Phi, its, res


def start_block(op, columns, seed=7):
    return np.random.default_rng(seed).standard_normal((len(op["free"]), columns))


def objective(nu, P=P_NORM):
    mu = -np.asarray(nu)
    top = mu.max()
    return float(top * np.sum((mu / top) ** P) ** (1.0 / P))


def mode_weights(nu, P=P_NORM):
    return (-np.asarray(nu) / objective(nu, P)) ** (P - 1.0)


def adjoint_load(op, nu, Phi, P=P_NORM):
    return kernel_adjoint_load(op["ne"], op["T"], op["mG"], Phi.T, -mode_weights(nu, P), op["fixed"])


def gradient(op, nu, Phi, P=P_NORM):
    """(dJ/drho [elements], a, v)"""
    w = mode_weights(nu, P)
    a = adjoint_load(op, nu, Phi, P)
    v = op["solver"](a)
    return kernel_gradient(op["ne"], op["T"], op["K0"], op["dmG"], op["dE"], op["u"], v, Phi.T, -w, w * nu), a, v


def evaluate(name_or_case, rho=None, k=NUM_MODES, P=P_NORM, want_gradient=True, solve=None):
    """the dense chain of a case (optionally at other densities): dict with op, nu, Phi, spectrum, J and the gradient"""
    ne, h, D, rho0, fixed, f = case(name_or_case) if isinstance(name_or_case, str) else name_or_case
    op = operators(ne, h, D, rho0 if rho is None else rho, fixed, f, solve=solve)
    nu, Phi, spectrum = dense_modes(op, k)
    out = dict(op=op, nu=nu, Phi=Phi, spectrum=spectrum, J=objective(nu, P))
    if want_gradient:
        out["gradient"], out["a"], out["v"] = gradient(op, nu, Phi, P)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the dense solution of a case, computed once and shared (tests leave it unchanged)"""
    return evaluate(name)


def euler_column(ne, h):
    """(lambda_1, the closed form pi^2 E b^3 / 12 / (4 L^2)) of a uniform solid clamped-free column, nu = 0, unit end load"""
    fixed = sc.cantilever(ne)[0]
    op = operators(ne, (h, h), hc.isotropic_D(1.0, 0.0, 2), np.ones(int(np.prod(ne))), fixed, end_load(ne, True))
    nu = scipy.linalg.eigh(op["KG"].toarray(), op["K"].toarray(), eigvals_only=True, subset_by_index=[0, 0])
    L, b = ne[0] * h, ne[1] * h
    return -1.0 / nu[0], np.pi ** 2 * b ** 3 / 12.0 / (4.0 * L ** 2)
