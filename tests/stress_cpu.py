"""numpy / scipy fp64 restatement of the element stresses, the p-norm stress measure and its adjoint gradient, for the tests.  Nothing
here comes from the library: Bbar is the mean of the strain-displacement matrix over the element by 2-point Gauss quadrature of the
shape functions' gradients, K0 is homogenization_cpu's quadrature, the stiffness matrix is assembled on the full node grid and
solved by SuperLU (two column orderings) or by a Jacobi-preconditioned conjugate gradient to a given relative residual.

Conventions: nodes and elements with the last axis fastest, element e owns the nodes (e_d + mu_d), local node index with axis 0 as
the most significant bit, dof = N * node + component.  Flattened order xx yy xy / xx yy zz yz xz xy, TENSOR components: D carries no
factor 2, so sigma = D (mult * eps) with mult = 2 on the shear entries.

    eps_e = Bbar u_e,  sigma_e = m_e D (mult * eps_e),  m = E_min + rho^q (E_0 - E_min),  vm_e = von Mises,  J = (sum vm^P)^(1/P)
    dJ/du (fixed rho) = sum_e w_e m_e Bbar^T (mult * D^T dv_e),  w_e = (vm_e / J)^(P-1),  dv_e = d vm / d sigma (flattened)
    K lambda = dJ/du (zero at the fixed dofs),
    dJ/drho_e = w_e q rho^(q-1) (E_0 - E_min) vm_e / m_e - gamma rho^(gamma-1) (E_0 - E_min) lambda_e^T K0 u_e
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import homogenization_cpu as hc

PAIRS = hc.PAIRS


def mult(N):
    return np.array([1.0 if i == j else 2.0 for i, j in PAIRS[N]])


def strain_matrix(h, x):
    """B(x) [S, ke]: the tensor components of sym(grad u) at the point x of the unit cube scaled by h"""
    N = len(h)
    npe = 2 ** N
    B = np.zeros((len(PAIRS[N]), N * npe))
    for n, l in enumerate(np.ndindex(*([2] * N))):
        grad = np.empty(N)
        for d in range(N):
            v = 1.0
            for e in range(N):
                v *= ((1.0 if l[e] else -1.0) / h[e]) if e == d else (x[e] if l[e] else 1.0 - x[e])
            grad[d] = v
        for r, (i, j) in enumerate(PAIRS[N]):
            if i == j:
                B[r, N * n + i] = grad[i]
            else:
                B[r, N * n + i] += 0.5 * grad[j]
                B[r, N * n + j] += 0.5 * grad[i]
    return B


def bbar(h):
    """the mean of B over the element, by 2-point Gauss quadrature per axis (exact: B is multilinear)"""
    N = len(h)
    gauss = (0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0))
    out = 0.0
    for q in np.ndindex(*([2] * N)):
        out = out + 0.5 ** N * strain_matrix(h, [gauss[i] for i in q])
    return out


def element_dofs(ne):
    """[numElements, ke] dof indices on the full (ne + 1) node grid"""
    ne = [int(n) for n in ne]
    N = len(ne)
    nn = [n + 1 for n in ne]
    e = np.stack(np.meshgrid(*[np.arange(n) for n in ne], indexing="ij"), -1).reshape(-1, N)
    nodes = np.stack([np.ravel_multi_index(tuple(e[:, d] + mu[d] for d in range(N)), nn) for mu in np.ndindex(*([2] * N))], axis=1)
    return (N * nodes[:, :, None] + np.arange(N)[None, None, :]).reshape(len(e), -1)


def num_nodes(ne):
    return int(np.prod([int(n) + 1 for n in ne]))


def von_mises(s):
    s = np.asarray(s, dtype=np.float64)
    if s.shape[-1] == 3:
        return np.sqrt(s[..., 0] ** 2 - s[..., 0] * s[..., 1] + s[..., 1] ** 2 + 3.0 * s[..., 2] ** 2)
    return np.sqrt(0.5 * ((s[..., 0] - s[..., 1]) ** 2 + (s[..., 1] - s[..., 2]) ** 2 + (s[..., 2] - s[..., 0]) ** 2)
                   + 3.0 * (s[..., 3] ** 2 + s[..., 4] ** 2 + s[..., 5] ** 2))


def von_mises_derivative(s, vm):
    """d vm / d s_q for the flattened components (a shear component stands for both of its tensor entries); 0 where vm = 0"""
    s = np.asarray(s, dtype=np.float64)
    r = np.where(vm > 0.0, 0.5 / np.where(vm > 0.0, vm, 1.0), 0.0)[..., None]
    if s.shape[-1] == 3:
        d = np.stack([2.0 * s[..., 0] - s[..., 1], 2.0 * s[..., 1] - s[..., 0], 6.0 * s[..., 2]], axis=-1)
    else:
        d = np.stack([2.0 * s[..., 0] - s[..., 1] - s[..., 2], 2.0 * s[..., 1] - s[..., 2] - s[..., 0],
                      2.0 * s[..., 2] - s[..., 0] - s[..., 1], 6.0 * s[..., 3], 6.0 * s[..., 4], 6.0 * s[..., 5]], axis=-1)
    return d * r


def multiplier(rho, E0, Emin, q):
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    return Emin + rho ** q * (E0 - Emin), q * rho ** (q - 1.0) * (E0 - Emin)


def fields(ne, h, D, m, u):
    """(strain [ne, S], stress [ne, S], vm [ne]) of the displacement u [numNodes * N]"""
    N = len(ne)
    ue = np.asarray(u, dtype=np.float64).reshape(-1)[element_dofs(ne)]
    eps = ue @ bbar(h).T
    sig = np.asarray(m)[:, None] * ((eps * mult(N)) @ np.asarray(D).T)
    return eps, sig, von_mises(sig)


def pnorm(vm, P):
    """(sum vm^P)^(1/P) as vmax (sum (vm / vmax)^P)^(1/P); 0 for the zero field"""
    vm = np.asarray(vm, dtype=np.float64)
    vmax = float(vm.max())
    if vmax == 0.0:
        return 0.0
    return vmax * float(np.sum((vm / vmax) ** P)) ** (1.0 / P)


def weights(vm, J, P):
    return (vm / J) ** (P - 1.0) if J > 0.0 else np.zeros_like(vm)


def adjoint_load(ne, h, D, m, u, P, fixed=None):
    """dJ/du at fixed m, [numNodes * N], zero at the dofs `fixed` (bool [numNodes * N])"""
    N = len(ne)
    _, sig, vm = fields(ne, h, D, m, u)
    J = pnorm(vm, P)
    dv = von_mises_derivative(sig, vm)
    per_element = (weights(vm, J, P) * np.asarray(m))[:, None] * (((dv @ np.asarray(D)) * mult(N)) @ bbar(h))
    a = np.zeros(num_nodes(ne) * N)
    np.add.at(a, element_dofs(ne).reshape(-1), per_element.reshape(-1))
    if fixed is not None:
        a[np.asarray(fixed).reshape(-1)] = 0.0
    return a


def assemble(ne, K0, E, fixed):
    """the stiffness matrix (csr) with the rows and columns of the fixed dofs replaced by the identity"""
    dofs = element_dofs(ne)
    ke = dofs.shape[1]
    nd = num_nodes(ne) * len(ne)
    rows, cols = np.repeat(dofs, ke, axis=1).reshape(-1), np.tile(dofs, (1, ke)).reshape(-1)
    K = sp.coo_matrix(((np.asarray(E)[:, None, None] * K0[None]).reshape(-1), (rows, cols)), shape=(nd, nd)).tocsr()
    keep = 1.0 - np.asarray(fixed, dtype=np.float64).reshape(-1)
    P = sp.diags(keep)
    return (P @ K @ P + sp.diags(1.0 - keep)).tocsr()


def solve_direct(K, b, ordering="COLAMD"):
    return spla.splu(K.tocsc(), permc_spec=ordering).solve(np.asarray(b, dtype=np.float64))


def solve_cg(K, b, tol, max_iter=200000):
    """Jacobi-preconditioned conjugate gradient from x = 0 to |r| / |b| <= tol"""
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros_like(b)
    bb = float(b @ b)
    if bb == 0.0:
        return x
    dinv = 1.0 / K.diagonal()
    r = b.copy()
    z = dinv * r
    p = z.copy()
    rz = float(r @ z)
    for _ in range(max_iter):
        Ap = K @ p
        alpha = rz / float(p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        if float(r @ r) <= tol * tol * bb:
            return x
        z = dinv * r
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    raise RuntimeError("solve_cg: no convergence")


def evaluate(ne, h, D, rho, f, fixed, E0=1.0, Emin=1e-3, gamma=3.0, q=0.5, P=8.0, solve=solve_direct, want_gradient=True):
    """the whole chain for the densities rho: dict with u, vm, J, a, lam, gradient, compliance (1/2 f.u) and its gradient"""
    N = len(ne)
    K0 = hc.element_constants(D, h)[0]
    E, dE = hc.moduli(rho, E0, Emin, gamma)
    m, dm = multiplier(rho, E0, Emin, q)
    fixed = np.asarray(fixed, dtype=bool).reshape(-1)
    K = assemble(ne, K0, E, fixed)
    fz = np.where(fixed, 0.0, np.asarray(f, dtype=np.float64).reshape(-1))
    u = solve(K, fz)
    eps, sig, vm = fields(ne, h, D, m, u)
    J = pnorm(vm, P)
    out = dict(K0=K0, K=K, m=m, u=u, strain=eps, stress=sig, vm=vm, J=J, compliance=0.5 * float(fz @ u))
    if want_gradient:
        dofs = element_dofs(ne)
        a = adjoint_load(ne, h, D, m, u, P, fixed)
        lam = solve(K, a)
        vm0 = von_mises((eps * mult(N)) @ np.asarray(D).T)                       # vm / m without the division
        out.update(a=a, lam=lam, gradient=weights(vm, J, P) * dm * vm0 - dE * np.einsum("ek,kl,el->e", lam[dofs], K0, u[dofs]),
                   compliance_gradient=-0.5 * dE * np.einsum("ek,kl,el->e", u[dofs], K0, u[dofs]))
    return out


def cantilever(ne):
    """(fixed [numNodes, N] bool, f [numNodes, N]): the x = 0 face clamped, a unit point load along -y (the last axis in 2-D, the
    middle one in 3-D) at the middle of the opposite face"""
    N = len(ne)
    nn = [int(n) + 1 for n in ne]
    fixed = np.zeros(nn + [N], dtype=bool)
    fixed[0] = True
    f = np.zeros(nn + [N])
    f[(nn[0] - 1,) + tuple(n // 2 for n in nn[1:]) + (1,)] = -1.0
    return fixed.reshape(-1, N), f.reshape(-1, N)


def isotropic_D(E, nu, N):
    return hc.isotropic_D(E, nu, N)


# the two design problems of the objective and autograd tests: elements, edge lengths, (E, nu), density seed
CASES = {"16x12": ((16, 12), (0.125, 0.125), (1.0, 0.3), 91), "8x8x6": ((8, 8, 6), (0.25, 0.25, 0.25), (1.0, 0.3), 92)}


def case(name):
    ne, h, (E, nu), seed = CASES[name]
    rho = np.random.default_rng(seed).uniform(0.2, 1.0, size=int(np.prod(ne)))
    fixed, f = cantilever(ne)
    return ne, h, isotropic_D(E, nu, len(ne)), rho, f, fixed
