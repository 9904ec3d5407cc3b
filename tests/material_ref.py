"""TEST INFRASTRUCTURE ONLY: the reference element stiffness matrix of a box voxel for ANY elasticity tensor, by Gauss quadrature in
numpy with its own loops (no code shared with ndr_amd/csrc or with oracle/), plus the K0 structure the tuned kernels assume.

    K0[(n,a),(m,b)] = vol * sum_pq C_apbq * int d_p N_n d_q N_m          (TPS.hh:127-140 with a general C)

``inject`` puts such a K0 into ``oracle.generic_oracle.GenericSim``: its assembled K, its sweeps and the P^T K P levels of
``GenericMG`` all read the ``K0`` attribute, so the generic oracle becomes the oracle of an orthotropic / anisotropic material
without a change to any oracle file.

Conventions: local nodes row-major with the last axis fastest, dof = N * node + component; the flattened tensor D is n x n in the
order xx yy zz yz xz xy (2-D: xx yy xy) and holds tensor components (shear rows carry no factor 2).
"""
import json
import os

import numpy as np

MATERIALS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "materials")
ORTHO_3D, ORTHO_2D = os.path.join(MATERIALS, "orthotropic_3d.material"), os.path.join(MATERIALS, "orthotropic_2d.material")
ANISO_3D, ANISO_2D = os.path.join(MATERIALS, "anisotropic_3d.material"), os.path.join(MATERIALS, "anisotropic_2d.material")
ASYMMETRIC, INCONSISTENT = os.path.join(MATERIALS, "asymmetric.material"), os.path.join(MATERIALS, "orthotropic_inconsistent.material")

_INDEX_PAIRS = {2: [(0, 0), (1, 1), (0, 1)], 3: [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]}


def full_tensor(D):
    """C[a, p, b, q] from the flattened D"""
    D = np.asarray(D, dtype=np.float64)
    N = {3: 2, 6: 3}[D.shape[0]]
    C = np.zeros((N, N, N, N))
    for i, (a, p) in enumerate(_INDEX_PAIRS[N]):
        for j, (b, q) in enumerate(_INDEX_PAIRS[N]):
            C[a, p, b, q] = C[p, a, b, q] = C[a, p, q, b] = C[p, a, q, b] = D[i, j]
    return C


def compliance_matrix_inverse(young, poisson, shear):
    """D of an orthotropic material file, computed here independently of ndr_amd.materials: the inverse of the matrix with
    1/E_i on the diagonal, -nu_ji/E_j above it and 1/mu on the shear diagonal.  ``poisson`` in the file's order (3-D: yz zy zx xz xy
    yx; 2-D: xy yx), ``shear`` 3-D: yz zx xy"""
    if len(young) == 2:
        (Ex, Ey), (_, nu_yx) = young, poisson
        S = np.array([[1 / Ex, -nu_yx / Ey, 0], [-nu_yx / Ey, 1 / Ey, 0], [0, 0, 1 / shear[0]]])
    else:
        Ex, Ey, Ez = young
        _, nu_zy, nu_zx, _, _, nu_yx = poisson
        S = np.zeros((6, 6))
        S[0, 0], S[1, 1], S[2, 2] = 1 / Ex, 1 / Ey, 1 / Ez
        S[0, 1] = S[1, 0] = -nu_yx / Ey
        S[0, 2] = S[2, 0] = -nu_zx / Ez
        S[1, 2] = S[2, 1] = -nu_zy / Ez
        S[3, 3], S[4, 4], S[5, 5] = 1 / shear[0], 1 / shear[1], 1 / shear[2]
    return np.linalg.inv(S)


def material_file_D(path):
    """the flattened tensor a material file of this suite stands for, read without the library's parser"""
    with open(path) as fh:
        m = json.load(fh)
    if "material_matrix" in m:
        return np.array(m["material_matrix"], dtype=np.float64)
    return compliance_matrix_inverse(m["young"], m["poisson"], m["shear"])


def _gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def _lagrange(p, a, x):
    nodes = [j / p for j in range(p + 1)]
    v = 1.0
    for j in range(p + 1):
        if j != a:
            v *= (x - nodes[j]) / (nodes[a] - nodes[j])
    return v


def _dlagrange(p, a, x):
    nodes = [j / p for j in range(p + 1)]
    s = 0.0
    for k in range(p + 1):
        if k == a:
            continue
        t = 1.0 / (nodes[a] - nodes[k])
        for j in range(p + 1):
            if j != a and j != k:
                t *= (x - nodes[j]) / (nodes[a] - nodes[j])
        s += t
    return s


def reference_stiffness(D, h, p=1):
    """K0 for the flattened tensor D on a voxel of edge lengths h, degree p: (p + 1)-point Gauss rule per axis (exact)"""
    h = [float(v) for v in h]
    N = len(h)
    C = full_tensor(D)
    xg, wg = _gauss(p + 1)
    loc = list(np.ndindex(*([p + 1] * N)))
    npe = len(loc)
    K = np.zeros((N * npe, N * npe))
    for q in np.ndindex(*([p + 1] * N)):
        w = float(np.prod(h))
        for axis in range(N):
            w *= wg[q[axis]]
        grad = np.zeros((npe, N))
        for n, l in enumerate(loc):
            for d in range(N):
                v = 1.0
                for e in range(N):
                    v *= _dlagrange(p, l[e], xg[q[e]]) if e == d else _lagrange(p, l[e], xg[q[e]])
                grad[n, d] = v / h[d]
        for n in range(npe):
            for m in range(npe):
                for a in range(N):
                    for b in range(N):
                        s = 0.0
                        for pp in range(N):
                            for qq in range(N):
                                s += C[a, pp, b, qq] * grad[n, pp] * grad[m, qq]
                        K[N * n + a, N * m + b] += w * s
    return K


def inject(generic_sim, D):
    """make ``generic_sim`` (oracle.generic_oracle.GenericSim) the oracle of the material D"""
    generic_sim.K0 = reference_stiffness(D, generic_sim.h, generic_sim.p)
    generic_sim.lam = generic_sim.mu = None            # nothing may fall back to the Lame pair
    return generic_sim


def stress_of(D, eps):
    """sigma = C : eps"""
    return np.einsum("apbq,bq->ap", full_tensor(D), np.asarray(eps, dtype=np.float64))


def constant_strain_load(D, eps, h, ne, rho, p=1):
    """TPS::constantStrainLoad for a general tensor: node j of element e receives rho_e * vol * (C : eps) . int grad(phi_j), the
    integral by the same Gauss rule as the stiffness (loops of its own)"""
    h = [float(v) for v in h]
    N = len(h)
    sigma = stress_of(D, eps)
    xg, wg = _gauss(p + 1)
    loc = list(np.ndindex(*([p + 1] * N)))
    g = np.zeros((len(loc), N))
    for q in np.ndindex(*([p + 1] * N)):
        w = float(np.prod([wg[i] for i in q]))
        for n, l in enumerate(loc):
            for d in range(N):
                v = 1.0
                for e in range(N):
                    v *= _dlagrange(p, l[e], xg[q[e]]) if e == d else _lagrange(p, l[e], xg[q[e]])
                g[n, d] += w * v / h[d]
    vol = float(np.prod(h))
    nn = tuple(p * int(n) + 1 for n in ne)
    F = np.zeros(nn + (N,))
    rho = np.asarray(rho, dtype=np.float64).reshape(tuple(int(n) for n in ne))
    for n, l in enumerate(loc):
        load = vol * (sigma @ g[n])
        sl = tuple(slice(l[d], l[d] + p * int(ne[d]), p) for d in range(N))
        F[sl] += rho[..., None] * load
    return F.reshape(-1, N)


# ----------------------------------------------------------------------------------------------
# the structure of K0 that the tuned trilinear kernels rely on (what vfem_sim::update_k0 verifies numerically)
# ----------------------------------------------------------------------------------------------

def mode_space_nonzeros(K0, tol=1e-13):
    """entries of T K0 T^T / 64 above tol * max, T = H (x) H (x) H (x) I_3 with H = [[1, 1], [-1, 1]]"""
    H = np.array([[1.0, 1.0], [-1.0, 1.0]])
    T = np.kron(np.kron(np.kron(H, H), H), np.eye(3))
    Dm = T @ K0 @ T.T / 64.0
    return int((np.abs(Dm) > tol * np.abs(Dm).max()).sum())


def distinct_magnitudes(K0, tol=1e-12):
    """number of distinct |K0| values (relative tolerance), zeros not counted"""
    v = np.sort(np.abs(K0).reshape(-1))
    v = v[v > tol * v[-1]]
    return int(1 + (np.diff(v) > tol * v[-1]).sum())


def mirror_residual(K0):
    """max over the reflections f of |K0[(n,a),(m,b)] - s_a(f) s_b(f) K0[(n^f,a),(m^f,b)]| / max|K0|"""
    K = K0.reshape(8, 3, 8, 3)
    worst = 0.0
    for f in range(1, 8):
        s = np.array([-1.0 if (f >> (2 - a)) & 1 else 1.0 for a in range(3)])
        perm = np.arange(8) ^ f
        Kf = K[perm][:, :, perm] * s[None, :, None, None] * s[None, None, None, :]
        worst = max(worst, float(np.abs(K - Kf).max()))
    return worst / float(np.abs(K0).max())
