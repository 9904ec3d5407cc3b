"""Dense numpy restatement of transient heat conduction on a degree-1 voxel grid, written from the formulas on top of
thermal_cpu.py and not from the kernels: the capacity matrix, the two-term operator, the theta-scheme march, its discrete adjoint,
the time-accumulated gradient and the two objectives, with element-wise versions of the apply, diagonal and gradient sums that also
run in np.longdouble (the reference of the kernel tests).

    c_e = c_min + rho_e^q (1 - c_min),   C = sum_e c_e Mc0,   Mc0[a][b] = m[popcount(a xor b)],
    m[d] = capacity ((1 - l) vol 2^(N - d) / 6^N + l [d = 0] vol / 2^N)                       (l: the lumping, 0 consistent, 1 lumped)
    A(Ka, Mb) = P (sum_e kappa_e Ka + sum_e c_e Mb) P + iota (I - P)
    T^0 = P T_init,   A T^n = B T^(n-1) + (theta s_n + (1 - theta) s_(n-1)) P Q,   A = A(theta Kc0, Mc0 / dt),  B = A(-(1 - theta) Kc0, Mc0 / dt), iota = 0
    A lam^S = P dj_S/dT,   A lam^n = P (dj_n/dT + B lam^(n+1))
    dJ/drho_e = -sum_n (c'_e / dt lam_e^n . Mc0 (T_e^n - T_e^(n-1)) + kappa'_e lam_e^n . Kc0 (theta T_e^n + (1 - theta) T_e^(n-1)))
"""
import functools

import numpy as np

import thermal_cpu as tc


def capacity_entries(h, capacity=1.0, lumping=0.0, dtype=np.float64):
    """m[d], d = 0 .. N"""
    h = np.asarray(h, dtype=dtype)
    N = h.size
    vol = dtype(np.prod(h))
    lump = dtype(lumping)
    m = np.array([(1 - lump) * vol * dtype(2 ** (N - d)) / dtype(6 ** N) for d in range(N + 1)], dtype=dtype)
    m[0] += lump * vol / dtype(2 ** N)
    return dtype(capacity) * m


def differing_axes(N):
    """[2^N, 2^N]: popcount(a xor b)"""
    bits = tc.node_bits(N)
    return (bits[:, None, :] != bits[None, :, :]).sum(axis=2)


def capacity_matrix(m):
    m = np.asarray(m)
    return m[differing_axes(m.size - 1)]


def cap(rho, q=1.0, c_min=1e-3):
    return c_min + rho ** q * (1.0 - c_min)


def dcap(rho, q=1.0, c_min=1e-3):
    return q * rho ** (q - 1.0) * (1.0 - c_min)


def assemble(ne, Ka, Mb, kap, cp, fixed=None, identity=1, dtype=np.float64):
    """A(Ka, Mb), dense"""
    A = tc.assemble(ne, Ka, kap, None, dtype) + tc.assemble(ne, Mb, cp, None, dtype)
    if fixed is not None and fixed.any():
        A[fixed, :] = 0
        A[:, fixed] = 0
        A[fixed, fixed] = identity
    return A


def operators(ne, Kc0, m, kap, cp, fixed, dt, theta):
    """(A, B) of a step"""
    Mb = capacity_matrix(np.asarray(m) / dt)
    return assemble(ne, theta * Kc0, Mb, kap, cp, fixed, 1), assemble(ne, -(1.0 - theta) * Kc0, Mb, kap, cp, fixed, 0)


def _project(v, fixed):
    return v if fixed is None else np.where(fixed, 0.0, v)


def march(A, B, Q, fixed, steps, theta, T0=None, s=None, solve=np.linalg.solve):
    """T [steps + 1, nodes]"""
    n = A.shape[0]
    s = np.ones(steps + 1) if s is None else np.asarray(s, dtype=np.float64)
    T = np.zeros((steps + 1, n))
    if T0 is not None:
        T[0] = _project(T0, fixed)
    PQ = _project(Q, fixed)
    for k in range(1, steps + 1):
        T[k] = solve(A, B @ T[k - 1] + (theta * s[k] + (1.0 - theta) * s[k - 1]) * PQ)
    return T


def adjoint(A, B, dJdT, fixed, solve=np.linalg.solve):
    """Lam [steps + 1, nodes] (row 0 zero) of J = sum_n j_n(T^n), dJdT [steps + 1, nodes] with row 0 ignored"""
    S = dJdT.shape[0] - 1
    Lam = np.zeros_like(dJdT)
    Lam[S] = solve(A, _project(dJdT[S], fixed))
    for k in range(S - 1, 0, -1):
        Lam[k] = solve(A, _project(dJdT[k] + B @ Lam[k + 1], fixed))
    return Lam


# ---- the kernels' sums, element by element, in float64 or np.longdouble ----

def apply(ne, Ka, mb, kap, cp, fixed, X, b=None, identity=1, dtype=np.float64):
    """Y_c = A(Ka, M(mb)) X_c + P b_c for the block X [columns, nodes]"""
    en = tc.element_nodes(ne)
    Ka, kap, cp, X = Ka.astype(dtype), kap.astype(dtype), cp.astype(dtype), np.atleast_2d(X).astype(dtype)
    Mb = capacity_matrix(np.asarray(mb).astype(dtype))
    Y = np.zeros_like(X)
    for c in range(X.shape[0]):
        xe = tc._free(X[c], fixed)[en]
        np.add.at(Y[c], en, kap[:, None] * np.einsum("ab,eb->ea", Ka, xe) + cp[:, None] * np.einsum("ab,eb->ea", Mb, xe))
        if b is not None:
            Y[c] += np.atleast_2d(b)[c].astype(dtype)
        if fixed is not None:
            Y[c] = np.where(fixed, dtype(identity) * X[c], Y[c])
    return Y


def diagonal(ne, Ka, mb, kap, cp, fixed, dtype=np.float64):
    en = tc.element_nodes(ne)
    d = np.zeros(tc.num_nodes(ne), dtype=dtype)
    np.add.at(d, en, kap.astype(dtype)[:, None] * np.diag(Ka).astype(dtype)[None, :] + cp.astype(dtype)[:, None] * dtype(mb[0]))
    return d if fixed is None else np.where(fixed, dtype(1), d)


def gradient(ne, Kc0, m, dkap, dcp, dt, theta, T, Lam, dtype=np.float64):
    """the time-accumulated gradient, [elements]"""
    en = tc.element_nodes(ne)
    Kc0, M = Kc0.astype(dtype), capacity_matrix(np.asarray(m).astype(dtype))
    dkap, dcp, T, Lam = np.asarray(dkap).astype(dtype), np.asarray(dcp).astype(dtype), np.asarray(T).astype(dtype), np.asarray(Lam).astype(dtype)
    dt, theta = dtype(dt), dtype(theta)
    sc = np.zeros(en.shape[0], dtype=dtype)
    sk = np.zeros(en.shape[0], dtype=dtype)
    for k in range(1, T.shape[0]):
        now, before, lam = T[k][en], T[k - 1][en], Lam[k][en]
        sc += np.einsum("ea,ab,eb->e", lam, M, now - before)
        sk += np.einsum("ea,ab,eb->e", lam, Kc0, theta * now + (1 - theta) * before)
    return -(dcp / dt * sc + dkap * sk)


# ---- problems and objectives ----

class Problem:
    """one design of a transient problem, dense: the operators of a step are built once"""

    def __init__(self, ne, h, k, rho, fixed, Q, steps, dt, theta=1.0, T0=None, s=None, capacity=1.0, q=1.0, c_min=1e-3, lumping=0.0,
                 p=3.0, k_min=1e-3):
        self.ne, self.h, self.fixed, self.steps, self.dt, self.theta = tuple(ne), tuple(h), fixed, steps, dt, theta
        self.s = np.ones(steps + 1) if s is None else np.asarray(s, dtype=np.float64)
        self.Kc0 = tc.conductivity_matrix(k, h)
        self.m = capacity_entries(h, capacity, lumping)
        self.kap, self.dkap = tc.kappa(rho, p, k_min), tc.dkappa(rho, p, k_min)
        self.cp, self.dcp = cap(rho, q, c_min), dcap(rho, q, c_min)
        self.A, self.B = operators(ne, self.Kc0, self.m, self.kap, self.cp, fixed, dt, theta)
        self.Q = _project(Q, fixed)
        self.T = march(self.A, self.B, self.Q, fixed, steps, theta, T0, self.s)

    def C(self):
        return assemble(self.ne, 0.0 * self.Kc0, capacity_matrix(self.m), self.kap, self.cp, None)

    def gradient_of(self, dJdT):
        Lam = adjoint(self.A, self.B, dJdT, self.fixed)
        return gradient(self.ne, self.Kc0, self.m, self.dkap, self.dcp, self.dt, self.theta, self.T, Lam), Lam

    def compliance(self):
        """(J, dJ/drho, Lam) of J = dt sum_{n >= 1} s_n Q . T^n"""
        J = self.dt * float(sum(self.s[k] * (self.Q @ self.T[k]) for k in range(1, self.steps + 1)))
        dJdT = self.dt * self.s[:, None] * self.Q[None, :]
        return (J,) + self.gradient_of(dJdT)

    def pnorm(self, P):
        """(J, dJ/drho, Lam, peak, its step) of J = (sum_{n >= 1} sum_i |T_i^n|^P)^(1/P), evaluated scaled by the peak"""
        T = self.T[1:]
        top = np.abs(T).max()
        J = top * np.sum((np.abs(T) / top) ** P) ** (1.0 / P)
        dJdT = np.zeros_like(self.T)
        dJdT[1:] = (np.abs(T) / J) ** (P - 1.0) * np.sign(T)
        g, Lam = self.gradient_of(dJdT)
        return float(J), g, Lam, float(top), 1 + int(np.unravel_index(np.abs(T).argmax(), T.shape)[0])

    def weighted(self, W):
        """(J, dJ/drho) of J = sum_{n >= 1} W_n . T^n: the linear functional of the finite-difference test"""
        J = float(np.sum(W[1:] * self.T[1:]))
        return J, self.gradient_of(W)[0]


def decay_factor(k, h, dt, theta, lumping):
    """what one step multiplies the mode sin(pi x) of a unit bar of elements of length h by"""
    mu = k * 2.0 * (1.0 - np.cos(np.pi * h)) / h / (h * ((1.0 - lumping) * (2.0 + np.cos(np.pi * h)) / 3.0 + lumping))
    return (1.0 - (1.0 - theta) * dt * mu) / (1.0 + theta * dt * mu)


# ---- fixtures shared with the GPU tests ----

def decay_case(theta, lumping, steps=3, dt=0.01):
    """the grid (16, 1) of a unit square's strip, both x faces fixed, full density, no source, T0 = sin(pi x): returns the problem and
    the exact T^steps"""
    ne, h = (16, 1), (1.0 / 16, 1.0 / 16)
    fixed = tc.face_mask(ne, 0, 0) | tc.face_mask(ne, 0, 1)
    x = tc.node_coordinates(ne, h)[:, 0]
    T0 = np.sin(np.pi * x)
    pr = Problem(ne, h, 1.0, np.ones(16), fixed, np.zeros(34), steps, dt, theta, T0, lumping=lumping)
    return pr, decay_factor(1.0, h[0], dt, theta, lumping) ** steps * np.where(fixed, 0.0, T0)


DECAY_CASES = [(1.0, 0.0), (0.5, 0.0), (1.0, 1.0)]
# the restatement's own error on the decay of the mode, relative to the largest entry, and on the energy balance, relative to 1^T Q
# (tests/test_transient_cpu.py measures and pins them within a factor of three); the device bounds are ten times these, or nodes x 2^-52
# where the figure is no more than one rounding (thermal_cpu.analytic_bound)
DECAY_MEASURED = {(1.0, 0.0): 3.7e-15, (0.5, 0.0): 3.3e-15, (1.0, 1.0): 3.7e-15}
ENERGY_SHAPES = [(16, 6), (6, 4, 3)]
ENERGY_MEASURED = {(16, 6): 6.1e-16, (6, 4, 3): 3.5e-16}                  # the larger of theta = 1 and theta = 0.5


@functools.lru_cache(maxsize=None)
def energy_case(ne, theta):
    """no sink: random densities, a volumetric source and a random start"""
    N = len(ne)
    rng = np.random.default_rng(1900 + tc.num_elements(ne))
    h = tc.EDGES[N]
    rho = rng.uniform(0.2, 1.0, size=tc.num_elements(ne))
    q = rng.uniform(0.5, 1.5, size=tc.num_elements(ne))
    fixed = np.zeros(tc.num_nodes(ne), dtype=bool)
    T0 = rng.uniform(0.0, 1.0, size=tc.num_nodes(ne))
    return dict(ne=ne, h=h, k=tc.K_ANISO[N], rho=rho, q=q, fixed=fixed, T0=T0, steps=4, dt=0.05, theta=theta)


def energy_error(ne, C, T, Q, dt):
    """the largest |1^T C (T^n - T^(n-1)) / dt - 1^T Q| over the steps, relative to |1^T Q|"""
    one = np.ones(C.shape[0])
    return max(abs(one @ (C @ (T[k] - T[k - 1])) / dt - one @ Q) for k in range(1, T.shape[0])) / abs(one @ Q)


@functools.lru_cache(maxsize=None)
def chain_fixture(ne, theta):
    """the direct-chain problem: thermal_cpu.direct_fixture with a start, source scales, six steps and a half-lumped capacity"""
    f = dict(tc.direct_fixture(ne))
    rng = np.random.default_rng(2000 + tc.num_elements(ne))
    f.update(T0=rng.uniform(0.0, 1.0, size=tc.num_nodes(ne)), s=rng.uniform(0.5, 1.5, size=7), steps=6, dt=0.05, theta=theta,
             capacity=1.7, q=2.0, c_min=1e-2, lumping=0.5)
    return f


def chain_problem(f, rho=None):
    rho = f["rho"] if rho is None else rho
    Q = tc.load(f["ne"], f["h"], f["fixed"], f.get("nodal"), f.get("volumetric"))
    return Problem(f["ne"], f["h"], f["k"], rho, f["fixed"], Q, f["steps"], f["dt"], f["theta"], f.get("T0"), f.get("s"),
                   f.get("capacity", 1.0), f.get("q", 1.0), f.get("c_min", 1e-3), f.get("lumping", 0.0))


# ---- the multigrid hierarchy of a step's operator ----

import thermal_mg_cpu as mg             # noqa: E402


class Hierarchy(mg.Hierarchy):
    """thermal_mg_cpu.Hierarchy with the two-term level 0: A'_0 = F_0 (sum_e kappa_e Ka + sum_e c_e M(mb)) F_0; the coarsening, the
    transfers, the Galerkin chain, the sweeps, the V-cycle and the PCG are that class's"""

    def __init__(self, ne, Ka, mb, kap, cp, fixed, max_coarsenings=-1, dtype=np.float64):
        self.dtype = dtype
        self.ne = mg.level_extents(ne, max_coarsenings)
        self.fixed = [np.asarray(fixed, dtype=bool).reshape(-1)]
        for l in range(1, len(self.ne)):
            self.fixed.append(mg.coarse_mask(self.ne[l - 1], self.fixed[-1]))
        a = mg.fine_operator(ne, Ka, kap, self.fixed[0], dtype)
        b = mg.fine_operator(ne, capacity_matrix(np.asarray(mb).astype(dtype)), cp, self.fixed[0], dtype)
        self.P = []
        self.Ap = [mg.Op(a.shape, np.concatenate([a.rows, b.rows]), np.concatenate([a.cols, b.cols]), np.concatenate([a.vals, b.vals]))]
        for l in range(1, len(self.ne)):
            self.P.append(mg.prolongation(self.ne[l - 1], self.fixed[l - 1], self.fixed[l], dtype))
            self.Ap.append(mg.galerkin(self.P[-1], self.Ap[-1]))
        self.A = [mg.with_identity(Ap, f) for Ap, f in zip(self.Ap, self.fixed)]
        self.diag = [A.diagonal() for A in self.A]
        self.colours = [[(sel, A.take_rows(sel)) for sel in mg.colour_nodes(e) if sel.size] for e, A in zip(self.ne, self.A)]
        self.coarsest = self.A[-1].dense().astype(np.float64)


MG_SHAPES = [(16, 12), (12, 8, 16), (12, 264), (4, 4, 136), (7, 5)]
MG_DT, MG_THETA = 2.0, 0.5


@functools.lru_cache(maxsize=None)
def mg_case(ne, mask="sink"):
    """thermal_mg_cpu.case with random capacities and the Crank-Nicolson operator of a step dt = 2: Ka = Kc0 / 2, mb = m / 2; mask
    "none": no fixed node at all (the steady operator would be singular)"""
    c = dict(mg.case(ne, "sink" if mask == "none" else mask))
    rng = np.random.default_rng(4300 + tc.num_elements(ne))
    c["cp"] = cap(rng.uniform(0.05, 1.0, size=tc.num_elements(ne)))
    c["Ka"] = np.ascontiguousarray(MG_THETA * c["Kc0"])
    c["mb"] = np.ascontiguousarray(capacity_entries(tc.EDGES[c["N"]]) / MG_DT)
    if mask == "none":
        c["fixed"] = np.zeros_like(c["fixed"])
    return c


@functools.lru_cache(maxsize=None)
def mg_hierarchy(ne, mask="sink", long=False):
    c = mg_case(ne, mask)
    return Hierarchy(ne, c["Ka"], c["mb"], c["kap"], c["cp"], c["fixed"], dtype=np.longdouble if long else np.float64)


@functools.lru_cache(maxsize=None)
def mg_pcg_solution(ne, mask="sink"):
    """(x, info, direct solution) of the restatement's PCG on mg_case(ne, mask) with the right-hand side B (zero at the fixed nodes), tol 1e-8"""
    c, H = mg_case(ne, mask), mg_hierarchy(ne, mask)
    b = np.where(c["fixed"], 0.0, c["B"])
    x, info = H.pcg(b, tol=1e-8)
    return x, info, mg.direct_solve(H, b)


# what Hierarchy.pcg takes there (tests/test_transient_cpu.py recomputes and pins them)
MG_PCG_COUNT = {((16, 12), "sink"): 10, ((12, 8, 16), "sink"): 9, ((12, 264), "sink"): 12, ((4, 4, 136), "sink"): 10, ((16, 12), "none"): 10,
                ((12, 8, 16), "none"): 9}


# ---- the multigrid-PCG march against the direct march ----

MARCH_SHAPES = [(16, 12), (12, 8, 16)]


@functools.lru_cache(maxsize=None)
def march_fixture(ne):
    """thermal_cpu.pcg_fixture's problem (unit voxels, the middle-third sink, a unit volumetric source) marched over five backward-Euler
    steps of dt = 2000 from zero: the history approaches the steady state, so a step started from the one before takes fewer and fewer
    iterations (the restatement: 19, 18, 16, 16, 14 on 16 x 12 and 15, 14, 13, 12, 11 on 12 x 8 x 16 at tol 1e-10)"""
    f = mg.pcg_data(ne)
    return dict(ne=ne, h=f["h"], rho=f["rho"], fixed=f["fixed"], Q=f["Q"], steps=5, dt=2000.0, theta=1.0)


@functools.lru_cache(maxsize=None)
def march_both(ne, tol=1e-10):
    """(T by sparse direct solves, T by the multigrid-PCG warm-started from the step before, the PCG count of every step)"""
    f = march_fixture(ne)
    kap, cp = tc.kappa(f["rho"]), cap(f["rho"])
    Kc0, m = tc.conductivity_matrix(1.0, f["h"]), capacity_entries(f["h"])
    H = Hierarchy(ne, f["theta"] * Kc0, m / f["dt"], kap, cp, f["fixed"])
    Bop = Hierarchy(ne, -(1.0 - f["theta"]) * Kc0, m / f["dt"], kap, cp, f["fixed"], max_coarsenings=0).Ap[0]
    n = tc.num_nodes(ne)
    Td, Tp, counts = np.zeros((f["steps"] + 1, n)), np.zeros((f["steps"] + 1, n)), []
    for k in range(1, f["steps"] + 1):
        Td[k] = mg.direct_solve(H, Bop.matvec(Td[k - 1]) + f["Q"])
        Tp[k], info = H.pcg(Bop.matvec(Tp[k - 1]) + f["Q"], x0=Tp[k - 1], tol=tol)
        counts.append(info["iterations"])
    return Td, Tp, counts


# what march_both gives (tests/test_transient_cpu.py recomputes and pins them): the counts, and the largest difference of the two
# histories relative to the largest temperature
MARCH_COUNTS = {(16, 12): [19, 18, 16, 16, 14], (12, 8, 16): [15, 14, 13, 12, 11]}
MARCH_MEASURED = {(16, 12): 3.1e-12, (12, 8, 16): 1.3e-12}


@functools.lru_cache(maxsize=None)
def march_jacobi(ne, tol=1e-10):
    """(T by the Jacobi-PCG of thermal_cpu.pcg warm-started from the step before, the count of every step) on march_fixture(ne)"""
    f = march_fixture(ne)
    kap, cp = tc.kappa(f["rho"]), cap(f["rho"])
    A, B = operators(ne, tc.conductivity_matrix(1.0, f["h"]), capacity_entries(f["h"]), kap, cp, f["fixed"], f["dt"], f["theta"])
    T, counts = np.zeros((f["steps"] + 1, A.shape[0])), []
    for k in range(1, f["steps"] + 1):
        T[k], info = tc.pcg(A, B @ T[k - 1] + f["Q"], x0=T[k - 1], tol=tol)
        counts.append(info["iterations"])
    return T, counts


# the same for march_jacobi on 16 x 12: where its loop stops, and its difference from the direct march
MARCH_JACOBI_COUNTS = {(16, 12): [88, 88, 80, 80, 72]}
MARCH_JACOBI_MEASURED = {(16, 12): 1.9e-12}
