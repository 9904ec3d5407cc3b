"""numpy / scipy fp64 restatement of the thermo-elastic coupling, for the tests.  Nothing here comes from the library and
nothing uses the closed form of the coupling matrix: G is a 2-point Gauss quadrature of int beta_aq dN_n/dx_q N_m with the shape
functions written out here; the elastic chain is that of loadcases_cpu, the heat chain that of thermal_cpu, both dense.

Conventions: those of loadcases_cpu and thermal_cpu (last axis fastest, local node index with axis 0 as the most significant bit,
dof = N node + c).  theta = T - T_ref, beta = C : alpha:

    f_i = P (F_i + sum_e m_e Lb_i + sum_e E_e Lt_i + sum_e E_e G_i theta_e),   K u_i = f_i,   c_i = 1/2 f_i . u_i
    q = P_T sum_i a_i sum_e E_e G_i^T u_ie,   A mu = q
    dJ/drho_e = [loadcases_cpu.kernel_gradient] + dE_e sum_i a_i u_ie^T G_i theta_e - kappa'_e mu_e^T Kc0 T_e
"""
import functools

import numpy as np
import scipy.linalg

import homogenization_cpu as hc
import loadcases_cpu as lc
import stress_cpu as sc
import thermal_cpu as tc

GAUSS = lc.GAUSS


# ---- the coupling matrix by quadrature ----

def expansion_tensor(alpha, N):
    alpha = np.asarray(alpha, dtype=np.float64)
    return alpha * np.eye(N) if alpha.ndim == 0 else alpha.reshape(N, N)


def thermal_stress(D, alpha):
    """beta = C : alpha as a symmetric N x N matrix"""
    N = 2 if np.asarray(D).shape[0] == 3 else 3
    flat = lc.eigenstress(D, expansion_tensor(alpha, N))
    beta = np.zeros((N, N))
    for r, (i, j) in enumerate(hc.PAIRS[N]):
        beta[i, j] = beta[j, i] = flat[r]
    return beta


def shape_gradients(h, x):
    """dN_n/dx_q [npe, N] at the point x of the unit cube, for a voxel with the edge lengths h"""
    N = len(h)
    out = np.empty((2 ** N, N))
    for n, l in enumerate(np.ndindex(*([2] * N))):
        for q in range(N):
            v = (1.0 if l[q] else -1.0) / h[q]
            for d in range(N):
                if d != q:
                    v *= x[d] if l[d] else 1.0 - x[d]
            out[n, q] = v
    return out


def coupling_matrix(D, h, alpha):
    """G [ke, npe] = int beta_aq dN_n/dx_q N_m dV by two Gauss points per axis (exact: the integrand is quadratic along every axis)"""
    N = len(h)
    beta = thermal_stress(D, alpha)
    G = np.zeros((N * 2 ** N, 2 ** N))
    wgt = float(np.prod(h)) * 0.5 ** N
    for pt in np.ndindex(*([2] * N)):
        x = [GAUSS[i] for i in pt]
        rows = (shape_gradients(h, x) @ beta.T).reshape(-1)                 # [(n, a)] = sum_q beta[a][q] dN_n/dx_q
        G += wgt * np.outer(rows, lc.shape_values(N, x))
    return G


# ---- what the three kernels compute, in the number format asked for ----

def kernel_load(ne, G, tref, E, T, fixed=None, f_in=None, dtype=np.float64):
    """f [ndof] = P (f_in + sum_e E_e G (T_e - T_ref))"""
    N = len(ne)
    dofs, en = sc.element_dofs(ne), tc.element_nodes(ne)
    f = np.zeros(sc.num_nodes(ne) * N, dtype=dtype)
    if f_in is not None:
        f += np.asarray(f_in, dtype=dtype).reshape(-1)
    theta = np.asarray(T, dtype=dtype).reshape(-1)[en] - dtype(tref)                                # [elements, npe]
    np.add.at(f, dofs.reshape(-1), (np.asarray(E, dtype=dtype)[:, None] * (theta @ np.asarray(G, dtype=dtype).T)).reshape(-1))
    if fixed is not None:
        f[np.asarray(fixed, dtype=bool).reshape(-1)] = 0
    return f


def kernel_adjoint_source(ne, a, G, E, U, fixed=None, dtype=np.float64):
    """q [nodes] = P_T sum_i a_i sum_e E_e G_i^T u_ie; G [cases, ke, npe], U [cases, ndof]"""
    dofs, en = sc.element_dofs(ne), tc.element_nodes(ne)
    q = np.zeros(tc.num_nodes(ne), dtype=dtype)
    E = np.asarray(E, dtype=dtype)
    for i in range(len(U)):
        ue = np.asarray(U[i], dtype=dtype).reshape(-1)[dofs]                                        # [elements, ke]
        np.add.at(q, en.reshape(-1), (dtype(a[i]) * E[:, None] * (ue @ np.asarray(G[i], dtype=dtype))).reshape(-1))
    if fixed is not None:
        q[np.asarray(fixed, dtype=bool).reshape(-1)] = 0
    return q


def kernel_gradient(ne, a, G, tref, dE, T, U, g_in=None, dtype=np.float64):
    """g[e] = g_in[e] + dE_e sum_i a_i u_ie^T G_i (T_e - T_ref,i)"""
    dofs, en = sc.element_dofs(ne), tc.element_nodes(ne)
    Te = np.asarray(T, dtype=dtype).reshape(-1)[en]
    s = np.zeros(len(dofs), dtype=dtype)
    for i in range(len(U)):
        ue = np.asarray(U[i], dtype=dtype).reshape(-1)[dofs]
        s = s + dtype(a[i]) * np.einsum("ek,km,em->e", ue, np.asarray(G[i], dtype=dtype), Te - dtype(tref[i]))
    out = np.asarray(dE, dtype=dtype) * s
    return out if g_in is None else out + np.asarray(g_in, dtype=dtype)


# ---- the chain ----

def solve_lu(K, b):
    return np.linalg.solve(K.toarray() if hasattr(K, "toarray") else K, b)


def solve_cholesky(K, b):
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(K.toarray() if hasattr(K, "toarray") else K), b)


def solve_cg(K, b, tol=1e-12):
    """conjugate gradients to a relative residual of ``tol`` (stress_cpu.solve_cg), for the elastic and the heat operator alike"""
    import scipy.sparse
    if not b.any():
        return np.zeros_like(b)
    return sc.solve_cg(K if hasattr(K, "toarray") else scipy.sparse.csr_matrix(K), b, tol)


def heat_solution(p, rho, solve=solve_lu):
    """(T, A, Kc0, dkappa, fixed_T) of the problem's heat half at the densities rho"""
    ht = p["heat"]
    Kc0 = tc.conductivity_matrix(ht.get("k", 1.0), p["h"])
    fixed = np.asarray(ht["fixed"], dtype=bool).reshape(-1)
    A = tc.assemble(p["ne"], Kc0, tc.kappa(rho), fixed)
    Q = tc.load(p["ne"], p["h"], fixed, ht.get("nodal"), ht.get("volumetric"))
    return solve(A, Q), A, Kc0, tc.dkappa(rho), fixed


def evaluate(problem, rho=None, aggregate="sum", P=lc.P_NORM, solve=solve_lu, want_gradient=True):
    """the dense chain of a problem (``problem(name)`` or a dict of the same kind: those of loadcases_cpu with a ``heat`` dict --
    fixed [nodes], k, nodal, volumetric -- and cases that may have ``alpha`` and ``tref``), optionally at other densities; every
    solve, elastic or thermal, goes through ``solve``.  dict with T, f, u [cases, ndof], c, J, a, gradient and its three parts:
    ``explicit`` (the load-case terms and the coupling's dE term) and ``adjoint`` (the thermal adjoint term), and the per-case
    gradients"""
    p = problem
    ne, h, D = p["ne"], p["h"], p["D"]
    rho = np.asarray(p["rho"] if rho is None else rho, dtype=np.float64).reshape(-1)
    K0 = hc.element_constants(D, h)[0]
    E, dE = hc.moduli(rho, lc.E0, lc.EMIN, lc.GAMMA)
    m, dm = lc.mass_law(rho, **p.get("mass", {}))
    fixed = np.asarray(p["fixed"], dtype=bool).reshape(-1)
    K = sc.assemble(ne, K0, E, fixed)
    T, A, Kc0, dkap, fixed_T = heat_solution(p, rho, solve)
    k, ke, npe = len(p["cases"]), K0.shape[0], 2 ** len(ne)
    Lb, Lt, G, tref, fs, us = np.zeros((k, ke)), np.zeros((k, ke)), np.zeros((k, ke, npe)), np.zeros(k), [], []
    hot = [i for i, case in enumerate(p["cases"]) if case.get("alpha") is not None]
    for i, case in enumerate(p["cases"]):
        hasb, hast = case.get("g") is not None, case.get("eps") is not None
        if hasb:
            Lb[i] = lc.body_pattern(h, case["g"])
        if hast:
            Lt[i] = lc.eigenstrain_pattern(D, h, case["eps"])
        f = lc.kernel_assemble(ne, Lb[i] if hasb else None, Lt[i] if hast else None, m, E, fixed, case.get("F"))
        if i in hot:
            G[i], tref[i] = coupling_matrix(D, h, case["alpha"]), case.get("tref", 0.0)
            f = kernel_load(ne, G[i], tref[i], E, T, fixed, f)
        fs.append(f)
        us.append(solve(K, f))
    fs, us = np.array(fs), np.array(us)
    c = 0.5 * np.einsum("id,id->i", fs, us)
    w = np.array([case.get("w", 1.0) for case in p["cases"]])
    J, a = lc.aggregate_value(c, w, aggregate, P)
    out = dict(K0=K0, E=E, dE=dE, T=T, G=G, tref=tref, f=fs, u=us, c=c, w=w, J=J, a=a, fixed=fixed, fixed_T=fixed_T, hot=hot)
    if want_gradient:
        def parts(coef):
            explicit = lc.kernel_gradient(ne, K0, Lb, Lt, dE, dm, us, -0.5 * coef, coef, coef)
            explicit = kernel_gradient(ne, coef[hot], G[hot], tref[hot], dE, T, us[hot], explicit)
            q = kernel_adjoint_source(ne, coef[hot], G[hot], E, us[hot], fixed_T)
            mu = solve(A, q)
            return explicit, tc.gradient(ne, Kc0, dkap, [-1.0], mu[None], T[None])
        eye = np.eye(k)
        out["case_gradients"] = np.array([sum(parts(eye[i])) for i in range(k)])
        out["explicit"], out["adjoint"] = parts(a)
        out["gradient"] = out["explicit"] + out["adjoint"]
    return out


# ---- the fixtures ----

ALPHA2, ALPHA3 = 0.8, 0.58                  # the expansions of the heated cases: their compliances have the order of the mechanical ones
ALPHA_TENSOR = {2: np.array([[0.7, 0.1], [0.1, 0.4]]), 3: np.array([[0.7, 0.1, -0.05], [0.1, 0.4, 0.08], [-0.05, 0.08, 0.55]])}


@functools.lru_cache(maxsize=None)
def problem(name):
    """the design problems of the tests: those of loadcases_cpu plus a heat half (a uniform volumetric source, the sink on the middle
    third of the face x = 0, unit conductivity).
      plate2: 16 x 6, the x = 0 edge clamped; a point load at the far top corner, a heated case (scalar alpha, T_ref = 0.05) that also
        carries a point load, gravity
      block3 / block3even: 8 x 4 x 3 / 8 x 4 x 4, the x = 0 face clamped; the cantilever's point load, a heated case (tensor alpha),
        gravity along -y"""
    if name == "plate2":
        ne, h = (16, 6), (0.125, 0.125)
        D = hc.isotropic_D(1.0, 0.3, 2)
        nn = [n + 1 for n in ne]
        fixed = np.zeros(nn + [2], dtype=bool)
        fixed[0] = True
        fixed = fixed.reshape(-1, 2)
        tip = lc.point_load(ne, (16, 6), 1, -lc.POINT2)
        cases = [dict(F=tip, w=1.0), dict(F=0.5 * tip, alpha=ALPHA2, tref=0.05, w=0.75), dict(g=(0.0, -1.0), w=1.25)]
        source = 1.0
    elif name in ("block3", "block3even"):
        ne, h = ((8, 4, 3) if name == "block3" else (8, 4, 4)), (0.25, 0.25, 0.25)
        D = hc.isotropic_D(1.0, 0.3, 3)
        fixed, F = sc.cantilever(ne)
        cases = [dict(F=lc.POINT3 * F, w=1.0), dict(alpha=ALPHA_TENSOR[3] * ALPHA3, tref=-0.02, w=0.75), dict(g=(0.0, -1.0, 0.0), w=1.25)]
        source = 1.0
    else:
        raise KeyError(name)
    rho = np.random.default_rng(0).uniform(0.2, 1.0, size=int(np.prod(ne)))
    heat = dict(fixed=tc.face_mask(ne, 0, 0, middle_third=True), k=1.0, volumetric=source, nodal=None)
    return dict(name=name, ne=ne, h=h, D=D, rho=rho, fixed=fixed, cases=cases, mass={}, heat=heat)


@functools.lru_cache(maxsize=None)
def reference(name, aggregate="sum"):
    """the dense solution of a problem, computed once and shared (tests leave it unchanged)"""
    return evaluate(problem(name), aggregate=aggregate)


def chain_differences(name, aggregate, solve):
    """(values, gradient): the chain of a problem with another solver against its dense (LU) chain: J and every c_i relative, the
    gradient relative to its largest entry"""
    dense = reference(name, aggregate)
    other = evaluate(problem(name), aggregate=aggregate, solve=solve)
    values = max(abs(other["J"] - dense["J"]) / dense["J"], float((np.abs(other["c"] - dense["c"]) / dense["c"]).max()))
    return values, float(np.abs(other["gradient"] - dense["gradient"]).max() / np.abs(dense["gradient"]).max())


# what the chain with Cholesky solves differs from the chain with LU solves by, the largest over plate2 and block3 and both aggregates
# (the float64 floor of the chain; tests/test_thermoelastic_cpu.py computes and pins it); the GPU's direct path is bounded at
# max(1e-11, ten times this)
FLOOR_VALUE_MEASURED, FLOOR_GRADIENT_MEASURED = 4.4e-13, 1.0e-12
# the same for block3even with conjugate-gradient solves to 1e-12 (elastic and thermal); the PCG GPU tests are bounded at ten times these
CG_VALUE_MEASURED, CG_GRADIENT_MEASURED = 2.1e-14, 4.9e-14


def direct_bound():
    return max(1e-11, 10.0 * max(FLOOR_VALUE_MEASURED, FLOOR_GRADIENT_MEASURED))


def free_expansion(ne, h, D, a, seed=3):
    """loadcases_cpu.free_expansion by the T_ref route: no heat source, so T = 0, and T_ref = -1 with the expansion a, so theta = 1
    everywhere: (u error, c error, the problem, its solution with want_u and want_c, the largest difference of the load from the
    constant-eigenstrain load relative to its largest entry)"""
    N = len(ne)
    eu, ec, p0, r0 = lc.free_expansion(ne, h, D, a, seed)
    heat = dict(fixed=tc.face_mask(ne, 0, 0), k=1.0, volumetric=None, nodal=None)
    p = dict(p0, cases=[dict(alpha=a, tref=-1.0)], heat=heat)
    r = evaluate(p, want_gradient=False)
    err_u = float(np.abs(r["u"][0] - r0["want_u"]).max() / np.abs(r0["want_u"]).max())
    err_c = abs(r["c"][0] - r0["want_c"]) / r0["want_c"]
    err_f = float(np.abs(r["f"][0] - r0["f"][0]).max() / np.abs(r0["f"][0]).max())
    return err_u, err_c, p, dict(r, want_u=r0["want_u"], want_c=r0["want_c"]), err_f
