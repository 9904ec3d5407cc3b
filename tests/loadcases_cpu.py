"""numpy / scipy fp64 restatement of the load-case chain, for the tests.  Nothing here comes from the library and nothing uses the
closed forms of the element load patterns: the patterns are 2-point Gauss quadratures of int N g and int B^T sigma* with the shape
functions and the strain matrix of stress_cpu, the stiffness matrix is assembled by scipy and solved densely.

Conventions: those of stress_cpu (last axis fastest, local node index with axis 0 as the most significant bit, dof = N node + c).

    f_i = P (F_i + sum_e m_e Lb_i + sum_e E_e Lt_i),   Lb_i = int N g_i dV,   Lt_i = int B^T (C : eps*_i) dV
    K u_i = f_i,  c_i = 1/2 f_i . u_i,  dc_i/drho_e = -1/2 dE_e u_ie^T K0 u_ie + dm_e Lb_i . u_ie + dE_e Lt_i . u_ie
    "sum": J = sum w_i c_i;  "pnorm": J = (sum (w_i c_i)^P)^(1/P);  dJ/drho = sum_i a_i dc_i/drho
"""
import functools

import numpy as np

import homogenization_cpu as hc
import stress_cpu as sc

E0, EMIN, GAMMA = 1.0, 1e-3, 3.0
P_NORM = 8.0
GAUSS = (0.5 - 0.5 / np.sqrt(3.0), 0.5 + 0.5 / np.sqrt(3.0))


# ---- the element patterns by quadrature ----

def shape_values(N, x):
    """N_n(x) [npe] at the point x of the unit cube"""
    return np.array([np.prod([x[d] if l[d] else 1.0 - x[d] for d in range(N)]) for l in np.ndindex(*([2] * N))])


def body_pattern(h, g):
    """Lb [ke] = int N_n g_a dV"""
    N = len(h)
    out = np.zeros(N * 2 ** N)
    wgt = float(np.prod(h)) * 0.5 ** N
    for q in np.ndindex(*([2] * N)):
        out += wgt * np.outer(shape_values(N, [GAUSS[i] for i in q]), np.asarray(g, dtype=np.float64)).reshape(-1)
    return out


def flat_strain(eps):
    """the tensor components of a symmetric N x N matrix in the order of the flattened tensors"""
    eps = np.asarray(eps, dtype=np.float64)
    return np.array([eps[i, j] for i, j in hc.PAIRS[eps.shape[0]]])


def eigenstress(D, eps):
    """sigma* = C : eps*, flattened"""
    e = flat_strain(eps)
    return np.asarray(D, dtype=np.float64) @ (sc.mult(np.asarray(eps).shape[0]) * e)


def eigenstrain_pattern(D, h, eps):
    """Lt [ke] = int B^T sigma* dV (virtual work: the shear components count twice)"""
    N = len(h)
    sig = sc.mult(N) * eigenstress(D, eps)
    out = np.zeros(N * 2 ** N)
    wgt = float(np.prod(h)) * 0.5 ** N
    for q in np.ndindex(*([2] * N)):
        out += wgt * sc.strain_matrix(h, [GAUSS[i] for i in q]).T @ sig
    return out


def mass_law(rho, massDensity=1.0, massExponent=1.0, lowDensityCut=None):
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    d, r = float(massDensity), float(massExponent)
    m, dm = d * rho ** r, d * r * rho ** (r - 1.0)
    if lowDensityCut is not None:
        c = float(lowDensityCut)
        low = rho < c
        m = np.where(low, d * (6.0 * rho ** 6 / c ** 5 - 5.0 * rho ** 7 / c ** 6), m)
        dm = np.where(low, d * (36.0 * rho ** 5 / c ** 5 - 35.0 * rho ** 6 / c ** 6), dm)
    return m, dm


# ---- what the two kernels compute, in the number format asked for ----

def kernel_assemble(ne, Lb, Lt, m, E, fixed=None, f_in=None, dtype=np.float64):
    """f [ndof] = P (f_in + sum_e m_e Lb + sum_e E_e Lt); a pattern (with its multipliers) may be None"""
    N = len(ne)
    dofs = sc.element_dofs(ne)
    f = np.zeros(sc.num_nodes(ne) * N, dtype=dtype)
    if f_in is not None:
        f += np.asarray(f_in, dtype=dtype).reshape(-1)
    if Lb is not None:
        np.add.at(f, dofs.reshape(-1), (np.asarray(m, dtype=dtype)[:, None] * np.asarray(Lb, dtype=dtype)[None]).reshape(-1))
    if Lt is not None:
        np.add.at(f, dofs.reshape(-1), (np.asarray(E, dtype=dtype)[:, None] * np.asarray(Lt, dtype=dtype)[None]).reshape(-1))
    if fixed is not None:
        f[np.asarray(fixed, dtype=bool).reshape(-1)] = 0
    return f


def kernel_gradient(ne, K0, Lb, Lt, dE, dm, U, cK, cB, cT, dtype=np.float64):
    """g[e] = dE_e sum_i cK_i u_ie^T K0 u_ie + dm_e sum_i cB_i Lb_i . u_ie + dE_e sum_i cT_i Lt_i . u_ie; Lb, Lt [cases, ke] or None"""
    dofs = sc.element_dofs(ne)
    K0, dE = np.asarray(K0, dtype=dtype), np.asarray(dE, dtype=dtype)
    sK = np.zeros(len(dofs), dtype=dtype)
    sB, sT = np.zeros_like(sK), np.zeros_like(sK)
    for i in range(len(U)):
        ue = np.asarray(U[i], dtype=dtype).reshape(-1)[dofs]
        sK = sK + dtype(cK[i]) * np.einsum("ek,kl,el->e", ue, K0, ue)
        if Lb is not None:
            sB = sB + dtype(cB[i]) * (ue @ np.asarray(Lb[i], dtype=dtype))
        if Lt is not None:
            sT = sT + dtype(cT[i]) * (ue @ np.asarray(Lt[i], dtype=dtype))
    out = dE * sK + dE * sT
    if Lb is not None:
        out = out + np.asarray(dm, dtype=dtype) * sB
    return out


# ---- the chain ----

def aggregate_value(c, w, aggregate, P=P_NORM):
    """(J, a = dJ/dc)"""
    c, w = np.asarray(c, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if aggregate == "sum":
        return float(np.sum(w * c)), w.copy()
    wc = w * c
    top = float(wc.max())
    if top == 0.0:
        return 0.0, np.zeros_like(w)
    J = top * float(np.sum((wc / top) ** P)) ** (1.0 / P)
    return J, w * (wc / J) ** (P - 1.0)


def solve_dense(K, b):
    return np.linalg.solve(K.toarray(), b)


def evaluate(problem, rho=None, aggregate="sum", P=P_NORM, solve=solve_dense, want_gradient=True):
    """the dense chain of a problem (``problem(name)`` or a dict of the same kind), optionally at other densities: dict with f, u
    [cases, ndof], c [cases], J, a, gradient, the per-case gradients and the element constants"""
    p = problem
    ne, h, D = p["ne"], p["h"], p["D"]
    rho = np.asarray(p["rho"] if rho is None else rho, dtype=np.float64).reshape(-1)
    K0 = hc.element_constants(D, h)[0]
    E, dE = hc.moduli(rho, E0, EMIN, GAMMA)
    m, dm = mass_law(rho, **p.get("mass", {}))
    fixed = np.asarray(p["fixed"], dtype=bool).reshape(-1)
    K = sc.assemble(ne, K0, E, fixed)
    k = len(p["cases"])
    ke = K0.shape[0]
    Lb, Lt, fs, us = np.zeros((k, ke)), np.zeros((k, ke)), [], []
    for i, case in enumerate(p["cases"]):
        hasb, hast = case.get("g") is not None, case.get("eps") is not None
        if hasb:
            Lb[i] = body_pattern(h, case["g"])
        if hast:
            Lt[i] = eigenstrain_pattern(D, h, case["eps"])
        f = kernel_assemble(ne, Lb[i] if hasb else None, Lt[i] if hast else None, m, E, fixed, case.get("F"))
        fs.append(f)
        us.append(solve(K, f))
    fs, us = np.array(fs), np.array(us)
    c = 0.5 * np.einsum("id,id->i", fs, us)
    w = np.array([case.get("w", 1.0) for case in p["cases"]])
    J, a = aggregate_value(c, w, aggregate, P)
    out = dict(K0=K0, K=K, E=E, dE=dE, m=m, dm=dm, Lb=Lb, Lt=Lt, f=fs, u=us, c=c, w=w, J=J, a=a, fixed=fixed)
    if want_gradient:
        eye = np.eye(k)
        out["case_gradients"] = np.array([kernel_gradient(ne, K0, Lb, Lt, dE, dm, us, -0.5 * eye[i], eye[i], eye[i]) for i in range(k)])
        out["gradient"] = kernel_gradient(ne, K0, Lb, Lt, dE, dm, us, -0.5 * a, a, a)
    return out


# ---- the fixtures ----

def corners_pinned(ne):
    """2-D: both bottom corners (y = 0, x = 0 and x = max) pinned in both components"""
    nn = [int(n) + 1 for n in ne]
    fixed = np.zeros(nn + [2], dtype=bool)
    fixed[0, 0] = fixed[-1, 0] = True
    return fixed.reshape(-1, 2)


def determinate_supports(ne):
    """statically determinate: node 0 fixed in every component, the far node of its x-line in the remaining ones, and in 3-D the
    far node of its y-line in z: no rigid motion is left and a free expansion is not hindered"""
    N = len(ne)
    nn = [int(n) + 1 for n in ne]
    fixed = np.zeros(nn + [N], dtype=bool)
    fixed[(0,) * N] = True
    fixed[(nn[0] - 1,) + (0,) * (N - 1)][1:] = True
    if N == 3:
        fixed[0, nn[1] - 1, 0, 2] = True
    return fixed.reshape(-1, N)


def node_positions(ne, h):
    nn = [int(n) + 1 for n in ne]
    return np.stack(np.meshgrid(*[np.arange(n) * hd for n, hd in zip(nn, h)], indexing="ij"), -1).reshape(-1, len(ne))


def point_load(ne, where, component, value):
    nn = [int(n) + 1 for n in ne]
    f = np.zeros(nn + [len(ne)])
    f[tuple(where) + (component,)] = value
    return f.reshape(-1, len(ne))


def orthotropic_D(N):
    """a positive definite orthotropic flattened tensor (axes along the grid)"""
    if N == 2:
        return np.array([[1.6, 0.3, 0.0], [0.3, 0.7, 0.0], [0.0, 0.0, 0.25]])
    D = np.zeros((6, 6))
    D[:3, :3] = [[1.8, 0.35, 0.3], [0.35, 1.1, 0.25], [0.3, 0.25, 0.7]]
    D[3, 3], D[4, 4], D[5, 5] = 0.2, 0.3, 0.4
    return D


# the isotropic eigenstrain of the thermal cases and the sizes of the point loads: chosen so that the three compliances of a fixture
# have one order of magnitude (the problem is linear: a p-norm over cases of very different sizes would test one case only)
THERMAL = 2.0
POINT2, POINT3 = 0.5, 0.4


@functools.lru_cache(maxsize=None)
def problem(name):
    """the design problems of the tests: dict with ne, h, D, rho (uniform in [0.2, 1] from default_rng(0)), fixed [numNodes, N],
    cases (dicts with F [numNodes, N] / g / eps / w) and the mass law.
      arch2: 16 x 6, both bottom corners pinned; a point load at the middle of the top, gravity, a uniform heating
      arch2_traffic: the same supports, two point loads on the top at a quarter and three quarters of the span (fixed loads only)
      arch2_weight: gravity alone
      block3 / block3even: 8 x 4 x 3 / 8 x 4 x 4, the x = 0 face clamped; the cantilever's point load, gravity along -y, heating"""
    if name.startswith("arch2"):
        ne, h = (16, 6), (0.125, 0.125)
        D = hc.isotropic_D(1.0, 0.3, 2)
        fixed = corners_pinned(ne)
        if name == "arch2":
            cases = [dict(F=point_load(ne, (8, 6), 1, -POINT2), w=1.0), dict(g=(0.0, -1.0), w=1.25), dict(eps=THERMAL * np.eye(2), w=0.75)]
        elif name == "arch2_traffic":
            cases = [dict(F=point_load(ne, (4, 6), 1, -1.0), w=1.0), dict(F=point_load(ne, (12, 6), 1, -1.0), w=1.0)]
        elif name == "arch2_weight":
            cases = [dict(g=(0.0, -1.0), w=1.0)]
        elif name == "arch2_bridge":
            cases = [dict(F=point_load(ne, (4, 6), 1, -0.25), g=(0.0, -1.0), w=1.0), dict(F=point_load(ne, (12, 6), 1, -0.25), g=(0.0, -1.0), w=1.0)]
        else:
            raise KeyError(name)
    elif name in ("block3", "block3even"):
        ne, h = ((8, 4, 3) if name == "block3" else (8, 4, 4)), (0.25, 0.25, 0.25)
        D = hc.isotropic_D(1.0, 0.3, 3)
        fixed, F = sc.cantilever(ne)
        cases = [dict(F=POINT3 * F, w=1.0), dict(g=(0.0, -1.0, 0.0), w=1.25), dict(eps=THERMAL * np.eye(3), w=0.75)]
    else:
        raise KeyError(name)
    rho = np.random.default_rng(0).uniform(0.2, 1.0, size=int(np.prod(ne)))
    return dict(name=name, ne=ne, h=h, D=D, rho=rho, fixed=fixed, cases=cases, mass={})


@functools.lru_cache(maxsize=None)
def reference(name, aggregate="sum"):
    """the dense solution of a problem, computed once and shared (tests leave it unchanged)"""
    return evaluate(problem(name), aggregate=aggregate)


def free_expansion(ne, h, D, a, seed=3):
    """a body on statically determinate supports heated uniformly (eps* = a I): (largest |u - a (x - x_0)| / largest |u|,
    |c - 1/2 eps*:C:eps* sum_e E_e vol| / c, the problem, its solution)"""
    N = len(ne)
    rho = np.random.default_rng(seed).uniform(0.2, 1.0, size=int(np.prod(ne)))
    p = dict(ne=ne, h=h, D=D, rho=rho, fixed=determinate_supports(ne), cases=[dict(eps=a * np.eye(N))], mass={})
    r = evaluate(p, want_gradient=False)
    want_u = (a * node_positions(ne, h)).reshape(-1)
    e = flat_strain(a * np.eye(N))
    want_c = 0.5 * float((sc.mult(N) * e) @ eigenstress(D, a * np.eye(N))) * float(r["E"].sum()) * float(np.prod(h))
    return float(np.abs(r["u"][0] - want_u).max() / np.abs(want_u).max()), abs(r["c"][0] - want_c) / want_c, p, dict(r, want_u=want_u, want_c=want_c)


# the free-expansion cases of the CPU and the GPU tests and what tests/test_loadcases_cpu.py measured on them (its docstring)
FREE = {"2": ((16, 6), (0.125, 0.125)), "3": ((6, 4, 3), (0.25, 0.2, 0.3))}
FREE_U_MEASURED = {("2", "isotropic"): 1.8e-13, ("2", "orthotropic"): 1.2e-13, ("3", "isotropic"): 7.9e-13, ("3", "orthotropic"): 3.9e-13}
FREE_C_MEASURED = {("2", "isotropic"): 2.2e-15, ("2", "orthotropic"): 2.0e-16, ("3", "isotropic"): 0.0, ("3", "orthotropic"): 1.4e-16}


def free_tensor(dim, kind):
    N = int(dim)
    return hc.isotropic_D(1.0, 0.3, N) if kind == "isotropic" else orthotropic_D(N)


def free_c_bound(dim, kind):
    """ten times what the restatement measures; where that figure is no more than one rounding of c itself (2^-52: it says that c
    came out exact or one unit off, not how large the error of a sum of ndof rounded products may be), ndof x 2^-52 instead"""
    ne = FREE[dim][0]
    measured = FREE_C_MEASURED[(dim, kind)]
    return 10.0 * measured if measured > 2.0 ** -52 else sc.num_nodes(ne) * len(ne) * 2.0 ** -52


# what the restatement's chain on block3even with conjugate-gradient solves to a relative residual of 1e-12 (stress_cpu.solve_cg)
# differs from its dense chain by, the larger of the two aggregates: the values (J and every c_i, relative) and the gradient (of its
# largest entry).  tests/test_loadcases_cpu.py computes and pins both; the multigrid GPU test is bounded at ten times them.
CG_VALUE_MEASURED, CG_GRADIENT_MEASURED = 8.9e-14, 5.7e-14


def cg_chain_differences(aggregate):
    """(values, gradient): the chain of block3even with CG solves to 1e-12 against the dense chain"""
    p = problem("block3even")
    dense = reference("block3even", aggregate)
    cg = evaluate(p, aggregate=aggregate, solve=lambda K, b: sc.solve_cg(K, b, 1e-12))
    values = max(abs(cg["J"] - dense["J"]) / dense["J"], float((np.abs(cg["c"] - dense["c"]) / dense["c"]).max()))
    return values, float(np.abs(cg["gradient"] - dense["gradient"]).max() / np.abs(dense["gradient"]).max())
