"""Plain numpy float64 restatement of the Method of Moving Asymptotes as DESIGN 3.12 states it (Svanberg 1987 / 2007 with a_i = 0,
d_i = 1, c_i = c), for the tests of ``ndr_amd.mma`` and of the ``vfem_mma_*`` entry points.

    min f_0(x)  subject to  f_i(x) <= 0 (i = 1 .. m),  xmin <= x <= xmax

The subproblem is solved by another route than the library's: Svanberg's primal-dual interior-point Newton method (``subsolv``) on
x, y, lambda and the slacks together, where the library runs a projected Newton iteration on the dual alone.  Both end by the same
stopping rule, which ``stopping_residual`` states once; the interior-point multipliers of the constraints that are not active are
set to zero before the rule is applied, and the step returned is x(lambda) of the multipliers that passed it.

Every term of the dual's sums is computed in one written order of operations, the order of ``ndr_amd/csrc/kernels_mma.hip`` (which
is compiled without contracted multiply-adds): a term is the same double here and there, and only the order of a sum differs.
"""
import math

import numpy as np

EPS = np.finfo(np.float64).eps


# ---------------------------------------------------------------------------------------------------------------------------
# the formulas
# ---------------------------------------------------------------------------------------------------------------------------

def asymptotes(it, x, xold1, xold2, xmin, xmax, L, U, asyinit=0.5, asyincr=1.2, asydecr=0.7):
    """(L, U) of step ``it`` (from 1)"""
    xm = np.maximum(xmax - xmin, 1e-5)
    if it <= 2:
        return x - asyinit * xm, x + asyinit * xm
    s = (x - xold1) * (xold1 - xold2)
    f = np.where(s > 0, asyincr, np.where(s < 0, asydecr, 1.0))
    l = x - f * (xold1 - L)
    u = x + f * (U - xold1)
    l = np.minimum(np.maximum(l, x - 10.0 * xm), x - 0.01 * xm)
    u = np.maximum(np.minimum(u, x + 10.0 * xm), x + 0.01 * xm)
    return l, u


def bounds(x, L, U, xmin, xmax, move=0.5):
    xm = np.maximum(xmax - xmin, 1e-5)
    alpha = np.maximum(np.maximum(xmin, L + 0.1 * (x - L)), x - move * xm)
    beta = np.minimum(np.minimum(xmax, U - 0.1 * (U - x)), x + move * xm)
    return alpha, beta


def pq(x, L, U, xmin, xmax, g):
    """(p, q) of one gradient, or of the rows of a stack of gradients"""
    xm = np.maximum(xmax - xmin, 1e-5)
    e = 1e-5 / xm
    ux, xl = U - x, x - L
    ux2, xl2 = ux * ux, xl * xl
    gp, gm = np.maximum(g, 0.0), np.maximum(-g, 0.0)
    return ux2 * ((1.001 * gp + 0.001 * gm) + e), xl2 * ((0.001 * gp + 1.001 * gm) + e)


class Subproblem:
    """the convex separable approximation at x: p, q of f_0 .. f_m, the bounds and b"""

    def __init__(self, x, L, U, xmin, xmax, g0, g, f, move=0.5, c=1000.0):
        as_array = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), np.shape(x)))
        self.x, self.L, self.U = as_array(x), as_array(L), as_array(U)
        self.xmin, self.xmax = as_array(xmin), as_array(xmax)
        self.g0, self.g = np.asarray(g0, dtype=np.float64), np.atleast_2d(np.asarray(g, dtype=np.float64))
        self.m, self.n = self.g.shape
        self.move, self.c = float(move), float(c)
        self.alpha, self.beta = bounds(self.x, self.L, self.U, self.xmin, self.xmax, self.move)
        self.p0, self.q0 = pq(self.x, self.L, self.U, self.xmin, self.xmax, self.g0)
        self.p, self.q = pq(self.x, self.L, self.U, self.xmin, self.xmax, self.g)
        self.f = None if f is None else np.asarray(f, dtype=np.float64).reshape(self.m)
        self.b = None
        if f is not None:
            rU, rL = 1.0 / (self.U - self.x), 1.0 / (self.x - self.L)
            self.b = np.array([math.fsum(self.p[i] * rU + self.q[i] * rL) for i in range(self.m)]) - self.f

    def PQ(self, lam):
        P, Q = self.p0.copy(), self.q0.copy()
        for i in range(self.m):
            P = P + lam[i] * self.p[i]
            Q = Q + lam[i] * self.q[i]
        return P, Q

    def x_of_lambda(self, lam):
        P, Q = self.PQ(lam)
        sP, sQ = np.sqrt(P), np.sqrt(Q)
        xs = (sP * self.L + sQ * self.U) / (sP + sQ)
        return np.minimum(np.maximum(xs, self.alpha), self.beta)

    def each_dual_sum(self, lam, b=None):
        """(name, index, terms) of every sum ``vfem_mma_dual_eval`` returns, one at a time so that a large case needs no
        [m][m][n] array: "W" (), "grad" (i,), "scale" (i,), "hess" (i, k) for i <= k.  The terms are the n terms of the variables
        (for hess: zero outside the open interval (alpha, beta)), then what lambda, b and y add.  p, q > 0, so the absolute terms of
        scale_i are the terms of G_i themselves."""
        lam = np.asarray(lam, dtype=np.float64)
        b = self.b if b is None else np.asarray(b, dtype=np.float64)
        P, Q = self.PQ(lam)
        xj = self.x_of_lambda(lam)
        rU, rL = 1.0 / (self.U - xj), 1.0 / (xj - self.L)
        y = np.maximum(0.0, lam - self.c)
        yield "W", (), np.concatenate([P * rU + Q * rL, -lam * b, -0.5 * y * y])
        for i in range(self.m):
            G = self.p[i] * rU + self.q[i] * rL
            yield "grad", (i,), np.concatenate([G, [-b[i], -y[i]]])
            yield "scale", (i,), np.concatenate([G, [abs(b[i]), y[i]]])
        rU2, rL2 = rU * rU, rL * rL
        w = 1.0 / (2.0 * (P * (rU2 * rU) + Q * (rL2 * rL)))
        free = (xj > self.alpha) & (xj < self.beta)
        for i in range(self.m):
            hw = (self.p[i] * rU2 - self.q[i] * rL2) * w
            for k in range(i, self.m):
                t = np.where(free, hw * (self.p[k] * rU2 - self.q[k] * rL2), 0.0)
                yield "hess", (i, k), np.concatenate([t, [1.0] if i == k and lam[i] > self.c else []])

    def dual(self, lam, b=None, exact=True):
        """(W, grad, scale, hess) as ``vfem_mma_dual_eval`` defines them, summed exactly (``math.fsum``) or by numpy"""
        total = math.fsum if exact else (lambda t: float(np.sum(t)))
        out = dict(W=np.zeros(()), grad=np.zeros(self.m), scale=np.zeros(self.m), hess=np.zeros((self.m, self.m)))
        for name, index, terms in self.each_dual_sum(lam, b):
            out[name][index] = out[name][index[::-1]] = total(terms)
        return float(out["W"]), out["grad"], out["scale"], out["hess"]

    def stopping_residual(self, lam, exact=True):
        """(max_i |r_i| / s_i, r, s): r_i = g_i where lambda_i > 0, else max(g_i, 0); s_i = sum_j (|p_ij| / (U - x_j) + |q_ij| / (x_j - L_j))
        + |b_i| + y_i at x = x(lambda)"""
        lam = np.asarray(lam, dtype=np.float64)
        _, grad, scale, _ = self.dual(lam, exact=exact)
        r = np.where(lam > 0, grad, np.maximum(grad, 0.0))
        return float(np.max(np.abs(r) / scale)), r, scale


# ---------------------------------------------------------------------------------------------------------------------------
# the subproblem by Svanberg's primal-dual interior-point method (subsolv of "MMA and GCMMA", 2007, with a = 0 and so without z)
# ---------------------------------------------------------------------------------------------------------------------------

def solve_subproblem(sp, tol=1e-9, max_newton=400):
    """(x_new, lambda, y, info): relaxed complementarity eps = 1, 0.1, ... ; each level by Newton steps on (x, y, lambda) with the
    slacks eliminated; from eps = 1e-4 on the multipliers are tested by ``stopping_residual`` after each level."""
    m, c = sp.m, sp.c
    act = sp.beta > sp.alpha                                # variables with alpha = beta do not take part: their terms are constants
    al, be, L, U = sp.alpha[act], sp.beta[act], sp.L[act], sp.U[act]
    p0, q0, p, q = sp.p0[act], sp.q0[act], sp.p[:, act], sp.q[:, act]
    xf = sp.alpha[~act]
    b = sp.b - np.array([np.sum(sp.p[i, ~act] / (sp.U[~act] - xf) + sp.q[i, ~act] / (xf - sp.L[~act])) for i in range(m)])
    x = 0.5 * (al + be)
    y, lam, s = np.ones(m), np.ones(m), np.ones(m)
    xsi, eta = np.maximum(1.0, 1.0 / (x - al)), np.maximum(1.0, 1.0 / (be - x))
    mu = np.maximum(1.0, 0.5 * c) * np.ones(m)

    def residual(x, y, lam, xsi, eta, mu, s, eps):
        ux, xl = U - x, x - L
        plam, qlam = p0 + lam @ p, q0 + lam @ q
        gvec = p @ (1.0 / ux) + q @ (1.0 / xl)
        return np.concatenate([plam / (ux * ux) - qlam / (xl * xl) - xsi + eta, c + y - mu - lam, gvec - y + s - b,
                               xsi * (x - al) - eps, eta * (be - x) - eps, mu * y - eps, lam * s - eps])

    eps, newton, info = 1.0, 0, None
    while True:
        res = residual(x, y, lam, xsi, eta, mu, s, eps)
        while np.max(np.abs(res)) > 0.9 * eps:
            newton += 1
            if newton > max_newton:
                raise RuntimeError("mma_cpu.solve_subproblem: %d Newton steps" % max_newton)
            ux, xl = U - x, x - L
            ux2, xl2 = ux * ux, xl * xl
            plam, qlam = p0 + lam @ p, q0 + lam @ q
            gvec = p @ (1.0 / ux) + q @ (1.0 / xl)
            GG = p / ux2 - q / xl2
            delx = plam / ux2 - qlam / xl2 - eps / (x - al) + eps / (be - x)
            dely = c + y - lam - eps / y
            dellam = gvec - y - b + eps / lam
            diagx = 2.0 * (plam / (ux2 * ux) + qlam / (xl2 * xl)) + xsi / (x - al) + eta / (be - x)
            diagy = 1.0 + mu / y
            Alam = np.diag(s / lam + 1.0 / diagy) + (GG / diagx) @ GG.T
            dlam = np.linalg.solve(Alam, dellam + dely / diagy - GG @ (delx / diagx))
            dx = -delx / diagx - (GG.T @ dlam) / diagx
            dy = -dely / diagy + dlam / diagy
            dxsi = -xsi + eps / (x - al) - xsi * dx / (x - al)
            deta = -eta + eps / (be - x) + eta * dx / (be - x)
            dmu = -mu + eps / y - mu * dy / y
            ds = -s + eps / lam - s * dlam / lam
            pos, dpos = np.concatenate([y, lam, xsi, eta, mu, s]), np.concatenate([dy, dlam, dxsi, deta, dmu, ds])
            step = 1.0 / max(1.0, np.max(-1.01 * dpos / pos), np.max(-1.01 * dx / (x - al)), np.max(1.01 * dx / (be - x)))
            norm = np.linalg.norm(res)
            for _ in range(60):
                new = (x + step * dx, y + step * dy, lam + step * dlam, xsi + step * dxsi, eta + step * deta, mu + step * dmu,
                       s + step * ds)
                res = residual(*new, eps)
                if np.linalg.norm(res) < norm:
                    break
                step *= 0.5
            x, y, lam, xsi, eta, mu, s = new
        if eps <= 1e-4:
            # a constraint that is not active keeps a multiplier of eps / slack: zero where the rule would not take it as it is
            _, grad, scale, _ = sp.dual(lam, exact=False)
            lam0 = np.where(-grad > tol * scale, 0.0, lam)
            rho, _, _ = sp.stopping_residual(lam0, exact=False)
            if rho <= tol:
                info = dict(newton=newton, eps=eps, residual=rho)
                lam = lam0
                break
        if eps < 1e-30:
            raise RuntimeError("mma_cpu.solve_subproblem: the stopping rule is not met at eps = %g" % eps)
        eps *= 0.1
    return sp.x_of_lambda(lam), lam, np.maximum(0.0, lam - c), info


# ---------------------------------------------------------------------------------------------------------------------------
# the optimiser
# ---------------------------------------------------------------------------------------------------------------------------

class MMA:
    """``step(f, g0, g)`` takes f_i(x) [m], df_0/dx [n], df_i/dx [m][n] at ``self.x`` and moves ``self.x``"""

    def __init__(self, x, xmin, xmax, move=0.5, c=1000.0, asyinit=0.5, asyincr=1.2, asydecr=0.7, tol=1e-9):
        self.x = np.array(x, dtype=np.float64)
        self.xmin = np.broadcast_to(np.asarray(xmin, dtype=np.float64), self.x.shape).copy()
        self.xmax = np.broadcast_to(np.asarray(xmax, dtype=np.float64), self.x.shape).copy()
        self.move, self.c, self.asy, self.tol = move, c, (asyinit, asyincr, asydecr), tol
        self.iteration, self.xold1, self.xold2, self.L, self.U = 0, None, None, None, None
        self.lambdas = None

    def step(self, f, g0, g):
        self.iteration += 1
        self.L, self.U = asymptotes(self.iteration, self.x, self.xold1, self.xold2, self.xmin, self.xmax, self.L, self.U, *self.asy)
        sp = Subproblem(self.x, self.L, self.U, self.xmin, self.xmax, g0, g, f, self.move, self.c)
        xnew, self.lambdas, _, _ = solve_subproblem(sp, self.tol)
        self.xold2, self.xold1, self.x = self.xold1, self.x, xnew
        return float(np.max(np.abs(xnew - self.xold1)))


# ---------------------------------------------------------------------------------------------------------------------------
# Svanberg's two test problems: (f_0, [f_i], df_0, [df_i]) of x, the start, the box
# ---------------------------------------------------------------------------------------------------------------------------

class Beam:
    """the five-segment cantilever of Svanberg 1987: min 0.0624 sum x  s.t.  61/x1^3 + 37/x2^3 + 19/x3^3 + 7/x4^3 + 1/x5^3 <= 1"""
    coef = np.array([61.0, 37.0, 19.0, 7.0, 1.0])
    x0, xmin, xmax = np.full(5, 5.0), 1.0, 10.0

    def __call__(self, x):
        return (0.0624 * np.sum(x), np.array([np.sum(self.coef / x ** 3) - 1.0]), np.full(5, 0.0624),
                np.array([-3.0 * self.coef / x ** 4]))


class Toy:
    """the three-variable problem of "MMA and GCMMA": min |x|^2  s.t.  |x - (5, 2, 1)|^2 <= 9,  |x - (3, 4, 3)|^2 <= 9,  0 <= x <= 5"""
    centres = np.array([[5.0, 2.0, 1.0], [3.0, 4.0, 3.0]])
    x0, xmin, xmax = np.array([4.0, 3.0, 2.0]), 0.0, 5.0

    def __call__(self, x):
        d = x[None, :] - self.centres
        return float(x @ x), np.sum(d * d, axis=1) - 9.0, 2.0 * x, 2.0 * d


# ---------------------------------------------------------------------------------------------------------------------------
# inputs of the subproblem tests: mixed-sign gradients with exact zeros, frozen variables, asymptotes at uneven distances
# ---------------------------------------------------------------------------------------------------------------------------

def random_subproblem(n, m, seed, infeasible=False, c=1000.0, move=0.5):
    rng = np.random.default_rng(seed)
    xmin, xmax = np.zeros(n), np.ones(n)
    x = rng.uniform(0.05, 0.95, n)
    frozen = rng.random(n) < 0.1
    frozen[0] = n > 3                                   # at n = 1 the one variable stays free
    x[frozen] = np.where(rng.random(n) < 0.5, 0.0, 1.0)[frozen]
    xmin[frozen] = xmax[frozen] = x[frozen]
    xm = np.maximum(xmax - xmin, 1e-5)
    L, U = x - rng.uniform(0.05, 1.5, n) * xm, x + rng.uniform(0.05, 1.5, n) * xm
    g0 = rng.standard_normal(n)
    g = rng.standard_normal((m, n)) / min(n, 256)       # multipliers of the order of min(n, 256): below c = 1000 when feasible
    g0[rng.random(n) < 0.1] = 0.0
    g[rng.random((m, n)) < 0.1] = 0.0
    # what the linearised f_i can lose inside the move limits is about 0.2 sum |g|: values inside that can be met, values far
    # above cannot, so that y_i > 0
    reach = 0.2 * np.sum(np.abs(g), axis=1)
    f = rng.uniform(-0.5, 0.5, m) * reach
    if infeasible:
        f[0] = 3.0 * reach[0] + 0.1
    return dict(x=x, L=L, U=U, xmin=xmin, xmax=xmax, g0=g0, g=g, f=f, move=move, c=c)


def tiled_subproblem(base, copies):
    """``copies`` copies of a subproblem side by side, with f multiplied by ``copies``: every sum of the dual, b and the scales s_i
    are ``copies`` times the base's, so where y = 0 the multipliers are the base's and x_new is the base's x_new, tiled.  A large
    subproblem whose solution the restatement finds at the base's cost."""
    tile = lambda a: np.tile(a, copies)
    out = {k: tile(base[k]) for k in ("x", "L", "U", "xmin", "xmax", "g0")}
    out.update(g=np.tile(base["g"], (1, copies)), f=base["f"] * copies, move=base["move"], c=base["c"])
    return out
