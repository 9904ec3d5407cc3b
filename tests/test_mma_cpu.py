"""The numpy restatement of the Method of Moving Asymptotes (tests/mma_cpu.py) pinned on its own, without a GPU: the subproblem's
solution against SLSQP on the primal subproblem, Svanberg's two test problems against SLSQP on the problems themselves, frozen
variables, the asymptote rule on hand-made histories, and the agreement of the dual's derivatives with its values."""
import math

import numpy as np
import pytest
from scipy.optimize import minimize

import mma_cpu as mc


def _slsqp(problem):
    f = lambda x: problem(x)
    m = len(f(problem.x0)[1])
    cons = [{"type": "ineq", "fun": (lambda x, i=i: -f(x)[1][i]), "jac": (lambda x, i=i: -f(x)[3][i])} for i in range(m)]
    r = minimize(lambda x: f(x)[0], problem.x0, jac=lambda x: f(x)[2], constraints=cons, method="SLSQP",
                 bounds=[(problem.xmin, problem.xmax)] * len(problem.x0), options=dict(ftol=1e-12, maxiter=500))
    assert r.success
    return r


@pytest.mark.parametrize("problem,optimum,needed", [(mc.Beam(), 1.3399564, 6), (mc.Toy(), 8.7702459, 5)], ids=["beam", "toy"])
def test_beam_and_toy_reach_their_optima(problem, optimum, needed):
    r = _slsqp(problem)
    assert abs(r.fun - optimum) < 1e-7
    opt = mc.MMA(problem.x0, problem.xmin, problem.xmax)
    values = []
    for _ in range(15):
        _, f, g0, g = problem(opt.x)
        opt.step(f, g0, g)
        values.append(problem(opt.x)[0])
    rel = np.abs(np.array(values) - r.fun) / r.fun
    assert np.all(rel[needed - 1:] < 1e-6), rel
    assert np.max(problem(opt.x)[1]) < 1e-6


@pytest.mark.parametrize("n,m,seed,infeasible", [(1, 1, 11, False), (3, 2, 12, False), (6, 2, 13, False), (6, 3, 14, True)])
def test_subproblem_solution_equals_slsqp_on_the_primal_subproblem(n, m, seed, infeasible):
    """min over alpha <= x <= beta, y >= 0 of  sum_j (p0/(U - x) + q0/(x - L)) + sum_i (c y_i + y_i^2 / 2)  subject to
    sum_j (p_i/(U - x) + q_i/(x - L)) - b_i - y_i <= 0: strictly convex, so SLSQP and the restatement end at the same point"""
    d = mc.random_subproblem(n, m, seed, infeasible=infeasible, c=10.0)
    sp = mc.Subproblem(**d)
    xnew, lam, y, _ = mc.solve_subproblem(sp, 1e-11)
    approx = lambda p, q, x: np.sum(p / (sp.U - x) + q / (x - sp.L), axis=-1)
    dapprox = lambda p, q, x: p / (sp.U - x) ** 2 - q / (x - sp.L) ** 2
    scale = approx(sp.p0, sp.q0, sp.x)
    cost = lambda v: (approx(sp.p0, sp.q0, v[:n]) + np.sum(sp.c * v[n:] + 0.5 * v[n:] ** 2)) / scale
    dcost = lambda v: np.concatenate([dapprox(sp.p0, sp.q0, v[:n]), sp.c + v[n:]]) / scale
    cons = [{"type": "ineq", "fun": (lambda v, i=i: -(approx(sp.p[i], sp.q[i], v[:n]) - sp.b[i] - v[n + i])),
             "jac": (lambda v, i=i: -np.concatenate([dapprox(sp.p[i], sp.q[i], v[:n]), -np.eye(m)[i]]))} for i in range(m)]
    start = np.concatenate([0.5 * (sp.alpha + sp.beta), np.ones(m)])
    r = minimize(cost, start, jac=dcost, constraints=cons, method="SLSQP", options=dict(ftol=1e-15, maxiter=1000),
                 bounds=list(zip(sp.alpha, sp.beta)) + [(0.0, None)] * m)
    assert r.status in (0, 8), r.message         # 8: its line search finds nothing better, the end of the road at ftol = 1e-15
    assert np.abs(r.x[:n] - xnew).max() < 1e-6 and np.abs(r.x[n:] - y).max() < 1e-5, (r.x, xnew, y)
    assert abs(cost(np.concatenate([xnew, y])) - r.fun) < 1e-9 * abs(r.fun)
    if infeasible:
        assert y[0] > 0 and lam[0] > sp.c
    assert np.all(xnew >= sp.alpha) and np.all(xnew <= sp.beta)


def test_frozen_variables_stay_put():
    d = mc.random_subproblem(257, 3, 21)
    frozen = d["xmin"] == d["xmax"]
    assert 5 < frozen.sum() < 100
    xnew = mc.solve_subproblem(mc.Subproblem(**d))[0]
    assert np.array_equal(xnew[frozen], d["x"][frozen])
    assert np.abs(xnew[~frozen] - d["x"][~frozen]).max() > 1e-3
    # through whole steps as well: the beam with its middle segment fixed
    beam = mc.Beam()
    xmin, xmax = np.full(5, 1.0), np.full(5, 10.0)
    xmin[2] = xmax[2] = 5.0
    opt = mc.MMA(beam.x0, xmin, xmax)
    for _ in range(6):
        _, f, g0, g = beam(opt.x)
        opt.step(f, g0, g)
        assert opt.x[2] == 5.0
    assert abs(beam(opt.x)[1][0]) < 1e-5                 # the constraint is still met with equality by the other four


def test_asymptote_rules_on_hand_made_histories():
    xmin, xmax = np.zeros(3), np.array([1.0, 2.0, 1.0])
    x = np.array([0.5, 1.0, 0.5])
    L, U = mc.asymptotes(1, x, None, None, xmin, xmax, None, None)
    assert np.array_equal(L, x - 0.5 * (xmax - xmin)) and np.array_equal(U, x + 0.5 * (xmax - xmin))
    assert all(np.array_equal(a, b) for a, b in zip(mc.asymptotes(2, x, x, None, xmin, xmax, L, U), (L, U)))
    # variable 0 keeps its direction, variable 1 turns, variable 2 stood still once
    xold2, xold1, x = np.array([0.3, 1.0, 0.5]), np.array([0.4, 1.2, 0.5]), np.array([0.5, 1.1, 0.6])
    L1, U1 = xold1 - np.array([0.5, 1.0, 0.5]), xold1 + np.array([0.5, 1.0, 0.5])
    L, U = mc.asymptotes(3, x, xold1, xold2, xmin, xmax, L1, U1)
    for j, factor in enumerate((1.2, 0.7, 1.0)):
        assert L[j] == x[j] - factor * (xold1[j] - L1[j]) and U[j] == x[j] + factor * (U1[j] - xold1[j])
    # an oscillating variable's asymptotes close in until 0.01 (xmax - xmin), a monotone one's open up to 10 (xmax - xmin)
    for step, limit in ((lambda k: 0.5 + 0.1 * (-1) ** k, 0.01), (lambda k: 0.1 + 0.001 * k, 10.0)):
        xs = [np.array([step(k)]) for k in range(60)]
        L, U = mc.asymptotes(1, xs[0], None, None, np.zeros(1), np.ones(1), None, None)
        for k in range(2, 60):
            L, U = mc.asymptotes(k + 1, xs[k], xs[k - 1], xs[k - 2], np.zeros(1), np.ones(1), L, U)
            assert xs[k][0] - 10.0 <= L[0] <= xs[k][0] - 0.01 and xs[k][0] + 0.01 <= U[0] <= xs[k][0] + 10.0
        assert math.isclose(xs[-1][0] - L[0], limit, rel_tol=1e-12) and math.isclose(U[0] - xs[-1][0], limit, rel_tol=1e-12)


def test_dual_gradient_and_hessian_are_the_derivatives_of_its_value():
    d = mc.random_subproblem(257, 3, 31)
    sp = mc.Subproblem(**d)
    lam = np.array([40.0, 3.0, 1200.0])                   # the last one above c: y_3 > 0
    W, grad, scale, hess = sp.dual(lam)
    h = 1e-4
    for i in range(3):
        e = np.zeros(3)
        e[i] = h
        Wp, gp, _, _ = sp.dual(lam + e)
        Wm, gm, _, _ = sp.dual(lam - e)
        assert abs((Wp - Wm) / (2 * h) - grad[i]) < 1e-6 * scale[i]
        # W is concave: hess is minus its second derivative; variables change sides of their bounds inside 2 h, hence 1e-3
        assert np.abs(-(gp - gm) / (2 * h) - hess[i]).max() < 1e-3 * np.abs(hess).max()
    assert np.all(np.linalg.eigvalsh(hess) > -1e-12 * np.abs(hess).max())
    assert np.all(scale > 0)


def test_stopping_rule_holds_at_the_returned_multipliers():
    for n, m, seed, infeasible in ((5, 2, 41, False), (255, 3, 42, False), (257, 8, 43, False), (255, 2, 44, True)):
        sp = mc.Subproblem(**mc.random_subproblem(n, m, seed, infeasible=infeasible))
        xnew, lam, y, info = mc.solve_subproblem(sp, 1e-9)
        rho, r, s = sp.stopping_residual(lam)
        assert rho <= 1e-9 * (1 + 1e-3) and np.array_equal(xnew, sp.x_of_lambda(lam)) and np.array_equal(y, np.maximum(0, lam - sp.c))
