"""-m gpu: the Method of Moving Asymptotes on the device (ndr_amd.mma, vfem_mma_*) against tests/mma_cpu.py.

Bounds.
  (a) One dual pass against ``math.fsum`` of the restatement's terms: n eps sum |terms| for W, every gradient, scale and Hessian
      entry: the worst case of any order of summation, nothing measured.  The terms themselves are the same doubles on both sides
      (one written order of operations, no contracted multiply-adds), which the cases n = 1 and n = 5 show: there the bound is a
      few units in the last place.
  (b) The subproblem: |r_i| <= 10 tol s_i with r, s recomputed by fsum from the returned multipliers (the device's sums differ
      from the exact ones by at most n eps s_i = 2.3e-10 s_i at the largest n, tol = 1e-9); x_new = x(lambda) to 16 eps (U - L);
      alpha <= x_new <= beta and the frozen variables bit for bit.
  (c) x_new against the restatement's: TOL_X, ten times the farthest the restatement's own x_new moves between tol = 1e-9 and
      tol = 1e-11 on these inputs (measured on the CPU: 9.7e-9, see TOL_X).  The restatement needs 16 s for a million variables
      (about fifty Newton steps on all of x, m = 2), so for (c) the case one past the cap is 17 copies of a 61 681-variable
      subproblem side by side with f multiplied by 17 (mma_cpu.tiled_subproblem): its sums are 17 times the base's, so its
      multipliers and its x_new are the base's, and the restatement solves the base.  (a) and (b) run one past the cap on inputs
      that are random throughout.
  (d) Svanberg's beam and toy through ``MMAOptimizer``: 1e-6 relative of the SLSQP optimum from step 10 on.
  (e) 24 x 12 cantilever, direct solve, SmoothingFilter radius 1, volume constraint, 8 steps: every step's x_new against the
      restatement fed with the device's own f, gradients and history, to TOL_X.
  (f) The same grid with a frozen L-shaped void, volume and p-norm stress constraints: see the test.

Measured on an MI355X:
  (a) n = 1: the same bits; n = 5: 0.06; n = 255 / 257: 0.004; n = 4096 x 256 + 1: 1e-6; the 16-byte loads at M = 8 over more than
      one sweep: 2e-6 of the bound; second call and off-line views bit-identical.
  (b) residuals 3e-15 .. 8.9e-10 of the scale, the exact recomputation agrees to three digits; 4 .. 13 Newton iterations.
  (c) 3.1e-10 (n1), 9.2e-11 (n5), 4.4e-9 (n255), 4.5e-9 (n257), 9.0e-9 (n257_off), 6.3e-11 (n255_infeasible), 1.7e-9 (cap+1_tiled).
  (d) beam 2.6e-7 at step 5 and below 1e-8 from step 6; toy 4.0e-7 at step 4 and below 3e-9 from step 6.
  (e) at most 2.8e-9 over the eight steps; compliance 224.5 -> 101.7; dual iterations 7, 7, 7, 7, 6, 6, 6, 6.
  (f) constraints end at (5.7e-4, 0.79): the stress bound is met after the first step and not active afterwards.
  The whole file runs in under 8 s.  Against the parent commit every test fails at import: neither the module nor the entry
  points exist.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
from scipy.optimize import minimize

import mma_cpu as mc
import stress_cpu as sc

pytestmark = pytest.mark.gpu

from ndr_amd import _lib                                       # noqa: E402
from ndr_amd import mma                                        # noqa: E402
from ndr_amd import pyVoxelFEM as pv                           # noqa: E402
from ndr_amd import stress                                     # noqa: E402

EPS = np.finfo(np.float64).eps
TOL = 1e-9
# The restatement's x_new at tol = 1e-9 against its x_new at tol = 1e-11, largest entry, measured on the CPU over CASES:
# 2.7e-10 (n1), 1.1e-13 (n5), 2.2e-9 (n255), 4.5e-9 (n257), 9.7e-9 (n257_off), 6.3e-11 (n255_infeasible), 1.8e-9 (cap+1_tiled, on its base)
TOL_X = 10 * 9.7e-9
CAP = 4096 * 256                                               # threads of one grid-stride launch of the elementwise kernels

SWEEP = 2 * 1024 * 256                                         # variables of one grid-stride sweep of the dual pass

# name: (n, m, seed, infeasible, views 8 bytes off a 16-byte line, copies)
SMALL = {"n1": (1, 1, 1, False, False, 1), "n5": (5, 2, 2, False, False, 1), "n255": (255, 3, 3, False, False, 1),
         "n257": (257, 8, 4, False, False, 1), "n257_off": (257, 3, 7, False, True, 1),
         "n255_infeasible": (255, 2, 6, True, False, 1)}
# one past the cap: random throughout for (a) and (b); for (c), whose restatement takes 16 s on a million variables, 17 copies of a
# 61 681-variable subproblem (see the docstring)
CAP1 = {"cap+1": (CAP + 1, 2, 8, False, False, 1)}
TILED = {"cap+1_tiled": (61681, 2, 5, False, False, 17)}
assert 61681 * 17 == CAP + 1
# an even n with every row of g on a 16-byte line, more than one sweep and a partial second one: the 16-byte loads at M = 8
EVEN = {"sweep+514_m8": (SWEEP + 514, 8, 9, False, False, 1)}
CASES = {**SMALL, **CAP1, **TILED, **EVEN}
LAMBDAS = np.array([0.0, 3.7, 1200.0, 0.0, 15.0, 1000.5, 0.25, 80.0])        # zeros, and values above c = 1000


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, off=False):
    """a device copy; off: a view that starts 8 bytes off a 16-byte line"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not off:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    view = buf[1:].reshape(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8
    return view


@functools.lru_cache(maxsize=None)
def _case(name):
    """the inputs, the restatement's subproblem and the device copies of one case; shared, left unchanged"""
    n, m, seed, infeasible, off, copies = CASES[name]
    base = mc.random_subproblem(n, m, seed, infeasible=infeasible)
    d = mc.tiled_subproblem(base, copies) if copies > 1 else base
    sp = mc.Subproblem(**d)
    dev = {k: _dev(d[k], off) for k in ("x", "L", "U", "xmin", "xmax", "g0", "g")}
    return dict(name=name, n=n * copies, m=m, d=d, sp=sp, dev=dev, off=off, base=mc.Subproblem(**base) if copies > 1 else sp,
                copies=copies)


def _dual_eval(c, lam):
    m, v = c["m"], c["dev"]
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    b = np.ascontiguousarray(c["sp"].b)
    W, grad, scale, hess = ctypes.c_double(np.nan), np.full(m, np.nan), np.full(m, np.nan), np.full((m, m), np.nan)
    _lib.check(_lib.load().vfem_mma_dual_eval(c["n"], m, _p(v["x"]), _p(v["L"]), _p(v["U"]), _p(v["xmin"]), _p(v["xmax"]),
                                              c["d"]["move"], _p(v["g0"]), _p(v["g"]), _dp(b), c["d"]["c"], _dp(lam),
                                              ctypes.byref(W), _dp(grad), _dp(scale), _dp(hess), None))
    return W.value, grad, scale, hess


def _subproblem(c, tol=TOL, max_iter=200, xnew=None, **replace):
    m, v = c["m"], dict(c["dev"], **replace)
    f = np.ascontiguousarray(c["d"]["f"])
    xnew = _dev(np.full(c["n"], np.nan), c["off"]) if xnew is None else xnew
    lam, y, its, res = np.full(m, np.nan), np.full(m, np.nan), ctypes.c_int(-1), ctypes.c_double(np.nan)
    _lib.check(_lib.load().vfem_mma_subproblem(c["n"], m, _p(v["x"]), _p(v["L"]), _p(v["U"]), _p(v["xmin"]), _p(v["xmax"]),
                                               replace.get("move", c["d"]["move"]), _dp(f), _p(v["g0"]), _p(v["g"]), c["d"]["c"], tol,
                                               max_iter, _p(xnew), _dp(lam), _dp(y), ctypes.byref(its), ctypes.byref(res), None))
    return xnew.cpu().numpy(), lam, y, its.value, res.value


@functools.lru_cache(maxsize=None)
def _solved(name):
    return _subproblem(_case(name))


# ---- (a) the fused dual pass ----

@pytest.mark.parametrize("name", list(SMALL) + list(CAP1) + list(EVEN))
def test_dual_pass_matches_the_exact_sums(name):
    c = _case(name)
    n, m, sp = c["n"], c["m"], c["sp"]
    aligned = all(t.data_ptr() % 16 == 0 for t in c["dev"].values()) and (m == 1 or n % 2 == 0)
    assert aligned == (name in ("n1",) + tuple(EVEN))         # which cases take the 16-byte loads
    for lam in (LAMBDAS[:m], np.roll(LAMBDAS, -2)[:m])[:1 if name in EVEN else 2]:        # (53 exact sums of half a million terms: once)
        W, grad, scale, hess = _dual_eval(c, lam)
        device = dict(W=np.array(W), grad=grad, scale=scale, hess=hess)
        worst = 0.0
        for what, index, terms in sp.each_dual_sum(lam):
            value = float(device[what][index])
            exact, bound = math.fsum(terms.tolist()), n * EPS * math.fsum(np.abs(terms).tolist())
            print("%s %s%s: device %.17g exact %.17g difference %.3g bound %.3g" % (name, what, list(index), value, exact,
                                                                                  abs(value - exact), bound))
            assert abs(value - exact) <= bound, (what, index, value, exact, bound)
            worst = max(worst, abs(value - exact) / bound if bound > 0 else 0.0)
        assert np.array_equal(hess, hess.T)
        again = _dual_eval(c, lam)
        assert again[0] == W and all(np.array_equal(a, b) for a, b in zip(again[1:], (grad, scale, hess)))     # the same bits
        print("%s lambda %s: largest difference %.3g of its bound" % (name, lam, worst))


def test_dual_pass_does_not_depend_on_the_alignment():
    """the 16-byte and the 8-byte loads read the same elements in the same partition: the same bits from views off the line"""
    n, m, seed = 257, 3, 7
    d = mc.random_subproblem(n, m, seed)
    sp = mc.Subproblem(**d)
    c = {a: dict(name="x", n=n, m=m, d=d, sp=sp, off=a, dev={k: _dev(d[k], a) for k in ("x", "L", "U", "xmin", "xmax", "g0", "g")})
         for a in (False, True)}
    # n is odd, so the second row of g is off the line in the aligned copy as well: an even n for the aligned path
    lam = LAMBDAS[1:4]
    off = _dual_eval(c[True], lam)
    on = _dual_eval(c[False], lam)
    assert on[0] == off[0] and all(np.array_equal(a, b) for a, b in zip(on[1:], off[1:]))
    n = 256
    d = {k: (v[..., :n] if isinstance(v, np.ndarray) and v.shape[-1:] == (257,) else v) for k, v in d.items()}
    d = {k: np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v for k, v in d.items()}
    sp = mc.Subproblem(**d)
    res = []
    for a in (False, True):
        dev = {k: _dev(d[k], a) for k in ("x", "L", "U", "xmin", "xmax", "g0")}
        g = _dev(d["g"].reshape(-1), a).reshape(m, n)
        assert all((g[i].data_ptr() % 16 == 8) == a for i in range(m))
        res.append(_dual_eval(dict(name="x", n=n, m=m, d=d, sp=sp, off=a, dev=dict(dev, g=g)), lam))
    assert res[0][0] == res[1][0] and all(np.array_equal(a, b) for a, b in zip(res[0][1:], res[1][1:]))
    for (what, index, terms), value in zip(sp.each_dual_sum(lam), res[0][:1]):
        assert what == "W" and abs(value - math.fsum(terms)) <= n * EPS * math.fsum(np.abs(terms))


# ---- (b), (c) the subproblem ----

@pytest.mark.parametrize("name", list(SMALL) + list(CAP1) + list(TILED))
def test_subproblem_meets_the_stopping_rule_and_the_bounds(name):
    c = _case(name)
    sp, d = c["sp"], c["d"]
    xnew, lam, y, its, res = _solved(name)
    assert np.all(lam >= 0) and np.array_equal(y, np.maximum(0.0, lam - d["c"])) and 0 <= its <= 200
    rho, r, s = sp.stopping_residual(lam)                     # fsum
    print("%s: lambda %s y %s, %d Newton iterations, residual %.3g (device) %.3g (exact)" % (name, lam, y, its, res, rho))
    assert np.all(np.abs(r) <= 10 * TOL * s), (r, s)
    assert res <= TOL
    expect = sp.x_of_lambda(lam)
    assert np.all(np.abs(xnew - expect) <= 16 * EPS * (d["U"] - d["L"]))
    assert np.all(xnew >= sp.alpha) and np.all(xnew <= sp.beta)
    frozen = d["xmin"] == d["xmax"]
    assert np.array_equal(xnew[frozen], d["x"][frozen]) and (frozen.any() or c["n"] < 4)
    if "infeasible" in name:
        assert y[0] > 0 and lam[0] > d["c"]
    if c["copies"] > 1:
        assert np.all(y == 0)                                 # what makes the tiled case the base case (c)


@pytest.mark.parametrize("name", list(SMALL) + list(TILED))
def test_subproblem_step_matches_the_restatement(name):
    c = _case(name)
    xnew, lam, y, _, _ = _solved(name)
    ref_x, ref_lam, ref_y, info = mc.solve_subproblem(c["base"], TOL)
    ref_x = np.tile(ref_x, c["copies"])
    print("%s: x_new differs by %.3g (bound %.3g), lambda %s against %s" % (name, np.abs(xnew - ref_x).max(), TOL_X, lam, ref_lam))
    assert np.abs(xnew - ref_x).max() <= TOL_X
    assert np.array_equal(lam > 0, ref_lam > 0) and np.array_equal(y > 0, ref_y > 0)


def test_subproblem_twice_gives_the_same_bits():
    c = _case("n257")
    a, b = _subproblem(c), _solved("n257")
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3:] == b[3:]


def test_asymptote_kernel():
    n = CAP + 1
    rng = np.random.default_rng(9)
    xmin, xmax = np.zeros(n), rng.choice([1.0, 2.0], n)
    xmin[::7] = xmax[::7] = 0.25                              # frozen: xm = 1e-5
    xold2, xold1, x = (np.clip(rng.uniform(-0.2, 1.2, n), xmin, xmax) for _ in range(3))
    x[::5] = xold1[::5]                                       # stood still: factor 1
    L0, U0 = xold1 - rng.uniform(0.01, 3.0, n), xold1 + rng.uniform(0.01, 3.0, n)
    lib = _lib.load()
    for it in (1, 2, 3):
        L, U = _dev(L0), _dev(U0)
        held = [_dev(a) for a in (x, xold1, xold2, xmin, xmax)]
        args = [_p(t) for t in held]
        if it == 1:
            args[1] = args[2] = None
        _lib.check(lib.vfem_mma_asymptotes(n, it, *args, 0.5, 1.2, 0.7, _p(L), _p(U), None))
        eL, eU = mc.asymptotes(it, x, xold1, xold2, xmin, xmax, L0, U0)
        assert np.array_equal(L.cpu().numpy(), eL) and np.array_equal(U.cpu().numpy(), eU)      # the same operations in the same order


# ---- (d) the optimiser on Svanberg's two problems ----

class _SmallProblem:
    """the interface ``MMAOptimizer`` uses, over a function of a handful of variables; c_i = -f_i"""

    def __init__(self, fn):
        self.fn, self.x, self.sets = fn, None, 0

    def numVars(self):
        return len(self.fn.x0)

    def getVars_device(self):
        return self.x

    def setVars(self, x):
        self.x, self.sets = x.clone(), self.sets + 1
        self.val = self.fn(self.x.cpu().numpy())

    def evaluateObjective(self):
        return self.val[0]

    def evaluateObjectiveGradient_device(self):
        return torch.from_numpy(np.ascontiguousarray(self.val[2])).cuda()

    def evaluateConstraints(self):
        return -self.val[1]

    def evaluateConstraintsJacobian_device(self):
        return [torch.from_numpy(np.ascontiguousarray(-row)).cuda() for row in self.val[3]]


@pytest.mark.parametrize("fn,optimum", [(mc.Beam(), 1.3399564), (mc.Toy(), 8.7702459)], ids=["beam", "toy"])
def test_optimizer_reaches_the_optimum_of_beam_and_toy(fn, optimum):
    m = len(fn(fn.x0)[1])
    cons = [{"type": "ineq", "fun": (lambda x, i=i: -fn(x)[1][i]), "jac": (lambda x, i=i: -fn(x)[3][i])} for i in range(m)]
    best = minimize(lambda x: fn(x)[0], fn.x0, jac=lambda x: fn(x)[2], constraints=cons, method="SLSQP",
                    bounds=[(fn.xmin, fn.xmax)] * len(fn.x0), options=dict(ftol=1e-12, maxiter=500)).fun
    assert abs(best - optimum) < 1e-7
    p = _SmallProblem(fn)
    p.setVars(torch.from_numpy(fn.x0.copy()).cuda())
    opt = mma.MMAOptimizer(p, xmin=fn.xmin, xmax=fn.xmax)
    values = []
    for k in range(15):
        change = opt.step()
        values.append(p.evaluateObjective())
        print("step %d: f %.10f, relative %.3g, change %.3g, lambda %s, %d dual iterations" % (
            k + 1, values[-1], abs(values[-1] - best) / best, change, opt.lambdas, opt.dualIterations))
    assert opt.iteration == 15 and p.sets == 16               # one setVars per step
    rel = np.abs(np.array(values) - best) / best
    assert np.all(rel[9:] < 1e-6), rel
    assert np.max(fn(p.x.cpu().numpy())[1]) < 1e-6


# ---- (e), (f) the design loop ----

NE, H = (24, 12), (1.0 / 12, 1.0 / 12)
XLOW = 1e-3


def _cantilever(ne=NE, h=H):
    N = len(ne)
    sim = pv.TensorProductSimulator([1] * N, [np.zeros(N), np.array(ne) * np.array(h)], list(ne))
    sim.ETensor = pv.ElasticityTensor(1.0, 0.3, dim=N)
    sim.E_0, sim.E_min, sim.gamma = 1.0, 1e-3, 3.0
    fixed, f = sc.cantilever(ne)
    sim.dirichletMask = fixed
    sim.setLoads_device(torch.from_numpy(f).cuda())
    sim.setUniformDensities(0.4)
    return sim


def _smoothing():
    f = pv.SmoothingFilter()
    f.radius = 1
    return f


class _Recorded:
    """a problem seen through what ``MMAOptimizer`` asks of it, keeping the answers of the step in ``rec`` (f = -c, g = -dc)"""

    def __init__(self, problem):
        self._problem, self.rec = problem, {}

    def numVars(self):
        return self._problem.numVars()

    def getVars_device(self):
        x = self._problem.getVars_device()
        self.rec = dict(x=x.cpu().numpy().copy())
        return x

    def evaluateObjectiveGradient_device(self):
        g0 = self._problem.evaluateObjectiveGradient_device()
        self.rec["g0"] = g0.cpu().numpy().copy()
        return g0

    def evaluateConstraints(self):
        values = self._problem.evaluateConstraints()
        self.rec["f"] = -np.asarray(values, dtype=np.float64)
        return values

    def evaluateConstraintsJacobian_device(self):
        rows = self._problem.evaluateConstraintsJacobian_device()
        self.rec["g"] = -np.stack([r.cpu().numpy() for r in rows])
        return rows

    def setVars(self, x):
        self.rec["xnew"] = x.cpu().numpy().copy()
        return self._problem.setVars(x)


def test_design_loop_matches_the_restatement_step_by_step():
    sim = _cantilever()
    objective = pv.ComplianceObjective(sim)
    problem = pv.TopologyOptimizationProblem(sim, objective, [pv.TotalVolumeConstraint(0.4)], [_smoothing()])
    n = problem.numVars()
    problem.setVars(np.full(n, 0.4))
    start = problem.evaluateObjective()
    seen = _Recorded(problem)
    opt = mma.MMAOptimizer(seen)
    xmin, xmax = np.zeros(n), np.ones(n)
    hist, L, U, worst, duals = [], None, None, 0.0, []
    for k in range(8):
        before = sim.numDirectFactorizations()
        opt.step()
        assert sim.numDirectFactorizations() == before + 1
        rec = seen.rec
        x = rec["x"]
        L, U = mc.asymptotes(k + 1, x, hist[-1] if hist else None, hist[-2] if len(hist) > 1 else None, xmin, xmax, L, U)
        dL, dU = (t.cpu().numpy() for t in opt.asymptotes_device())
        assert np.array_equal(dL, L) and np.array_equal(dU, U)
        sp = mc.Subproblem(x, L, U, xmin, xmax, rec["g0"], rec["g"], rec["f"])
        ref, ref_lam, _, _ = mc.solve_subproblem(sp, TOL)
        worst = max(worst, np.abs(rec["xnew"] - ref).max())
        duals.append(opt.dualIterations)
        print("step %d: compliance %.6f, volume constraint %.3g, x_new differs by %.3g, lambda %s (restatement %s), %d dual iterations"
              % (k + 1, problem.evaluateObjective(), problem.evaluateConstraints()[0], np.abs(rec["xnew"] - ref).max(), opt.lambdas,
                 ref_lam, opt.dualIterations))
        assert np.abs(rec["xnew"] - ref).max() <= TOL_X
        assert np.array_equal(problem.getVars(), rec["xnew"])
        hist.append(x)
    print("dual iterations per step: %s; largest difference %.3g" % (duals, worst))
    assert problem.evaluateObjective() < start
    assert problem.evaluateConstraints()[0] >= -1e-6


def _void(ne):
    """the upper right quarter is cut out of the rectangle: an L-shaped design domain"""
    v = np.zeros(ne, dtype=bool)
    v[ne[0] // 2:, ne[1] // 2:] = True
    return v.reshape(-1)


def test_two_constraints_on_the_l_shape_end_feasible_with_one_factorisation_per_step():
    """Volume <= 0.4 and p-norm stress <= 0.9 of the start's measure on the L-shape; the void is frozen at the lower bound (positive:
    the relaxed stress has an unbounded derivative at density 0).  The start violates the stress bound by 11 %.

    Asserted: both constraints END feasible to 1e-3 (they are normalised: 1 - J / bound and 1 - volume / 0.4, so their scale is 1).
    Every subproblem holds the convex approximations of both constraints with y = 0 wherever that is possible, so a step ends
    feasible up to the approximation's error, which shrinks with the steps; monotone improvement is not a property of MMA (the
    asymptotes open and a step may overshoot), so it is not what is asserted."""
    sim = _cantilever()
    compliance = pv.ComplianceObjective(sim)
    void = _void(NE)
    xmin, xmax = np.full(void.size, XLOW), np.ones(void.size)
    xmax[void] = XLOW
    x0 = np.where(void, XLOW, 0.4)
    measure = stress.PNormStressObjective(compliance)
    # the bound comes from the start's measure: set the start once to read it
    volume = pv.TotalVolumeConstraint(0.4)
    problem = pv.TopologyOptimizationProblem(sim, compliance, [volume], [_smoothing()])
    problem.setVars(x0)
    bound = 0.9 * measure.evaluate()
    capped = mma.ObjectiveConstraint(measure, bound)
    problem.constraints = [volume, capped]
    opt = mma.MMAOptimizer(problem, xmin=xmin, xmax=xmax)
    first = problem.evaluateConstraints()
    assert first[0] > 0 and abs(first[1] - (1 - 1 / 0.9)) < 1e-12
    for k in range(10):
        before = sim.numDirectFactorizations()
        opt.step()
        cons = problem.evaluateConstraints()
        print("step %d: compliance %.6f, constraints %s, lambda %s, %d dual iterations" % (
            k + 1, problem.evaluateObjective(), cons, opt.lambdas, opt.dualIterations))
        assert sim.numDirectFactorizations() == before + 1            # the stress measure reuses the step's solve and its factor
        x = problem.getVars()
        assert np.array_equal(x[void], x0[void]) and np.all(x >= xmin) and np.all(x <= xmax)
    assert np.all(cons >= -1e-3), cons
    assert abs(measure.evaluate() / bound - (1 - cons[1])) < 1e-12


def test_multigrid_3d_wiring():
    ne = (16, 8, 8)
    sim = _cantilever(ne, (0.125, 0.125, 0.125))
    compliance = pv.MultigridComplianceObjective(sim.multigridSolver(1))
    measure = stress.PNormStressObjective(compliance)
    volume = pv.TotalVolumeConstraint(0.4)
    problem = pv.TopologyOptimizationProblem(sim, compliance, [volume], [_smoothing()])
    n = problem.numVars()
    problem.setVars(np.full(n, 0.4))
    start = problem.evaluateObjective()
    problem.constraints = [volume, mma.ObjectiveConstraint(measure, 1.1 * measure.evaluate())]
    opt = mma.MMAOptimizer(problem, xmin=XLOW)
    for k in range(3):
        change = opt.step()
        print("step %d: compliance %.6f, constraints %s, change %.3g" % (k + 1, problem.evaluateObjective(), problem.evaluateConstraints(), change))
        assert 0 < change <= 0.5
    x = problem.getVars()
    assert opt.iteration == 3 and np.all(x >= XLOW) and np.all(x <= 1) and np.isfinite(problem.evaluateObjective())
    assert np.all(np.isfinite(problem.evaluateConstraints())) and np.isfinite(start)


def test_volume_objective_and_objective_constraint():
    x = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, 1000)).cuda()
    v = mma.VolumeObjective()
    with pytest.raises(RuntimeError):
        v.evaluate()
    v.updateCache(x)
    assert abs(v.evaluate() - float(x.mean())) < 1e-14 and np.array_equal(v.gradient(), np.full(1000, 1e-3))
    c = mma.ObjectiveConstraint(v, 0.5)
    assert abs(c.evaluate_dev(x) - (1 - v.evaluate() / 0.5)) < 1e-15
    assert np.array_equal(c.backprop(x), np.full(1000, -1e-3 / 0.5))
    calls = []
    v.updateCache = lambda xp, keep=v.updateCache: (calls.append(1), keep(xp))[1]
    c.evaluate_dev(x), c.backprop_dev(x.clone())
    assert calls == []                                        # the same densities: no update
    c.evaluate_dev(x * 0.5)
    assert calls == [1] and abs(v.evaluate() - 0.5 * float(x.mean())) < 1e-15
    with pytest.raises(RuntimeError):
        mma.ObjectiveConstraint(v, 0.0)


def test_objective_constraint_solves_for_densities_that_were_set_without_a_solve():
    """the simulator holding xPhys is not enough: the shared solver must have solved since the densities changed"""
    sim = _cantilever()
    compliance = pv.ComplianceObjective(sim)
    capped = mma.ObjectiveConstraint(stress.PNormStressObjective(compliance), 1.0)
    x = torch.full((sim.numElements(),), 0.4, dtype=torch.float64, device="cuda")
    compliance.updateCache(x)
    before = sim.numDirectFactorizations()
    at_x = capped.evaluate_dev(x)
    assert sim.numDirectFactorizations() == before            # the solve of its owner serves
    half = (0.5 * x).contiguous()
    sim.setElementDensities(half)                             # nobody solved
    at_half = capped.evaluate_dev(half)
    assert sim.numDirectFactorizations() == before + 1 and at_half != at_x
    fresh = stress.PNormStressObjective(pv.ComplianceObjective(sim)).evaluate()
    assert abs((1.0 - at_half) - fresh) <= 1e-12 * fresh
    capped.backprop_dev(half)
    assert sim.numDirectFactorizations() == before + 1        # and only once


# ---- (g) refusals ----

def test_refused_arguments_raise_before_any_launch():
    c = _case("n255")
    v = c["dev"]
    nan = lambda: _dev(np.full(c["n"], np.nan))

    def refused(message, **kw):
        xnew = kw.pop("xnew", None)
        xnew = nan() if xnew is None else xnew
        untouched = xnew.clone()
        with pytest.raises(RuntimeError, match=message):
            _subproblem(c, xnew=xnew, **kw)
        assert torch.equal(torch.nan_to_num(xnew, nan=-7.0), torch.nan_to_num(untouched, nan=-7.0))      # nothing was written

    small = dict(c, n=0)
    with pytest.raises(RuntimeError, match="n must be at least 1"):
        _subproblem(small)
    refused("null argument", x=None)
    refused("null argument", g=None)
    for key in ("x", "L", "U", "xmin", "xmax", "g0"):
        copy = v[key].clone()
        with pytest.raises(RuntimeError, match="xnew aliases an input"):
            _subproblem(c, xnew=copy, **{key: copy})
        assert torch.equal(copy, v[key])
    g = v["g"].clone()
    with pytest.raises(RuntimeError, match="xnew aliases an input"):
        _subproblem(c, xnew=g[1], g=g)
    assert torch.equal(g, v["g"])
    refused("move must be positive", move=0.0)
    refused("move must be positive", move=-0.5)
    refused("tol must be positive", tol=0.0)
    refused("max_iter must be at least 1", max_iter=0)
    for m_bad in (0, 9):
        with pytest.raises(RuntimeError, match="must be 1 to 8"):
            _subproblem(dict(c, m=m_bad, d=dict(c["d"], f=np.zeros(9))))
    lib = _lib.load()
    L, U = nan(), nan()
    base = [_p(v["x"]), _p(v["x"]), _p(v["x"]), _p(v["xmin"]), _p(v["xmax"])]
    for (init, incr, decr), message in (((0.5, 1.2, 0.0), "asydecr"), ((0.5, 1.2, 1.0), "asydecr"), ((0.5, 0.99, 0.7), "asyincr"),
                                        ((0.0, 1.2, 0.7), "asyinit")):
        with pytest.raises(RuntimeError, match=message):
            _lib.check(lib.vfem_mma_asymptotes(c["n"], 3, *base, init, incr, decr, _p(L), _p(U), None))
    with pytest.raises(RuntimeError, match="n must be at least 1"):
        _lib.check(lib.vfem_mma_asymptotes(0, 1, *base, 0.5, 1.2, 0.7, _p(L), _p(U), None))
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.check(lib.vfem_mma_asymptotes(c["n"], 3, base[0], None, None, base[3], base[4], 0.5, 1.2, 0.7, _p(L), _p(U), None))
    assert bool(torch.isnan(L).all()) and bool(torch.isnan(U).all())
    with pytest.raises(RuntimeError, match="lambda must be finite and not negative"):
        _dual_eval(c, -LAMBDAS[1:4])


def test_nine_constraints_and_the_iteration_cap_raise():
    sim = _cantilever()
    objective = pv.ComplianceObjective(sim)
    nine = [pv.TotalVolumeConstraint(0.4 + 0.01 * i) for i in range(9)]
    problem = pv.TopologyOptimizationProblem(sim, objective, nine, [_smoothing()])
    x0 = np.full(problem.numVars(), 0.4)
    problem.setVars(x0)
    with pytest.raises(RuntimeError, match="1 to 8 constraints"):
        mma.MMAOptimizer(problem).step()
    problem.constraints = nine[:1]
    opt = mma.MMAOptimizer(problem, maxDualIterations=1)
    with pytest.raises(RuntimeError, match="not solved after 1 Newton iterations: residual"):
        opt.step()
    assert opt.iteration == 0 and np.array_equal(problem.getVars(), x0)      # nothing moved
    opt.maxDualIterations = 200
    opt.step()
    assert opt.iteration == 1 and opt.dualIterations > 1
    with pytest.raises(RuntimeError, match="leave"):
        mma.MMAOptimizer(problem, xmin=0.9).step()
