"""-m "not gpu": pins tests/loadcases_cpu.py, the restatement the GPU tests of ndr_amd.loadcases compare with, and the argument
refusals of vfem_loads_assemble / vfem_loads_gradient, which come before any device call.

Measured with this file (printed by every test):
  central differences of J, step 1e-5, direction default_rng(1): arch2 sum 4.40e-10, pnorm 1.07e-9; block3 sum 4.40e-9, pnorm 3.46e-9
    of the directional derivative; the bounds are ten times these.
  free thermal expansion (eps* = 0.01 I, densities uniform in [0.2, 1], statically determinate supports): u against a (x - x_0),
    relative to the largest displacement: 16 x 6 isotropic 1.8e-13, orthotropic 1.2e-13; 6 x 4 x 3 isotropic 7.9e-13, orthotropic
    3.9e-13; the bounds are ten times these.  c against 1/2 eps*:C:eps* sum_e E_e vol: 2.2e-15, 2.0e-16, 0, 1.4e-16 relative.  The
    first is bounded at ten times itself, 2.2e-14.  The other three are no more than one rounding of c (2^-52 = 2.2e-16): such a
    figure says that c came out exact or one unit off, and ten times it bounds nothing, so their bound is ndof x 2^-52 (c is a sum
    of ndof products, each rounded once): 5.3e-14 on 16 x 6, 9.3e-14 on 6 x 4 x 3.
  chain with conjugate-gradient solves to 1e-12 against the dense chain on block3even: values 8.9e-14, gradient 5.6e-14 (the bounds
    of the multigrid GPU test are ten times the recorded 8.9e-14 and 5.7e-14).
  self-weight: sum_n f_n = g sum_e m_e vol to 1.2e-16; the 16 x 6 arch under its own weight has 58 positive and 38 negative
    gradient entries, the smallest 8.5e-4 of the largest (no sign hangs on rounding).
"""
import ctypes

import numpy as np
import pytest

import homogenization_cpu as hc
import loadcases_cpu as lc
import stress_cpu as sc

FD_STEP = 1e-5
FD_MEASURED = {("arch2", "sum"): 4.40e-10, ("arch2", "pnorm"): 1.07e-9, ("block3", "sum"): 4.40e-9, ("block3", "pnorm"): 3.46e-9}
ARCH_SIGNS = (58, 38)


@pytest.mark.parametrize("aggregate", ["sum", "pnorm"])
@pytest.mark.parametrize("name", ["arch2", "block3"])
def test_central_difference_of_the_aggregate(name, aggregate):
    p = lc.problem(name)
    r = lc.evaluate(p, aggregate=aggregate)
    d = np.random.default_rng(1).standard_normal(p["rho"].size)
    an = float(r["gradient"] @ d)
    J = lambda rho: lc.evaluate(p, rho, aggregate, want_gradient=False)["J"]
    fd = (J(p["rho"] + FD_STEP * d) - J(p["rho"] - FD_STEP * d)) / (2.0 * FD_STEP)
    err = abs(fd - an) / abs(an)
    print("central difference %s %s: %.2e (bound %.2e); c = %s, a = %s" % (name, aggregate, err, 10 * FD_MEASURED[(name, aggregate)], r["c"], r["a"]))
    assert err < 10.0 * FD_MEASURED[(name, aggregate)]
    # the gradient of J is the a-weighted sum of the case gradients, and every case enters
    assert np.allclose(r["gradient"], r["a"] @ r["case_gradients"], rtol=1e-13, atol=1e-13 * np.abs(r["gradient"]).max())
    assert (r["c"] > 0).all() and (r["a"] > 0).all()


@pytest.mark.parametrize("name", ["arch2", "block3"])
def test_central_difference_of_every_case(name):
    p = lc.problem(name)
    r = lc.reference(name)
    d = np.random.default_rng(1).standard_normal(p["rho"].size)
    plus, minus = (lc.evaluate(p, p["rho"] + s * FD_STEP * d, want_gradient=False)["c"] for s in (1.0, -1.0))
    fd = (plus - minus) / (2.0 * FD_STEP)
    an = r["case_gradients"] @ d
    print("central difference per case %s: %s" % (name, np.abs(fd - an) / np.abs(an)))
    assert (np.abs(fd - an) < 1e-7 * np.abs(an)).all()


@pytest.mark.parametrize("kind", ["isotropic", "orthotropic"])
@pytest.mark.parametrize("dim", ["2", "3"])
def test_free_thermal_expansion_is_an_identity_of_the_discretisation(dim, kind):
    ne, h = lc.FREE[dim]
    eu, ec, p, r = lc.free_expansion(ne, h, lc.free_tensor(dim, kind), 0.01)
    print("free expansion %s %s: u %.2e (bound %.2e), c %.2e (bound %.2e)" % (dim, kind, eu, 10 * lc.FREE_U_MEASURED[(dim, kind)], ec,
                                                                            lc.free_c_bound(dim, kind)))
    assert eu < 10.0 * lc.FREE_U_MEASURED[(dim, kind)] and ec < lc.free_c_bound(dim, kind)
    assert not r["u"][0][r["fixed"]].any()


def test_chain_with_conjugate_gradient_solves_matches_the_dense_chain():
    """what the multigrid GPU test may differ by: every u_i from a conjugate gradient to a relative residual of 1e-12
    (stress_cpu.solve_cg) instead of the dense solve, on block3even.  Measured here: values (J and every c_i) 8.9e-14 for both
    aggregates (J alone 2.1e-14 / 7.4e-15), gradient 4.5e-14 / 5.6e-14 of the largest entry (sum / pnorm).  The recorded figures the
    GPU bounds are ten times of must be what this computes: not below it, and not more than twice it."""
    values, gradient = zip(*(lc.cg_chain_differences(aggregate) for aggregate in ("sum", "pnorm")))
    print("CG chain block3even: values %.2e / %.2e, gradient %.2e / %.2e (recorded %.1e, %.1e)"
          % (*values, *gradient, lc.CG_VALUE_MEASURED, lc.CG_GRADIENT_MEASURED))
    assert max(values) <= lc.CG_VALUE_MEASURED <= 2.0 * max(values)
    assert max(gradient) <= lc.CG_GRADIENT_MEASURED <= 2.0 * max(gradient)


def test_the_patterns_by_quadrature_are_the_closed_forms():
    """int N g = vol / 2^N g at every node; int B^T sigma* = sum_q sigma*[a][q] s_nq vol / (2^(N-1) h_q)"""
    for h, N in (((0.5, 0.3), 2), ((0.5, 0.3, 0.7), 3)):
        rng = np.random.default_rng(N)
        g = rng.standard_normal(N)
        vol = float(np.prod(h))
        assert np.allclose(lc.body_pattern(h, g), np.tile(vol / 2 ** N * g, 2 ** N), rtol=1e-14, atol=0)
        A = rng.standard_normal((3 if N == 2 else 6,) * 2)
        D = hc.isotropic_D(1.3, 0.3, N) + 0.05 * (A + A.T)
        eps = rng.standard_normal((N, N))
        eps = eps + eps.T
        flat = lc.eigenstress(D, eps)
        sigma = np.zeros((N, N))
        for r, (i, j) in enumerate(hc.PAIRS[N]):
            sigma[i, j] = sigma[j, i] = flat[r]
        want = np.concatenate([sigma @ (np.array([1.0 if l[q] else -1.0 for q in range(N)]) * vol / (2.0 ** (N - 1) * np.array(h)))
                               for l in np.ndindex(*([2] * N))])
        assert np.allclose(lc.eigenstrain_pattern(D, h, eps), want, rtol=1e-13, atol=1e-15 * np.abs(want).max())


def test_self_weight_sums_to_the_weight_and_its_gradient_has_both_signs():
    p = lc.problem("arch2_weight")
    r = lc.reference("arch2_weight")
    f = lc.kernel_assemble(p["ne"], r["Lb"][0], None, r["m"], r["E"])                     # unmasked
    total, want = f.reshape(-1, 2).sum(axis=0), -float(r["m"].sum()) * float(np.prod(p["h"]))
    print("self-weight: sum f = %s, g sum m vol = %.15e" % (total, want))
    assert total[0] == 0.0 and abs(total[1] - want) < 1e-14 * abs(want)
    long = lc.kernel_assemble(p["ne"], r["Lb"][0], None, r["m"], r["E"], dtype=np.longdouble)
    assert np.abs(long - f).max() < 1e-15 * np.abs(f).max()
    g = r["gradient"]
    print("arch under its own weight: %d positive and %d negative entries, smallest |g| %.2e of the largest"
          % ((g > 0).sum(), (g < 0).sum(), np.abs(g).min() / np.abs(g).max()))
    assert ((g > 0).sum(), (g < 0).sum()) == ARCH_SIGNS
    # with the fixed loads alone the gradient is nowhere positive
    assert (lc.reference("arch2_traffic")["gradient"] <= 0).all()


def test_aggregates():
    p = lc.problem("arch2")
    for case in p["cases"]:
        one = lc.evaluate(dict(p, cases=[dict(case, w=1.0)]))
        for k in (2, 5):
            shared = lc.evaluate(dict(p, cases=[dict(case, w=1.0 / k)] * k))
            assert abs(shared["J"] - one["J"]) < 1e-14 * one["J"]
            assert np.abs(shared["gradient"] - one["gradient"]).max() < 1e-13 * np.abs(one["gradient"]).max()
            copies = lc.evaluate(dict(p, cases=[dict(case, w=1.0)] * k), aggregate="pnorm")
            assert abs(copies["J"] - k ** (1.0 / lc.P_NORM) * one["J"]) < 1e-14 * one["J"]
    s, n1 = lc.evaluate(p), lc.evaluate(p, aggregate="pnorm", P=1.0)
    assert abs(s["J"] - n1["J"]) < 1e-15 * s["J"] and np.abs(s["gradient"] - n1["gradient"]).max() < 1e-14 * np.abs(s["gradient"]).max()
    # the p-norm is a smooth upper bound of the worst weighted case
    worst = float((s["w"] * s["c"]).max())
    J8 = lc.evaluate(p, aggregate="pnorm")["J"]
    assert worst <= J8 <= 3 ** (1.0 / lc.P_NORM) * worst
    assert lc.aggregate_value(np.zeros(3), np.ones(3), "pnorm") [0] == 0.0


def test_extended_precision_variants_agree_with_float64():
    """the longdouble forms the GPU tests use as their reference are the float64 forms to rounding"""
    ne = (7, 5)
    rng = np.random.default_rng(11)
    nel, nd = 35, sc.num_nodes(ne) * 2
    Lb, Lt = rng.standard_normal((2, 8)), rng.standard_normal((2, 8))
    m, E, dm = rng.uniform(0.1, 1, nel), rng.uniform(0.1, 1, nel), rng.uniform(0.1, 1, nel)
    U = rng.standard_normal((2, nd))
    K0 = hc.element_constants(hc.isotropic_D(1.0, 0.3, 2), (0.5, 0.3))[0]
    a64 = lc.kernel_assemble(ne, Lb[0], Lt[0], m, E, None, U[0])
    a80 = lc.kernel_assemble(ne, Lb[0], Lt[0], m, E, None, U[0], dtype=np.longdouble)
    assert a80.dtype == np.longdouble and np.abs(a80 - a64).max() < 1e-15 * np.abs(a64).max()
    args = (ne, K0, Lb, Lt, E, dm, U, rng.standard_normal(2), rng.standard_normal(2), rng.standard_normal(2))
    g64, g80 = lc.kernel_gradient(*args), lc.kernel_gradient(*args, dtype=np.longdouble)
    assert g80.dtype == np.longdouble and np.abs(g80 - g64).max() < 1e-14 * np.abs(g64).max()


# ---- the C boundary: refusals that come before any device call (they run without a GPU) ----

def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _head(ne, h):
    n, hh = np.asarray(ne, dtype=np.int64), np.ascontiguousarray(h, dtype=np.float64)
    return (len(ne), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(hh)), (n, hh)


def test_assemble_refuses_bad_arguments_before_any_device_call():
    """status 1 and a message; the device pointers are addresses nobody dereferences"""
    from ndr_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vfem_last_error().decode()
    args, keep = _head((7, 5), (0.5, 0.3))
    L = np.ones(8)
    P = lambda a: ctypes.c_void_p(a)
    m, E, mask, fin, fout = P(0x100000), P(0x200000), P(0x300000), P(0x400000), P(0x500000)
    call = lambda *t: lib.vfem_loads_assemble(*t, None)
    assert call(*args, _dp(L), _dp(L), m, E, mask, fin, None) == 1 and "null" in err()
    assert call(*args, None, None, None, None, mask, fin, fout) == 1 and "neither" in err()
    assert call(*args, _dp(L), None, None, None, mask, fin, fout) == 1 and "go together" in err()
    assert call(*args, None, _dp(L), None, None, mask, fin, fout) == 1 and "go together" in err()
    assert call(*args, None, _dp(L), m, E, mask, fin, fout) == 1 and "go together" in err()
    assert call(4, *args[1:], _dp(L), _dp(L), m, E, mask, fin, fout) == 1 and "dim" in err()
    assert call(2, None, args[2], _dp(L), _dp(L), m, E, mask, fin, fout) == 1 and "null" in err()
    bad, keep2 = _head((7, 0), (0.5, 0.3))
    assert call(*bad, _dp(L), _dp(L), m, E, mask, fin, fout) == 1 and "extent" in err()
    for hbad in ((0.5, 0.0), (0.5, -1.0), (np.inf, 0.3)):
        bad, keep3 = _head((7, 5), hbad)
        assert call(*bad, _dp(L), _dp(L), m, E, mask, fin, fout) == 1 and "edge lengths" in err()
    for v in (np.nan, np.inf):
        Lbad = L.copy()
        Lbad[3] = v
        assert call(*args, _dp(Lbad), _dp(L), m, E, mask, fin, fout) == 1 and "body-force pattern is not finite" in err()
        assert call(*args, _dp(L), _dp(Lbad), m, E, mask, fin, fout) == 1 and "eigenstrain pattern is not finite" in err()
    # overlaps: f_out is 48 nodes x 2 doubles = 768 bytes
    assert call(*args, _dp(L), _dp(L), m, E, mask, P(0x500008), fout) == 1 and "overlaps f_in" in err()
    assert call(*args, _dp(L), _dp(L), P(0x500100), E, mask, fin, fout) == 1 and "aliases the multipliers" in err()
    assert call(*args, _dp(L), _dp(L), m, P(0x500000 - 8), mask, fin, fout) == 1 and "aliases the multipliers" in err()
    assert call(*args, _dp(L), _dp(L), m, E, P(0x500000 + 767), fin, fout) == 1 and "aliases the mask" in err()


def test_gradient_refuses_bad_arguments_before_any_device_call():
    from ndr_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vfem_last_error().decode()
    args, keep = _head((6, 4, 5), (0.5, 0.3, 0.7))
    K0, co, L = np.eye(24), np.ones(8), np.ones((8, 24))
    P = lambda a: ctypes.c_void_p(a)
    dE, dm, U, g = P(0x100000), P(0x200000), P(0x300000), P(0x800000)
    call = lambda *t: lib.vfem_loads_gradient(*t, None)
    full = lambda **kw: [kw.get(k, d) for k, d in (("K0", _dp(K0)), ("cK", _dp(co)), ("cB", _dp(co)), ("cT", _dp(co)), ("Lb", _dp(L)),
                                                    ("Lt", _dp(L)), ("dE", dE), ("dm", dm), ("U", U), ("g", g))]
    for n in (0, 9, -1):
        assert call(*args, n, *full()) == 1 and "ncases must be 1 to 8" in err()
    for name in ("K0", "cK", "dE", "U", "g"):
        assert call(*args, 3, *full(**{name: None})) == 1 and "null" in err()
    for name in ("cB", "Lb", "dm"):
        assert call(*args, 3, *full(**{name: None})) == 1 and "body-force patterns, their coefficients and dm go together" in err()
    for name in ("cT", "Lt"):
        assert call(*args, 3, *full(**{name: None})) == 1 and "eigenstrain patterns and their coefficients go together" in err()
    assert call(5, *args[1:], 3, *full()) == 1 and "dim" in err()
    bad, keep2 = _head((6, 0, 5), (0.5, 0.3, 0.7))
    assert call(*bad, 3, *full()) == 1 and "extent" in err()
    bad, keep3 = _head((6, 4, 5), (0.5, 0.3, 0.0))
    assert call(*bad, 3, *full()) == 1 and "edge lengths" in err()
    nan = lambda a, i: (lambda b: (b.__setitem__(i, np.nan), b)[1])(a.copy())
    assert call(*args, 3, *full(K0=_dp(nan(K0, (2, 3))))) == 1 and "element matrix is not finite" in err()
    for name in ("cK", "cB", "cT"):
        bad_co = nan(co, 2)
        assert call(*args, 3, *full(**{name: _dp(bad_co)})) == 1 and "coefficients are not finite" in err()
    assert call(*args, 3, *full(Lb=_dp(nan(L, (2, 5))))) == 1 and "body-force patterns are not finite" in err()
    assert call(*args, 3, *full(Lt=_dp(nan(L, (0, 0))))) == 1 and "eigenstrain patterns are not finite" in err()
    # overlaps: g is 120 doubles = 960 bytes
    assert call(*args, 3, *full(dE=P(0x800000 + 952))) == 1 and "aliases an input" in err()
    assert call(*args, 3, *full(dm=P(0x800000 - 8))) == 1 and "aliases an input" in err()
    assert call(*args, 3, *full(U=P(0x800000 - 3 * 7 * 5 * 6 * 3 * 8 + 8))) == 1 and "aliases an input" in err()
