"""CPU: the dense restatement of heat conduction (tests/thermal_cpu.py) against closed forms and finite differences, the figures the GPU
bounds of tests/test_gpu_thermal.py are derived from (printed, and pinned where thermal_cpu stores them), and the refusals of the
``vfem_thermal_*`` entry points that come before any device call."""
import ctypes

import numpy as np
import pytest

import thermal_cpu as tc


def _fd(fun, rho, g, step=1e-5, n=12, seed=0):
    """the largest difference between central differences and g over n random elements, relative to the largest entry of g"""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for e in rng.choice(rho.size, size=n, replace=False):
        rp, rm = rho.copy(), rho.copy()
        rp[e] += step
        rm[e] -= step
        worst = max(worst, abs((fun(rp) - fun(rm)) / (2 * step) - g[e]))
    return worst / np.abs(g).max()


@pytest.mark.parametrize("N", [2, 3])
def test_element_matrix_is_symmetric_with_zero_row_sums(N):
    K = tc.conductivity_matrix(tc.K_ANISO[N], tc.EDGES[N])
    print("Kc0 %d-D: row sums %.1e, asymmetry %.1e of %.3f" % (N, np.abs(K.sum(1)).max(), np.abs(K - K.T).max(), np.abs(K).max()))
    assert np.abs(K.sum(axis=1)).max() < 1e-15 * np.abs(K).max() * 2 ** N
    assert np.abs(K - K.T).max() < 1e-15 * np.abs(K).max()
    assert np.linalg.eigvalsh(K)[1] > 0.0                          # one zero eigenvalue (the constant field), the rest positive
    # an isotropic scalar against the closed form of the unit square: 1/6 [[4, -1, -1, -2], ...]
    if N == 2:
        K1 = tc.conductivity_matrix(1.0, (1.0, 1.0))
        assert np.allclose(K1, np.array([[4, -1, -1, -2], [-1, 4, -2, -1], [-1, -2, 4, -1], [-2, -1, -1, 4]]) / 6.0, atol=1e-15)


def test_the_product_forms_the_same_element_matrix():
    """ndr_amd.thermal.conductivityMatrix is what the device gets; it is written separately from the restatement's"""
    pytest.importorskip("torch")
    from ndr_amd.thermal import conductivityMatrix
    for N in (2, 3):
        a, b = conductivityMatrix(tc.K_ANISO[N], tc.EDGES[N]), tc.conductivity_matrix(tc.K_ANISO[N], tc.EDGES[N])
        assert np.abs(a - b).max() < 4e-16 * np.abs(b).max()


@pytest.mark.parametrize("ne,w", [((16, 6), 8), ((6, 4, 3), 25), ((7, 5), 7), ((40, 37), 39), ((5, 70), 72), ((12, 10, 9), 121)])
def test_half_bandwidth_is_the_sum_of_the_node_strides(ne, w):
    assert tc.band_width(ne) == w
    f = tc.direct_fixture(ne) if tc.num_nodes(ne) < 200 else None
    if f is not None:
        A = tc.assemble(ne, tc.conductivity_matrix(f["k"], f["h"]), tc.kappa(f["rho"]), None)
        i, j = np.nonzero(A)
        assert np.abs(i - j).max() == w


@pytest.mark.parametrize("ne", tc.SLAB_SHAPES, ids=str)
def test_slab_and_layers_reproduce_their_closed_forms(ne):
    T, exact, J = tc.slab_case(ne)
    slab = np.abs(T - exact).max() / np.abs(exact).max()
    far, value = tc.layers_case(ne)
    layers = np.abs(far - value).max() / value
    print("%s: slab %.2e (stored %.1e, device bound %.1e), layers %.2e (stored %.1e, device bound %.1e)"
          % (ne, slab, tc.SLAB_MEASURED[ne], tc.analytic_bound(tc.SLAB_MEASURED[ne], ne), layers, tc.LAYERS_MEASURED[ne],
             tc.analytic_bound(tc.LAYERS_MEASURED[ne], ne)))
    for measured, stored in ((slab, tc.SLAB_MEASURED[ne]), (layers, tc.LAYERS_MEASURED[ne])):
        assert measured <= stored <= 3.0 * measured + 1e-15


@pytest.mark.parametrize("ne", [(16, 6), (8, 4, 3)], ids=str)
def test_compliance_gradient_matches_central_differences(ne):
    f = tc.direct_fixture(ne)
    args = (f["fixed"], f["nodal"], f["volumetric"])
    J, T, g, Q = tc.compliance(ne, f["h"], f["k"], f["rho"], *args)
    err = _fd(lambda r: tc.compliance(ne, f["h"], f["k"], r, *args)[0], f["rho"], g)
    print("%s: compliance gradient against central differences %.2e; largest entry %.3e" % (ne, err, g.max()))
    assert err < 1e-7
    assert g.max() <= 0.0                                           # nowhere positive: the OC step applies


def test_peak_temperature_gradient_matches_central_differences():
    ne = (8, 5)
    f = tc.direct_fixture(ne)
    args = (f["fixed"], 8.0, f["nodal"], f["volumetric"])
    J, T, g, lam = tc.pnorm_temperature(ne, f["h"], f["k"], f["rho"], *args)
    err = _fd(lambda r: tc.pnorm_temperature(ne, f["h"], f["k"], r, *args)[0], f["rho"], g)
    print("8 x 5, P = 8, anisotropic k: gradient against central differences %.2e; J_P %.6g, max |T| %.6g" % (err, J, np.abs(T).max()))
    assert err < 1e-7
    assert np.abs(T).max() <= J <= tc.num_nodes(ne) ** (1.0 / 8.0) * np.abs(T).max()


@pytest.mark.parametrize("ne", tc.PCG_SHAPES, ids=str)
def test_pcg_counts_gaps_and_solutions_of_the_gpu_fixtures(ne):
    f = tc.pcg_fixture(ne)
    x, info = tc.pcg(f["A"], f["Q"], tol=1e-8)
    T = tc.solve(f["A"], f["Q"])
    sol = np.abs(x - T).max() / np.abs(T).max()
    print("%s: crossing %d, stopped at %d, |r|/|b| %.3e (true %.3e, gap %.2e), solution %.2e of max |T|; device bound %d iterations"
          % (ne, info["crossing"], info["iterations"], info["relres"], info["true_relres"], info["gap"], sol, tc.pcg_iteration_bound(ne)))
    assert info["converged"] and info["crossing"] == tc.PCG_CROSSING[ne]
    assert info["iterations"] == (info["crossing"] + tc.CHECK - 1) // tc.CHECK * tc.CHECK < 2000
    assert info["gap"] <= tc.PCG_GAP_MEASURED
    assert sol <= tc.PCG_SOLUTION_MEASURED[ne] <= 3.0 * sol
    # a second solve from the solution stops before its first iteration
    assert tc.pcg(f["A"], f["Q"], x0=x, tol=1e-8)[1]["iterations"] == 0


def test_the_largest_gap_is_the_stored_one():
    gaps = [tc.pcg(f["A"], f["Q"], tol=1e-8)[1]["gap"] for f in map(tc.pcg_fixture, tc.PCG_SHAPES)]
    print("recurrence-to-true gaps %s, stored %.1e" % (" ".join("%.2e" % g for g in gaps), tc.PCG_GAP_MEASURED))
    assert max(gaps) <= tc.PCG_GAP_MEASURED <= 3.0 * max(gaps)


def test_extended_precision_variants_agree_with_float64():
    ne = (6, 4, 5)
    rng = np.random.default_rng(7)
    nn, nel = tc.num_nodes(ne), tc.num_elements(ne)
    Kc0, kap = tc.conductivity_matrix(tc.K_ANISO[3], tc.EDGES[3]), rng.uniform(0.05, 1.0, size=nel)
    fixed, X = rng.uniform(size=nn) < 0.2, rng.standard_normal((3, nn))
    L = np.longdouble
    pairs = [(tc.apply(ne, Kc0, kap, fixed, X), tc.apply(ne, Kc0, kap, fixed, X, dtype=L)),
             (tc.diagonal(ne, Kc0, kap, fixed), tc.diagonal(ne, Kc0, kap, fixed, dtype=L)),
             (tc.source(ne, tc.EDGES[3], kap, fixed, X[0]), tc.source(ne, tc.EDGES[3], kap, fixed, X[0], dtype=L)),
             (tc.gradient(ne, Kc0, kap, [0.3, -1.0, 2.0], X, X[::-1]), tc.gradient(ne, Kc0, kap, [0.3, -1.0, 2.0], X, X[::-1], dtype=L)),
             (tc.flux(ne, tc.EDGES[3], tc.K_ANISO[3], kap, X[0]), tc.flux(ne, tc.EDGES[3], tc.K_ANISO[3], kap, X[0], dtype=L))]
    for a64, a80 in pairs:
        assert a64.dtype == np.float64 and a80.dtype == np.longdouble
        assert np.abs(a80 - a64).max() < 1e-14 * np.abs(a64).max()
    # and the element-wise apply is the dense operator
    A = tc.assemble(ne, Kc0, kap, fixed)
    assert np.abs(pairs[0][0] - X @ A.T).max() < 1e-13 * np.abs(X @ A.T).max()
    assert np.abs(pairs[1][0] - np.diag(A)).max() < 1e-14 * np.diag(A).max()


# ---- the C boundary: refusals that come before any device call (they run without a GPU) ----

def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _head(ne):
    n = np.asarray(ne, dtype=np.int64)
    return (len(ne), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), n


P = ctypes.c_void_p


def _lib_err():
    from ndr_amd import _lib
    lib = _lib.load()
    return lib, lambda: lib.vfem_last_error().decode()


def _nan(a, i):
    b = a.copy()
    b[i] = np.nan
    return b


def test_apply_and_diagonal_refuse_bad_arguments_before_any_device_call():
    """status 1 and a message; the device pointers are addresses nobody dereferences"""
    lib, err = _lib_err()
    args, keep = _head((7, 5))
    K = np.eye(4)
    kappa, fixed, X, Y = P(0x100000), P(0x200000), P(0x300000), P(0x500000)
    call = lambda *t: lib.vfem_thermal_apply(*t, None)
    assert call(*args, _dp(K), kappa, fixed, 1, X, None) == 1 and "null" in err()
    assert call(*args, _dp(K), None, fixed, 1, X, Y) == 1 and "null" in err()
    assert call(*args, _dp(K), kappa, fixed, 1, None, Y) == 1 and "null" in err()
    assert call(*args, None, kappa, fixed, 1, X, Y) == 1 and "null" in err()
    assert call(2, None, _dp(K), kappa, fixed, 1, X, Y) == 1 and "null" in err()
    assert call(4, args[1], _dp(K), kappa, fixed, 1, X, Y) == 1 and "dim" in err()
    bad, keep2 = _head((7, 0))
    assert call(*bad, _dp(K), kappa, fixed, 1, X, Y) == 1 and "extent" in err()
    for v in (np.nan, np.inf):
        Kb = K.copy()
        Kb[1, 2] = v
        assert call(*args, _dp(Kb), kappa, fixed, 1, X, Y) == 1 and "element matrix is not finite" in err()
    for n in (0, 9, -1):
        assert call(*args, _dp(K), kappa, fixed, n, X, Y) == 1 and "ncols must be 1 to 8" in err()
    # overlaps: one column is 48 nodes = 384 bytes, the multipliers 35 x 8 = 280 bytes
    assert call(*args, _dp(K), kappa, fixed, 2, P(0x500000 + 760), Y) == 1 and "Y aliases X" in err()
    assert call(*args, _dp(K), P(0x500000 - 272), fixed, 1, X, Y) == 1 and "aliases the element multipliers" in err()
    assert call(*args, _dp(K), kappa, P(0x500000 + 383), 1, X, Y) == 1 and "aliases the fixed-node mask" in err()

    call = lambda *t: lib.vfem_thermal_diagonal(*t, None)
    assert call(*args, _dp(K), kappa, fixed, None) == 1 and "null" in err()
    assert call(*args, _dp(K), None, fixed, Y) == 1 and "null" in err()
    assert call(*args, None, kappa, fixed, Y) == 1 and "null" in err()
    assert call(1, args[1], _dp(K), kappa, fixed, Y) == 1 and "dim" in err()
    assert call(*bad, _dp(K), kappa, fixed, Y) == 1 and "extent" in err()
    assert call(*args, _dp(_nan(K, (0, 0))), kappa, fixed, Y) == 1 and "element matrix is not finite" in err()
    assert call(*args, _dp(K), P(0x500000 + 376), fixed, Y) == 1 and "aliases the element multipliers" in err()
    assert call(*args, _dp(K), kappa, P(0x500000 - 47), Y) == 1 and "aliases the fixed-node mask" in err()


def test_source_and_flux_refuse_bad_arguments_before_any_device_call():
    lib, err = _lib_err()
    args, keep = _head((6, 4, 5))
    h, k = np.array([0.5, 0.3, 0.7]), np.eye(3)
    q, fixed, fin, fout = P(0x100000), P(0x200000), P(0x300000), P(0x500000)
    call = lambda *t: lib.vfem_thermal_source(*t, None)
    assert call(*args, _dp(h), q, fixed, fin, None) == 1 and "null" in err()
    assert call(*args, None, q, fixed, fin, fout) == 1 and "null" in err()
    assert call(*args, _dp(h), None, fixed, None, fout) == 1 and "neither" in err()
    assert call(5, args[1], _dp(h), q, fixed, fin, fout) == 1 and "dim" in err()
    bad, keep2 = _head((6, 0, 5))
    assert call(*bad, _dp(h), q, fixed, fin, fout) == 1 and "extent" in err()
    for hb in ((0.5, 0.0, 0.7), (0.5, -1.0, 0.7), (np.inf, 0.3, 0.7)):
        assert call(*args, _dp(np.array(hb)), q, fixed, fin, fout) == 1 and "edge lengths" in err()
    # f_out is 7 x 5 x 6 = 210 nodes = 1680 bytes
    assert call(*args, _dp(h), q, fixed, P(0x500008), fout) == 1 and "overlaps f_in" in err()
    assert call(*args, _dp(h), P(0x500000 + 1672), fixed, fin, fout) == 1 and "aliases the element multipliers" in err()
    assert call(*args, _dp(h), q, P(0x500000 - 209), fin, fout) == 1 and "aliases the fixed-node mask" in err()

    kappa, T, flux = P(0x100000), P(0x300000), P(0x800000)
    call = lambda *t: lib.vfem_thermal_flux(*t, None)
    for i in range(2, 7):
        t = [*args, _dp(h), _dp(k), kappa, T, flux]
        t[i] = None
        assert call(*t) == 1 and "null" in err()
    assert call(1, args[1], _dp(h), _dp(k), kappa, T, flux) == 1 and "dim" in err()
    assert call(*bad, _dp(h), _dp(k), kappa, T, flux) == 1 and "extent" in err()
    assert call(*args, _dp(np.array([0.5, 0.3, 0.0])), _dp(k), kappa, T, flux) == 1 and "edge lengths" in err()
    assert call(*args, _dp(h), _dp(_nan(k, (1, 1))), kappa, T, flux) == 1 and "conductivity tensor is not finite" in err()
    # flux is 120 elements x 3 = 2880 bytes
    assert call(*args, _dp(h), _dp(k), kappa, P(0x800000 + 2872), flux) == 1 and "aliases an input" in err()
    assert call(*args, _dp(h), _dp(k), P(0x800000 - 952), T, flux) == 1 and "aliases an input" in err()


def test_band_and_pcg_refuse_bad_arguments_before_any_device_call():
    lib, err = _lib_err()
    args, keep = _head((7, 5))
    K = np.eye(4)
    kappa, fixed, b, x = P(0x100000), P(0x200000), P(0x300000), P(0x500000)
    call = lambda *t: lib.vfem_thermal_band_assemble(*t, None)
    assert call(*args, _dp(K), kappa, fixed, None) == 1 and "null" in err()
    assert call(*args, _dp(K), None, fixed, x) == 1 and "null" in err()
    assert call(*args, None, kappa, fixed, x) == 1 and "null" in err()
    assert call(0, args[1], _dp(K), kappa, fixed, x) == 1 and "dim" in err()
    bad, keep2 = _head((0, 5))
    assert call(*bad, _dp(K), kappa, fixed, x) == 1 and "extent" in err()
    assert call(*args, _dp(_nan(K, (3, 3))), kappa, fixed, x) == 1 and "element matrix is not finite" in err()
    # the band of 48 nodes, w = 7: one tile row of three tiles, 12288 doubles = 98304 bytes
    assert call(*args, _dp(K), P(0x500000 + 98296), fixed, x) == 1 and "aliases the element multipliers" in err()
    assert call(*args, _dp(K), kappa, P(0x500000 + 98303), x) == 1 and "aliases the fixed-node mask" in err()

    it, rel = ctypes.c_int(-1), ctypes.c_double(-1.0)
    call = lambda *t: lib.vfem_thermal_pcg(*t, None)
    full = lambda **kw: [kw.get(n, d) for n, d in (("K", _dp(K)), ("kappa", kappa), ("fixed", fixed), ("b", b), ("x", x), ("tol", 1e-8),
                                                    ("max_iter", 100), ("it", ctypes.byref(it)), ("rel", ctypes.byref(rel)))]
    for name in ("K", "kappa", "b", "x", "it", "rel"):
        assert call(*args, *full(**{name: None})) == 1 and "null" in err()
    assert call(3, None, *full()) == 1 and "null" in err()
    assert call(7, args[1], *full()) == 1 and "dim" in err()
    assert call(*bad, *full()) == 1 and "extent" in err()
    assert call(*args, *full(K=_dp(_nan(K, (0, 1))))) == 1 and "element matrix is not finite" in err()
    for tol in (0.0, -1e-8, np.nan, np.inf):
        assert call(*args, *full(tol=tol)) == 1 and "tol must be positive" in err()
    assert call(*args, *full(max_iter=0)) == 1 and "max_iter at least 1" in err()
    assert call(*args, *full(b=P(0x500000 + 376))) == 1 and "x aliases b" in err()
    assert call(*args, *full(kappa=P(0x500000 - 272))) == 1 and "aliases the element multipliers" in err()
    assert call(*args, *full(fixed=P(0x500000 + 383))) == 1 and "aliases the fixed-node mask" in err()
    assert it.value == -1 and rel.value == -1.0                    # nothing was written by a refused call


def test_gradient_refuses_bad_arguments_before_any_device_call():
    lib, err = _lib_err()
    args, keep = _head((6, 4, 5))
    K, co = np.eye(8), np.ones(8)
    dk, A, B, g = P(0x100000), P(0x300000), P(0x400000), P(0x800000)
    call = lambda *t: lib.vfem_thermal_gradient(*t, None)
    full = lambda **kw: [kw.get(n, d) for n, d in (("K", _dp(K)), ("c", _dp(co)), ("dk", dk), ("A", A), ("B", B), ("g", g))]
    for n in (0, 9, -1):
        assert call(*args, n, *full()) == 1 and "ncols must be 1 to 8" in err()
    for name in ("K", "c", "dk", "A", "B", "g"):
        assert call(*args, 3, *full(**{name: None})) == 1 and "null" in err()
    assert call(5, args[1], 3, *full()) == 1 and "dim" in err()
    bad, keep2 = _head((6, 4, 0))
    assert call(*bad, 3, *full()) == 1 and "extent" in err()
    assert call(*args, 3, *full(K=_dp(_nan(K, (2, 3))))) == 1 and "element matrix is not finite" in err()
    assert call(*args, 3, *full(c=_dp(_nan(co, 2)))) == 1 and "coefficients are not finite" in err()
    # overlaps: g is 120 doubles = 960 bytes; three columns are 3 x 210 x 8 = 5040 bytes
    assert call(*args, 3, *full(dk=P(0x800000 + 952))) == 1 and "aliases an input" in err()
    assert call(*args, 3, *full(A=P(0x800000 - 5032))) == 1 and "aliases an input" in err()
    assert call(*args, 3, *full(B=P(0x800000 + 952))) == 1 and "aliases an input" in err()
