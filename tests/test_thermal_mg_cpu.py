"""CPU: the restatement of the scalar multigrid (tests/thermal_mg_cpu.py) against dense algebra, the iteration counts the GPU tests of
tests/test_gpu_thermal_mg.py are bounded by (recomputed here and pinned), and the refusals of the ``vfem_thermal_mg_*`` entry points
that need no handle and so come before any device call."""
import ctypes

import numpy as np
import pytest

import thermal_cpu as tc
import thermal_mg_cpu as mg


def _name(ne):
    return "x".join(map(str, ne))


# ---- the restatement against dense algebra ----

@pytest.mark.parametrize("ne", [(16, 12), (12, 8, 16), (4, 4)], ids=_name)
@pytest.mark.parametrize("mask", ["sink", "random"])
def test_levels_are_galerkin_products_and_positive_definite(ne, mask):
    """A'_{l+1} = P_l^T A'_l P_l formed densely; every A_l symmetric positive definite with 20 % random fixed nodes (and with the sink)
    and the anisotropic conductivity; a coarse node is fixed exactly when its fine node is"""
    c = mg.case(ne, mask)
    H = mg.case_hierarchy(ne, mask)
    assert H.ne == mg.level_extents(ne) and len(H.ne) == (2 if ne == (4, 4) else 3)
    A0 = tc.assemble(ne, c["Kc0"], c["kap"], c["fixed"])
    assert np.abs(H.A[0].dense() - A0).max() < 1e-14 * np.abs(A0).max()
    idx = mg.node_index_grid(ne)
    for l in range(1, len(H.ne)):
        P, Af = H.P[l - 1].dense(), H.Ap[l - 1].dense()
        want = P.T @ Af @ P
        assert np.abs(H.Ap[l].dense() - want).max() < 1e-14 * np.abs(want).max()
        # rows at fixed fine nodes and columns at fixed coarse nodes of P are zero; a free coarse node has weight 1 on its own fine node
        assert not P[H.fixed[l - 1]].any() and not P[:, H.fixed[l]].any()
        fine_of = np.ravel_multi_index(tuple((2 * mg.node_index_grid(H.ne[l])).T), tuple(n + 1 for n in H.ne[l - 1]))
        assert np.array_equal(H.fixed[l], H.fixed[l - 1][fine_of])
        free = np.flatnonzero(~H.fixed[l])
        assert np.all(P[fine_of[free], free] == 1.0)
        # the interpolation reproduces a linear field on the free interior
        if mask == "sink" and l == 1:
            I = mg.interpolation(ne).dense()
            lin_f, lin_c = idx @ np.arange(1.0, len(ne) + 1), 2.0 * mg.node_index_grid(H.ne[1]) @ np.arange(1.0, len(ne) + 1)
            assert np.abs(I @ lin_c - lin_f).max() < 1e-12
    for l, A in enumerate(H.A):
        D = A.dense()
        assert np.abs(D - D.T).max() < 1e-14 * np.abs(D).max()
        assert np.linalg.eigvalsh(0.5 * (D + D.T)).min() > 0.0
        assert np.all(np.diag(D)[H.fixed[l]] == 1.0)
    # the coordinate-form triple product of the longdouble hierarchy agrees with scipy's
    HL = mg.case_hierarchy(ne, mask, long=True)
    for l in range(len(H.ne)):
        assert np.abs(HL.A[l].dense() - H.A[l].dense()).max() < 1e-14 * np.abs(H.A[l].dense()).max()


def _cycle_matrix(H, smoothing):
    n = H.A[0].shape[0]
    return np.stack([H.vcycle(e, smoothing) for e in np.eye(n)], axis=1)


@pytest.mark.parametrize("smoothing", [1, 2])
def test_vcycle_is_symmetric_positive_definite(smoothing):
    H = mg.case_hierarchy((16, 12), "random")
    M = _cycle_matrix(H, smoothing)
    asym = np.abs(M - M.T).max() / np.abs(M).max()
    low = np.linalg.eigvalsh(0.5 * (M + M.T)).min()
    print("V-cycle matrix 16x12, smoothing %d: asymmetry %.1e, smallest eigenvalue %.3e" % (smoothing, asym, low))
    assert asym < 1e-13 and low > 0.0
    # a preconditioner: the spectrum of M A lies in (0, 1]
    ev = np.linalg.eigvals(M @ H.A[0].dense()).real
    assert ev.min() > 0.0 and ev.max() < 1.0 + 1e-10


@pytest.mark.parametrize("ne", [(7, 5), (2, 2)], ids=_name)
def test_one_level_cycle_is_the_exact_inverse(ne):
    c = mg.case(ne, "random")
    H = mg.case_hierarchy(ne, "random")
    assert H.ne == [ne]
    A = tc.assemble(ne, c["Kc0"], c["kap"], c["fixed"])
    x = H.vcycle(c["B"], 1)
    assert np.abs(A @ x - c["B"]).max() < 1e-12 * np.abs(c["B"]).max()
    assert np.array_equal(x[c["fixed"]], c["B"][c["fixed"]])


def test_level_rule():
    assert mg.level_extents((16, 12)) == [(16, 12), (8, 6), (4, 3)]
    assert mg.level_extents((12, 8, 16)) == [(12, 8, 16), (6, 4, 8), (3, 2, 4)]
    assert mg.level_extents((4, 4, 136)) == [(4, 4, 136), (2, 2, 68)]
    assert mg.level_extents((4, 4)) == [(4, 4), (2, 2)] and mg.level_extents((7, 5)) == [(7, 5)] and mg.level_extents((2, 2)) == [(2, 2)]
    assert mg.level_extents((96, 96, 96), 0) == [(96, 96, 96)] and mg.level_extents((16, 12), 1) == [(16, 12), (8, 6)]


# ---- the pinned counts ----

def test_pcg_data_is_the_fixture():
    f, d = tc.pcg_fixture((40, 36)), mg.pcg_data((40, 36))
    assert all(np.array_equal(f[k], d[k]) for k in ("rho", "fixed", "Kc0", "Q"))
    assert np.abs(mg.pcg_hierarchy((40, 36)).A[0].dense() - f["A"]).max() < 1e-15


@pytest.mark.parametrize("smoothing", [1, 2])
@pytest.mark.parametrize("ne", mg.PCG_SHAPES, ids=_name)
def test_pinned_iteration_counts(ne, smoothing):
    x, info = mg.pcg_solution(ne, smoothing)
    print("multigrid-PCG %s, smoothing %d: %d iterations, |r|/|b| %.3e, true %.3e, gap %.1e" %
          (_name(ne), smoothing, info["iterations"], info["relres"], info["true_relres"], info["gap"]))
    assert info["converged"] and info["iterations"] == mg.PCG_COUNT[smoothing][ne]
    assert info["true_relres"] < 1e-8 + 1e-12


@pytest.mark.parametrize("ne", list(mg.GROWTH_COUNT), ids=_name)
def test_pinned_growth_counts(ne):
    """the count grows by a few iterations while the grid grows 16 times (2-D) and 8 times (3-D); Jacobi-PCG doubles with the extent"""
    x, info = mg.pcg_solution(ne, 1)
    print("multigrid-PCG %s: %d iterations" % (_name(ne), info["iterations"]))
    assert info["converged"] and info["iterations"] == mg.GROWTH_COUNT[ne]


def test_jacobi_needs_many_more():
    f = tc.pcg_fixture((40, 36))
    jac = tc.pcg(f["A"], f["Q"], tol=1e-8)[1]
    assert jac["crossing"] > 8 * mg.PCG_COUNT[1][(40, 36)]


# ---- the C boundary: refusals that need no handle (they run without a GPU) ----

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


def test_create_refuses_bad_arguments_before_any_device_call():
    lib, err = _lib_err()
    args, keep = _head((7, 5))
    K = np.eye(4)
    kappa, fixed = P(0x100000), P(0x200000)
    h = ctypes.c_void_p()
    call = lambda *t: lib.vfem_thermal_mg_create(*t, None)
    assert call(None, *args, _dp(K), kappa, fixed, -1) == 1 and "null" in err()
    assert call(ctypes.byref(h), *args, None, kappa, fixed, -1) == 1 and "null" in err()
    assert call(ctypes.byref(h), *args, _dp(K), None, fixed, -1) == 1 and "null" in err()
    assert call(ctypes.byref(h), 2, None, _dp(K), kappa, fixed, -1) == 1 and "null" in err()
    assert call(ctypes.byref(h), 4, args[1], _dp(K), kappa, fixed, -1) == 1 and "dim" in err()
    bad, keep2 = _head((7, 0))
    assert call(ctypes.byref(h), *bad, _dp(K), kappa, fixed, -1) == 1 and "extent" in err()
    Kn = K.copy()
    Kn[1, 2] = np.inf
    assert call(ctypes.byref(h), *args, _dp(Kn), kappa, fixed, -1) == 1 and "element matrix is not finite" in err()
    assert not h.value
    # a coarsest level above the dense solver's limit is refused with the level sizes and the rule, before anything is allocated
    big, keep3 = _head((96, 96, 96))
    assert call(ctypes.byref(h), *big, _dp(np.eye(8)), kappa, fixed, 0) == 1
    assert "96x96x96 has 912673 nodes, above the limit of 40000" in err() and "even and at least 4" in err()
    assert call(ctypes.byref(h), *big, _dp(np.eye(8)), kappa, fixed, 1) == 1
    assert "96x96x96, 48x48x48 has 117649 nodes" in err()
    odd, keep4 = _head((399, 399))
    assert call(ctypes.byref(h), *odd, _dp(K), kappa, fixed, -1) == 1 and "399x399 has 160000 nodes" in err()
    assert not h.value


def test_entry_points_refuse_a_null_handle_and_bad_arguments_before_any_device_call():
    lib, err = _lib_err()
    X, B = P(0x300000), P(0x500000)
    n = (ctypes.c_int64 * 3)()
    assert lib.vfem_thermal_mg_num_levels(None) == 0 and lib.vfem_thermal_mg_bytes(None) == 0
    assert lib.vfem_thermal_mg_destroy(None) == 0
    assert lib.vfem_thermal_mg_level_dims(None, 0, n) == 1 and "null handle" in err()
    assert lib.vfem_thermal_mg_level_fixed(None, 0, X, None) == 1 and "null handle" in err()
    for f in (lib.vfem_thermal_mg_level_apply, lib.vfem_thermal_mg_restrict, lib.vfem_thermal_mg_prolong_add):
        assert f(None, 0, X, B, None) == 1 and "null handle" in err()
        assert f(None, 0, None, B, None) == 1 and "null argument" in err()
        assert f(None, 0, X, None, None) == 1 and "null argument" in err()
    assert lib.vfem_thermal_mg_smooth(None, 0, X, B, 1, None) == 1 and "null handle" in err()
    assert lib.vfem_thermal_mg_smooth(None, 0, None, B, 1, None) == 1 and "null argument" in err()
    assert lib.vfem_thermal_mg_vcycle(None, B, X, 1, None) == 1 and "null handle" in err()
    assert lib.vfem_thermal_mg_vcycle(None, None, X, 1, None) == 1 and "null argument" in err()
    for s in (0, 17, -1):
        assert lib.vfem_thermal_mg_vcycle(None, B, X, s, None) == 1 and "smoothing must be in [1, 16]" in err()
    it, rel = ctypes.c_int(0), ctypes.c_double(0.0)
    pcg = lambda b=B, x=X, tol=1e-8, mx=10, s=1, i=ctypes.byref(it), r=ctypes.byref(rel): lib.vfem_thermal_mg_pcg(None, b, x, tol, mx, s, i, r, None)
    assert pcg() == 1 and "null handle" in err()
    for kw in (dict(b=None), dict(x=None), dict(i=None), dict(r=None)):
        assert pcg(**kw) == 1 and "null argument" in err()
    for kw in (dict(tol=0.0), dict(tol=-1e-8), dict(tol=float("nan")), dict(tol=float("inf")), dict(mx=0)):
        assert pcg(**kw) == 1 and "tol must be positive and max_iter at least 1" in err()
    for s in (0, 17):
        assert pcg(s=s) == 1 and "smoothing must be in [1, 16]" in err()
