"""The fp64 restatement of the element stresses and the p-norm measure (tests/stress_cpu.py) checked against what is known in
closed form and against finite differences; no GPU.

Measured with the committed restatement (direct solves):
  patch test: 2-D 5 x 3 3.3e-16, 3-D 3 x 2 x 4 7.8e-16 (bound 1e-13); duality vol Bbar^T s against _stress_load: 2.8e-17 / 2.8e-17
  P = 64 on 24 stresses of order 1e6: J / vmax = 1.0182, the naive sum is inf
  central difference of J along one random direction, step 1e-5, gamma = 3, q = 0.5, P = 8, densities in [0.2, 1]:
    6 x 4 cantilever 7.2e-7 relative, 4 x 3 x 3 cantilever 7.6e-10; the bounds are ten times these, not below 1e-7: 7.2e-6 and 1e-7.
    The 6 x 4 figure is the difference quotient's own error, not the gradient's: along this direction the terms g_e d_e cancel from
    292 to 2.86, the mismatch falls with the square of the step down to 2.8e-7 at 1e-6 and Richardson extrapolation leaves 7e-8.
    Entry by entry (no cancellation) the same step gives 3.3e-9 of the largest entry; that bound is 1e-7 (ten times, not below 1e-7)
  the 6 x 4 gradient has entries of both signs (counts are printed)
"""
import numpy as np
import pytest

import homogenization_cpu as hc
import stress_cpu as sc

FD_STEP = 1e-5
FD_MEASURED = {"6x4": 7.2e-7, "4x3x3": 7.6e-10}
TOL_FD_ENTRY = max(10.0 * 3.3e-9, 1e-7)
TOL_FD = {k: max(10.0 * v, 1e-7) for k, v in FD_MEASURED.items()}
SMALL = {"6x4": ((6, 4), (0.5, 0.4), 5), "4x3x3": ((4, 3, 3), (0.5, 0.4, 0.3), 6)}


@pytest.mark.parametrize("ne,h", [((5, 3), (0.5, 0.3)), ((3, 2, 4), (0.5, 0.3, 0.7))])
def test_patch_test_affine_field_gives_its_symmetric_gradient(ne, h):
    N = len(ne)
    A = np.random.default_rng(1).standard_normal((N, N))
    x = np.stack(np.meshgrid(*[np.arange(n + 1) * hh for n, hh in zip(ne, h)], indexing="ij"), -1).reshape(-1, N)
    u = x @ A.T
    eps, _, _ = sc.fields(ne, h, np.eye(len(sc.PAIRS[N])), np.ones(int(np.prod(ne))), u.reshape(-1))
    sym = 0.5 * (A + A.T)
    expect = np.array([sym[i, j] for i, j in sc.PAIRS[N]])
    err = np.abs(eps - expect[None]).max()
    print("patch test %s: %.1e" % ("x".join(map(str, ne)), err))
    assert err < 1e-13


@pytest.mark.parametrize("h", [(0.5, 0.3), (0.5, 0.3, 0.7)])
def test_bbar_transposed_is_the_constant_stress_load(h):
    """vol Bbar^T s (the contraction counts the shear entries twice) is what the package's constant-stress load puts on an element"""
    import torch
    from ndr_amd.pyVoxelFEM import _stress_load
    N = len(h)
    s = np.random.default_rng(2).standard_normal(len(sc.PAIRS[N]))
    sigma = np.zeros((N, N))
    for r, (i, j) in enumerate(sc.PAIRS[N]):
        sigma[i, j] = sigma[j, i] = s[r]
    load = _stress_load(sigma, np.asarray(h), 1, torch.ones((1,) * N, dtype=torch.float64)).numpy().reshape(-1)
    mine = float(np.prod(h)) * sc.bbar(h).T @ (sc.mult(N) * s)
    err = np.abs(mine - load).max()
    print("duality %d-D: %.1e" % (N, err))
    assert err < 1e-14 * np.abs(load).max() + 1e-300 and np.abs(load).max() > 0.1


def test_von_mises_identities():
    assert sc.von_mises(np.array([2.5, 2.5, 2.5, 0.0, 0.0, 0.0])) == 0.0                     # hydrostatic
    for s in (3.0, -3.0):
        assert sc.von_mises(np.array([0.0, s, 0.0, 0.0, 0.0, 0.0])) == pytest.approx(3.0, rel=1e-15)        # uniaxial
        assert sc.von_mises(np.array([s, 0.0, 0.0])) == pytest.approx(3.0, rel=1e-15)
    for t in (0.7, -0.7):
        assert sc.von_mises(np.array([0.0, 0.0, 0.0, 0.0, t, 0.0])) == pytest.approx(np.sqrt(3.0) * 0.7, rel=1e-15)     # pure shear
        assert sc.von_mises(np.array([0.0, 0.0, t])) == pytest.approx(np.sqrt(3.0) * 0.7, rel=1e-15)


def test_von_mises_derivative_is_the_derivative():
    rng = np.random.default_rng(3)
    for S in (3, 6):
        s, d = rng.standard_normal(S), rng.standard_normal(S)
        fd = (sc.von_mises(s + 1e-6 * d) - sc.von_mises(s - 1e-6 * d)) / 2e-6
        assert float(sc.von_mises_derivative(s, sc.von_mises(s)) @ d) == pytest.approx(fd, rel=1e-8)


def test_measure_does_not_overflow_and_bounds_the_maximum():
    vm = 1e6 * np.random.default_rng(4).uniform(0.5, 1.0, size=24)
    J = sc.pnorm(vm, 64.0)
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.sum(vm ** 64.0))                        # the naive sum: 1e384
    assert np.isfinite(J) and vm.max() <= J <= vm.max() * 24 ** (1.0 / 64.0)
    print("P = 64: J / vmax = %.4f" % (J / vm.max()))
    assert sc.pnorm(vm, 1.0) == pytest.approx(vm.sum(), rel=1e-14)


def test_zero_field_gives_zero_and_a_zero_gradient():
    ne, h = (3, 2), (0.5, 0.5)
    fixed, f = sc.cantilever(ne)
    res = sc.evaluate(ne, h, sc.isotropic_D(1.0, 0.3, 2), np.full(6, 0.5), 0.0 * f, fixed)
    assert res["J"] == 0.0
    assert np.array_equal(res["a"], np.zeros_like(res["a"])) and np.array_equal(res["gradient"], np.zeros(6))


def _small(name):
    ne, h, seed = SMALL[name]
    fixed, f = sc.cantilever(ne)
    rho = np.random.default_rng(seed).uniform(0.2, 1.0, size=int(np.prod(ne)))
    return ne, h, sc.isotropic_D(1.0, 0.3, len(ne)), rho, f, fixed


@pytest.mark.parametrize("name", list(SMALL))
def test_gradient_matches_a_central_difference(name):
    ne, h, D, rho, f, fixed = _small(name)
    res = sc.evaluate(ne, h, D, rho, f, fixed)
    d = np.random.default_rng(7).standard_normal(rho.size)
    Jp = sc.evaluate(ne, h, D, rho + FD_STEP * d, f, fixed, want_gradient=False)["J"]
    Jm = sc.evaluate(ne, h, D, rho - FD_STEP * d, f, fixed, want_gradient=False)["J"]
    fd, an = (Jp - Jm) / (2.0 * FD_STEP), float(res["gradient"] @ d)
    err = abs(fd - an) / abs(an)
    print("central difference %s: %.2e (dJ = %.6e)" % (name, err, an))
    assert err < TOL_FD[name]
    # the adjoint load is dJ/du at fixed densities
    du = np.random.default_rng(8).standard_normal(res["u"].size) * np.abs(res["u"]).max()
    Ju = lambda v: sc.pnorm(sc.fields(ne, h, D, res["m"], v)[2], 8.0)
    a_free = sc.adjoint_load(ne, h, D, res["m"], res["u"], 8.0)
    fd = (Ju(res["u"] + 1e-6 * du) - Ju(res["u"] - 1e-6 * du)) / 2e-6
    assert float(a_free @ du) == pytest.approx(fd, rel=1e-7)
    assert np.array_equal(res["a"][fixed.reshape(-1)], np.zeros(int(fixed.sum())))


def test_gradient_matches_central_differences_entry_by_entry():
    ne, h, D, rho, f, fixed = _small("6x4")
    g = sc.evaluate(ne, h, D, rho, f, fixed)["gradient"]
    fd = np.empty_like(g)
    for i in range(g.size):
        e = np.zeros(g.size)
        e[i] = FD_STEP
        fd[i] = (sc.evaluate(ne, h, D, rho + e, f, fixed, want_gradient=False)["J"]
                 - sc.evaluate(ne, h, D, rho - e, f, fixed, want_gradient=False)["J"]) / (2.0 * FD_STEP)
    err = np.abs(fd - g).max() / np.abs(g).max()
    print("entry by entry: %.2e" % err)
    assert err < TOL_FD_ENTRY


def test_gradient_is_sign_indefinite():
    """what PNormStressObjective's docstring says about the optimality-criterion step rests on this"""
    ne, h, D, rho, f, fixed = _small("6x4")
    g = sc.evaluate(ne, h, D, rho, f, fixed)["gradient"]
    print("6 x 4 gradient: %d positive, %d negative entries" % ((g > 0).sum(), (g < 0).sum()))
    assert (g > 0).any() and (g < 0).any()


def test_cg_and_both_orderings_agree_with_each_other():
    ne, h, D, rho, f, fixed = sc.case("16x12")
    a = sc.evaluate(ne, h, D, rho, f, fixed, want_gradient=False)
    b = sc.evaluate(ne, h, D, rho, f, fixed, want_gradient=False, solve=lambda K, r: sc.solve_direct(K, r, "NATURAL"))
    c = sc.evaluate(ne, h, D, rho, f, fixed, want_gradient=False, solve=lambda K, r: sc.solve_cg(K, r, 1e-12))
    assert np.abs(a["u"] - b["u"]).max() < 1e-11 * np.abs(a["u"]).max()
    assert np.abs(a["u"] - c["u"]).max() < 1e-9 * np.abs(a["u"]).max()
    assert a["K0"] is not None and np.abs(a["K0"] - hc.element_constants(D, h)[0]).max() == 0.0
