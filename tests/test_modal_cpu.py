"""CPU checks of tests/modal_cpu.py, the restatement the GPU tests of ndr_amd.modal compare against (no GPU, no library).

Fixtures: 16 x 12 and 8 x 8 x 6, densities uniform in [0.2, 1] from default_rng(0), E = 1, nu = 0.3, E_min = 1e-3, gamma = 3, left
face clamped, four modes.  Measured here:
  the lowest five eigenvalues are separated by relative gaps of 0.88 / 0.15 / 0.73 / 0.069 (16 x 12) and 0.25 / 0.43 / 0.70 / 0.18
  (8 x 8 x 6): the modes can be compared one by one (the tests ask for 1e-2);
  the restatement's LOBPCG (exact K^-1, two guard columns) reaches tol 1e-9 in 14 iterations on either fixture with eigenvalue
  errors of 1.8e-14 and 4.2e-14 of the largest of the four against the dense solver, mode overlaps within 1.2e-15 / 2.0e-15 of 1
  and X^T M X within 2.3e-15 / 3.8e-15 of the identity; at tol 1e-12 it takes 19 / 18 iterations, and its residuals then hover
  between 1e-12 and 1e-11 on 16 x 12 (the rounding floor 2^-53 lambda_max / lambda_1 is 3.7e-12 there);
  the central difference of J (step 1e-5, dense solves) misses the gradient by 6.57e-8 (16 x 12) and 9.19e-9 (8 x 8 x 6);
  the gradient of J has 71 positive and 121 negative entries on 16 x 12, 147 and 237 on 8 x 8 x 6.
"""
import numpy as np
import pytest

import modal_cpu as mc
import stress_cpu as sc

NAMES = ["16x12", "8x8x6"]


@pytest.mark.parametrize("h", [(0.5, 0.3), (0.5, 0.3, 0.7)])
def test_element_mass_matrix_is_symmetric_positive_definite_and_sums_to_the_volume(h):
    M0 = mc.mass_element(h)
    N = len(h)
    assert M0.shape == (N * 2 ** N,) * 2 and np.array_equal(M0, M0.T)
    assert np.linalg.eigvalsh(M0).min() > 0.0
    for c in range(N):
        one = np.zeros(N * 2 ** N)
        one[c::N] = 1.0
        assert abs(one @ M0 @ one - np.prod(h)) < 1e-15 * np.prod(h) * 8
        other = np.zeros(N * 2 ** N)
        other[(c + 1) % N::N] = 1.0
        assert one @ M0 @ other == 0.0                     # the identity across components


@pytest.mark.parametrize("name", NAMES)
def test_total_mass_per_component(name):
    ne, h, D, rho, fixed = mc.case(name)
    N = len(ne)
    m = mc.mass_multipliers(rho, massDensity=2.5, massExponent=1.5)[0]
    M = mc.assemble_mass(ne, h, m)
    assert abs(M - M.T).max() < 1e-15 * abs(M).max()            # (duplicates are summed in the order scipy meets them)
    for c in range(N):
        one = np.zeros(M.shape[0])
        one[c::N] = 1.0
        total = m.sum() * np.prod(h)
        assert abs(one @ (M @ one) - total) < 1e-13 * total


@pytest.mark.parametrize("name", NAMES)
def test_fixture_eigenvalues_are_separated(name):
    spectrum = mc.reference(name)["spectrum"]
    gaps = np.diff(spectrum[:5]) / spectrum[1:5]
    print("relative gaps %s: %s" % (name, " ".join("%.3g" % v for v in gaps)))
    assert spectrum[0] > 0.0 and gaps.min() >= 1e-2


@pytest.mark.parametrize("name", NAMES)
def test_lobpcg_matches_the_dense_solver(name):
    ref = mc.reference(name)
    op = ref["op"]
    lam, X, its, res = mc.lobpcg(op["K"], op["M"], mc.NUM_MODES, 1e-9, mc.start_block(op, mc.NUM_MODES + 2))
    err = np.abs(lam - ref["lam"]).max() / ref["lam"].max()
    overlap = np.abs(np.einsum("ni,ni->i", ref["Phi"][op["free"]], op["M"] @ X))
    print("lobpcg %s: %d iterations, eigenvalues %.2e, 1 - overlap %.2e, residuals %.2e" % (name, its, err, np.abs(1 - overlap).max(), res.max()))
    assert res.max() <= 1e-9 and err < 1e-11 and np.abs(1.0 - overlap).max() < 1e-10 and its <= 30
    assert np.abs(X.T @ (op["M"] @ X) - np.eye(mc.NUM_MODES)).max() < 1e-12
    # a warm start from the converged block finishes at once
    again = mc.lobpcg(op["K"], op["M"], mc.NUM_MODES, 1e-9, np.hstack([X, mc.start_block(op, 2, seed=8)]))
    assert again[2] <= 2


@pytest.mark.parametrize("name", NAMES)
def test_gradient_matches_a_central_difference_and_has_both_signs(name):
    ne, h, D, rho, fixed = mc.case(name)
    ref = mc.reference(name)
    g = ref["gradient"]
    d = np.random.default_rng(17).standard_normal(rho.size)
    step = 1e-5
    J = [mc.objective(mc.dense_modes(mc.operators(ne, h, D, rho + s * step * d, fixed), mc.NUM_MODES)[0]) for s in (1.0, -1.0)]
    fd, an = (J[0] - J[1]) / (2.0 * step), float(g @ d)
    print("central difference %s: %.2e; %d positive and %d negative entries" % (name, abs(fd - an) / abs(an), (g > 0).sum(), (g < 0).sum()))
    assert abs(fd - an) < 1e-6 * abs(an)            # step 1e-5: the truncation error measured here is 6.6e-8 and 9.2e-9
    assert (g > 0).sum() > 0 and (g < 0).sum() > 0


def test_gradient_with_a_mass_law_of_its_own():
    ne, h, D, rho, fixed = mc.case("16x12")
    mass = dict(massDensity=2.0, massExponent=1.0, lowDensityCut=0.5)
    d = np.random.default_rng(18).standard_normal(rho.size)
    op = mc.operators(ne, h, D, rho, fixed, mass)
    lam, Phi, _ = mc.dense_modes(op, 3)
    an = float(mc.gradient(op, lam, Phi) @ d)
    J = [mc.objective(mc.dense_modes(mc.operators(ne, h, D, rho + s * 1e-5 * d, fixed, mass), 3)[0]) for s in (1.0, -1.0)]
    assert abs((J[0] - J[1]) / 2e-5 - an) < 1e-7 * abs(an)


@pytest.mark.parametrize("cut", [0.1, 0.3])
def test_low_density_law_is_c1_at_the_cut(cut):
    eps = 1e-9
    below, above = mc.mass_multipliers([cut - eps], 3.0, 1.0, cut), mc.mass_multipliers([cut + eps], 3.0, 1.0, cut)
    assert abs(below[0][0] - above[0][0]) < 1e-7 and abs(below[1][0] - above[1][0]) < 1e-6
    m, dm = mc.mass_multipliers([cut], 3.0, 1.0, cut)                     # the polynomial at the cut itself: the linear law's values
    poly = 3.0 * (6.0 * cut ** 6 / cut ** 5 - 5.0 * cut ** 7 / cut ** 6), 3.0 * (36.0 - 35.0)
    assert abs(poly[0] - 3.0 * cut) < 1e-15 and poly[1] == 3.0 and m[0] == 3.0 * cut and dm[0] == 3.0
    if cut == 0.1:                                                        # the published coefficients
        r = 0.05
        assert abs(mc.mass_multipliers([r], 1.0, 1.0, 0.1)[0][0] - (6e5 * r ** 6 - 5e6 * r ** 7)) < 1e-18
    x = np.linspace(1e-3, cut, 50, endpoint=False)
    m, dm = mc.mass_multipliers(x, 1.0, 1.0, cut)
    assert (m > 0).all() and (dm > 0).all() and (m <= x).all()
