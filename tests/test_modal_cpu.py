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
  the gradient of J has 71 positive and 121 negative entries on 16 x 12, 147 and 237 on 8 x 8 x 6;
  at the other block sizes (modes + guard columns; tests/test_gpu_modal_blocks.py takes its bounds from these) the LOBPCG takes, with
  eigenvalue errors relative to the largest one asked for and X^T M X - I,
      1 + 0:  7 iterations, 5.72e-13, 6.7e-16 (16 x 12)   and 17, 3.23e-13, 1.1e-16 (8 x 8 x 6)
      1 + 2:  6, 5.77e-13, 4.4e-16                        and  8, 3.18e-13, 1.1e-15
      2 + 2:  9, 7.10e-14, 2.2e-16                        and  8, 2.42e-13, 1.4e-15
      8 + 0: 22, 1.07e-14, 2.6e-15                        and 18, 2.20e-14, 1.1e-15
  and on buckling_cpu's column2 with one mode and two guard columns 9 iterations, 9.13e-14 of |nu_1|, phi^T K phi - 1 7.9e-14;
  modal_cpu.kernel_gradient (np.longdouble) differs from modal_cpu.gradient (float64) by 1.8e-16 / 1.7e-16 of the sum of the
  absolute values of its products on the two fixtures.
"""
import numpy as np
import pytest

import modal_cpu as mc
import stress_cpu as sc

NAMES = ["16x12", "8x8x6"]
BLOCKS = [(1, 0), (1, 2), (2, 2), (8, 0)]          # (modes, guard columns): the block sizes m = 1, 3, 4, 8


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


@pytest.mark.parametrize("modes,guard", BLOCKS)
@pytest.mark.parametrize("name", NAMES)
def test_lobpcg_at_the_other_block_sizes(name, modes, guard):
    """prints the figures the bounds of tests/test_gpu_modal_blocks.py are ten times of (its docstring quotes them)"""
    op = mc.reference(name)["op"]
    want = mc.reference(name)["spectrum"][:modes]
    lam, X, its, res = mc.lobpcg(op["K"], op["M"], modes, 1e-9, mc.start_block(op, modes + guard), guard=guard)
    err = np.abs(lam - want).max() / want.max()
    orth = np.abs(X.T @ (op["M"] @ X) - np.eye(modes)).max()
    print("lobpcg %s, %d modes + %d guard: %d iterations, eigenvalues %.2e, X^T M X - I %.2e, residuals %.2e" % (name, modes, guard, its, err, orth, res.max()))
    assert res.max() <= 1e-9 and err < 1e-11 and orth < 1e-12 and its <= 30
    block = np.hstack([X, mc.start_block(op, guard, seed=8)]) if guard else X
    assert mc.lobpcg(op["K"], op["M"], modes, 1e-9, block, guard=guard)[2] <= 2


def test_buckling_lobpcg_with_one_mode():
    """the shared driver with the other pair of operators at m = 3: the figures behind test_gpu_modal_blocks' buckling bound"""
    import buckling_cpu as bc
    ref = bc.reference("column2")
    op = ref["op"]
    nu, Phi, its, res = bc.lobpcg_modes(op, 1, 1e-9, bc.start_block(op, 3))
    err = abs(nu[0] - ref["nu"][0]) / abs(ref["nu"][0])
    p = Phi[op["free"]]
    orth = abs(float((p.T @ (op["K"] @ p))[0, 0]) - 1.0)
    print("buckling lobpcg column2, 1 mode + 2 guard: %d iterations, nu %.2e, phi^T K phi - 1 %.2e, residual %.2e" % (its, err, orth, res.max()))
    assert res.max() <= 1e-9 and err < 1e-11 and orth < 1e-12 and its <= 30


def _gradient_bound(ne, nmodes):
    """the bound the device kernel is held to (tests/test_gpu_modal_blocks.py); float64 numpy sums have no longer chains"""
    return 2.0 * mc.kernel_gradient_chain(len(ne), nmodes) * 2.0 ** -53


@pytest.mark.parametrize("name", NAMES)
def test_kernel_gradient_is_the_gradient_on_the_fixtures(name):
    ref = mc.reference(name)
    op, lam = ref["op"], ref["lam"]
    ne, h = mc.CASES[name][0], mc.CASES[name][1]
    g, S = mc.kernel_gradient(ne, h, op["K0"], op["dE"], op["dm"], ref["Phi"].T, -lam ** -2.0, 1.0 / lam)
    ratio = (np.abs(g - ref["gradient"]) / S).max().astype(np.float64)
    print("kernel_gradient against gradient, %s: %.2e of S (bound %.2e)" % (name, ratio, _gradient_bound(ne, len(lam))))
    assert g.dtype == np.longdouble and (S > 0).all() and (np.abs(g) <= S).all()
    assert ratio < _gradient_bound(ne, len(lam))


def test_kernel_gradient_is_the_derivative_of_the_assembled_matrices():
    """on 3 x 2, a random block, coefficients of both signs and a random (unsymmetric) element matrix:
    g_e = sum_i cK_i phi_i^T dK/drho_e phi_i + cM_i phi_i^T dM/drho_e phi_i with the two derivatives assembled by scipy"""
    ne, h = (3, 2), (0.5, 0.3)
    rng = np.random.default_rng(31)
    nel, nd = 6, sc.num_nodes(ne) * 2
    K0 = rng.standard_normal((8, 8))
    dE, dm, Phi = rng.standard_normal(nel), rng.standard_normal(nel), rng.standard_normal((3, nd))
    cK, cM = np.array([0.7, -1.3, 0.4]), np.array([-0.6, 0.9, 1.1])
    g, S = mc.kernel_gradient(ne, h, K0, dE, dm, Phi, cK, cM)
    free = np.zeros(nd, dtype=bool)
    for e in range(nel):
        one = np.zeros(nel)
        one[e] = 1.0
        dK = sc.assemble(ne, K0, dE * one, free).toarray()
        dM = mc.assemble_mass(ne, h, dm * one).toarray()
        want = sum(cK[i] * Phi[i] @ dK @ Phi[i] + cM[i] * Phi[i] @ dM @ Phi[i] for i in range(3))
        assert abs(float(g[e]) - want) < _gradient_bound(ne, 3) * float(S[e])
    # the symmetric part of K0 alone enters the value, every entry the sum of absolute values
    gs, Ss = mc.kernel_gradient(ne, h, 0.5 * (K0 + K0.T), dE, dm, Phi, cK, cM)
    assert np.abs(gs - g).max() < 1e-15 * S.max() and (Ss <= S * (1 + 1e-15)).all() and (Ss < S).any()


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
