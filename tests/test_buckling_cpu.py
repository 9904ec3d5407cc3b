"""CPU checks of tests/buckling_cpu.py, the restatement the GPU tests of ndr_amd.buckling compare against (no GPU, no library).

Fixtures: column2 (16 x 6, h = 0.125) and column3 (8 x 4 x 3, h = 0.25) under a unit end load along -x spread evenly over the nodes
of the far face, cantilever2 (16 x 12, h = 0.125) under stress_cpu.cantilever's point load; densities uniform in [0.2, 1] from
default_rng(0), E = 1, nu = 0.3, E_min = 1e-3, gamma = q = 3, the x = 0 face clamped, four modes, P = 8.  column3even is column3 on
8 x 4 x 4 elements, a grid a multigrid hierarchy can halve: lowest nu -108.5 -100.7 -58.09 -55.66 -54.43, 17 iterations, 0 / 128
gradient signs, central difference 1.3e-7 (its fourth and fifth nu lie 2 % apart).  Measured here:
  the lowest five nu are -297.7 -63.92 -49.69 -37.61 -36.08 (column2), -240.4 -136.2 -50.92 -40.25 -29.94 (column3) and
  -74.75 -60.33 -58.32 -53.44 -40.48 (cantilever2, whose largest nu is +80.8: K_G is indefinite);
  the central difference of J (step 1e-5 along a default_rng(1) direction, dense solves) misses the gradient by 2.4e-8 / 3.7e-9 /
  1.7e-8 of it; the gradient has 0 positive and 96 negative entries on the two columns, 42 and 150 on the cantilever;
  Euler's column (uniform solid, nu = 0, clamped-free): lambda_1 is 1.0286 times pi^2 E b^3 / 12 / (4 L^2) at 64 x 4 and 1.0051
  times at 128 x 8 (the voxel column is too stiff by its shear locking, and converges from above);
  the restatement's LOBPCG (exact K^-1, 4 + 2 columns, start default_rng(7), tol 1e-9) takes 19 / 18 / 25 iterations and differs
  from the dense solver by 3e-14 to 6e-14 of |nu_1|.
"""
import numpy as np
import pytest

import buckling_cpu as bc
import stress_cpu as sc

NAMES = ["column2", "column3", "cantilever2", "column3even"]
LOWEST = {"column2": (-297.7, -63.92, -49.69, -37.61, -36.08), "column3": (-240.4, -136.2, -50.92, -40.25, -29.94),
          "cantilever2": (-74.75, -60.33, -58.32, -53.44, -40.48), "column3even": (-108.5, -100.7, -58.09, -55.66, -54.43)}
SIGNS = {"column2": (0, 96), "column3": (0, 96), "cantilever2": (42, 150), "column3even": (0, 128)}
LOBPCG_ITERATIONS = {"column2": 19, "column3": 18, "cantilever2": 25, "column3even": 17}


@pytest.mark.parametrize("h", [(0.5, 0.3), (0.5, 0.3, 0.7)])
def test_geometric_element_matrices_are_symmetric_and_carry_no_rigid_translation(h):
    N = len(h)
    D = bc.hc.isotropic_D(1.3, 0.3, N)
    T = bc.geometric_element_matrices(D, h)
    assert T.shape == (N * 2 ** N, 2 ** N, 2 ** N)
    assert np.abs(T - T.transpose(0, 2, 1)).max() < 1e-15 * np.abs(T).max()
    assert np.abs(T.sum(axis=2)).max() < 1e-14 * np.abs(T).max()            # grad of a constant is zero
    # a rigid translation of the element stresses nothing
    for c in range(N):
        one = np.zeros(N * 2 ** N)
        one[c::N] = 1.0
        assert np.abs(np.einsum("j,jnm->nm", one, T)).max() < 1e-14 * np.abs(T).max()
    # a uniform uniaxial strain along x gives sigma_xx = D[0, 0]: K_G,e is then D00 times the x-part of the Laplacian
    u = np.zeros((2 ** N, N))
    for n, l in enumerate(np.ndindex(*([2] * N))):
        u[n, 0] = l[0] * h[0]
    G = np.einsum("j,jnm->nm", u.reshape(-1), T)
    x = np.array([l[0] * h[0] for l in np.ndindex(*([2] * N))])
    assert abs(x @ G @ x - D[0, 0] * np.prod(h)) < 1e-13 * D[0, 0] * np.prod(h)


@pytest.mark.parametrize("name", NAMES)
def test_geometric_stiffness_is_symmetric_and_the_fixture_spectrum_is_the_recorded_one(name):
    ref = bc.reference(name)
    KG = ref["op"]["KG"]
    assert abs(KG - KG.T).max() < 1e-14 * abs(KG).max()
    low = ref["spectrum"][:5]
    print("%s: lowest nu %s, largest %.4g" % (name, " ".join("%.4g" % v for v in low), ref["spectrum"][-1]))
    assert np.allclose(low, LOWEST[name], rtol=5e-4, atol=0.0)                # (recorded to four digits)
    assert (np.diff(low[:bc.NUM_MODES + 1]) / np.abs(low[1:bc.NUM_MODES + 1])).min() > 1e-2
    if name == "cantilever2":
        assert ref["spectrum"][-1] > 50.0                                    # indefinite: part of the beam is in tension
    # the element-by-element product is the assembled one
    op = ref["op"]
    X = np.random.default_rng(3).standard_normal((2, op["ndof"]))
    Y = bc.kernel_apply(op["ne"], op["T"], op["mG"], op["u"], X, op["fixed"])
    Xf = X[:, op["free"]]
    assert np.abs(Y[:, op["free"]] - (KG @ Xf.T).T).max() < 1e-13 * np.abs(Y).max() and not Y[:, op["fixed"]].any()


@pytest.mark.parametrize("name", NAMES)
def test_gradient_matches_a_central_difference(name):
    c = bc.case(name)
    rho = c[3]
    g = bc.reference(name)["gradient"]
    d = np.random.default_rng(1).standard_normal(rho.size)
    step = 1e-5
    J = [bc.evaluate(c, rho + s * step * d, want_gradient=False)["J"] for s in (1.0, -1.0)]
    fd, an = (J[0] - J[1]) / (2.0 * step), float(g @ d)
    print("central difference %s: %.2e; %d positive and %d negative entries" % (name, abs(fd - an) / abs(an), (g > 0).sum(), (g < 0).sum()))
    assert abs(fd - an) < 1e-6 * abs(an)
    assert ((g > 0).sum(), (g < 0).sum()) == SIGNS[name]


def test_adjoint_load_is_the_derivative_of_the_rayleigh_quotients():
    """a is -sum_i w_i d(phi_i^T K_G(u) phi_i)/du at fixed modes: K_G is linear in u, so a difference quotient is exact"""
    ref = bc.reference("column2")
    op, nu, Phi = ref["op"], ref["nu"], ref["Phi"]
    w = bc.mode_weights(nu)
    d = np.random.default_rng(2).standard_normal(op["ndof"])
    d[op["fixed"]] = 0.0
    q = lambda u: sum(w[i] * Phi[:, i] @ bc.kernel_apply(op["ne"], op["T"], op["mG"], u, Phi[:, i][None])[0] for i in range(len(nu)))
    assert abs(-q(d) - ref["a"] @ d) < 1e-12 * abs(ref["a"] @ d)


@pytest.mark.parametrize("ne,h,low,high", [((64, 4), 0.25, 1.0, 1.04), ((128, 8), 0.125, 1.0, 1.01)])
def test_eulers_column(ne, h, low, high):
    lam, closed = bc.euler_column(ne, h)
    print("Euler column %d x %d: lambda_1 %.6e, closed form %.6e, ratio %.4f" % (ne[0], ne[1], lam, closed, lam / closed))
    assert low < lam / closed < high


@pytest.mark.parametrize("name", NAMES)
def test_lobpcg_matches_the_dense_solver(name):
    ref = bc.reference(name)
    op = ref["op"]
    nu, Phi, its, res = bc.lobpcg_modes(op, bc.NUM_MODES, 1e-9, bc.start_block(op, bc.NUM_MODES + 2))
    err = np.abs(nu - ref["nu"]).max() / abs(ref["nu"][0])
    Kf = op["K"]
    overlap = np.abs(np.einsum("ni,ni->i", ref["Phi"][op["free"]], Kf @ Phi[op["free"]]))
    orth = np.abs(Phi[op["free"]].T @ (Kf @ Phi[op["free"]]) - np.eye(bc.NUM_MODES)).max()
    J = bc.objective(nu)
    g = bc.gradient(op, nu, Phi)[0]
    print("lobpcg %s: %d iterations, nu %.2e, 1 - overlap %.2e, orthonormality %.2e, residuals %.2e; J %.2e gradient %.2e"
          % (name, its, err, np.abs(1 - overlap).max(), orth, res.max(), abs(J - ref["J"]) / ref["J"],
             np.abs(g - ref["gradient"]).max() / np.abs(ref["gradient"]).max()))
    assert res.max() <= 1e-9 and err < 1e-12 and its <= LOBPCG_ITERATIONS[name] + 2
    assert np.abs(1.0 - overlap).max() < 1e-10 and orth < 1e-12


def test_column2_pulled_is_not_in_pure_tension():
    """K_G is linear in u: reversing the load negates the spectrum.  With its random densities the pushed column2 has 20 positive nu
    (lateral compression around the stiff inclusions and at the clamp), so the pulled column has 20 buckling modes of its own, the
    first at lambda = 1 / 1.283 = 0.780: a correct solver finds them and does not refuse that load as one that compresses nothing."""
    ne, h, D, rho, fixed, f = bc.case("column2")
    pushed = bc.reference("column2")["spectrum"]
    op = bc.operators(ne, h, D, rho, fixed, -f)
    pulled = bc.dense_modes(op, 1)[2]
    assert np.abs(pulled + pushed[::-1]).max() < 1e-10 * np.abs(pushed).max()
    assert (pulled < 0).sum() == 20 and np.allclose(pulled[:4], (-1.2826, -1.1779, -0.98237, -0.75556), rtol=5e-5, atol=0.0)


def test_chain_with_conjugate_gradient_solves_matches_the_direct_chain():
    """what the multigrid-objective GPU test may differ by: u and the adjoint v from a conjugate gradient to a relative residual of
    1e-12 (stress_cpu.solve_cg) instead of SuperLU, dense modes in both chains, on column3even.  Measured here: J 7.9e-15, gradient
    2.7e-12 of the largest entry (printed)."""
    ref = bc.reference("column3even")
    cg = bc.evaluate("column3even", solve=lambda K, b: sc.solve_cg(K, b, 1e-12))
    dJ = abs(cg["J"] - ref["J"]) / ref["J"]
    dg = np.abs(cg["gradient"] - ref["gradient"]).max() / np.abs(ref["gradient"]).max()
    print("CG chain column3even: J %.2e gradient %.2e" % (dJ, dg))
    assert dJ < 1e-11 and dg < 1e-11
