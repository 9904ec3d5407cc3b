"""CPU: pins tests/homogenization_cpu.py (the restatement the GPU tests of periodic homogenisation compare against) on facts that
do not come from it, and ``closestIsotropicTensor`` (host code of ndr_amd/homogenization.py)."""
import numpy as np
import pytest

import homogenization_cpu as hc
import material_ref as mr


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def test_element_constants_match_the_independent_quadrature():
    """K0 against material_ref.reference_stiffness (loops of its own) and L against its constant_strain_load on one element"""
    D = mr.material_file_D(mr.ANISO_3D)
    h = (1.0, 0.7, 1.3)
    K0, L, vol = hc.element_constants(D, h)
    assert _relmax(K0, mr.reference_stiffness(D, h)) < 1e-13
    for q, (i, j) in enumerate(hc.PAIRS[3]):
        eps = np.zeros((3, 3))
        eps[i, j] = eps[j, i] = 1.0 if i == j else 0.5
        assert np.abs(L[:, q] - mr.constant_strain_load(D, eps, h, (1, 1, 1), [1.0]).reshape(-1)).max() < 1e-13 * np.abs(L).max()
    assert vol == pytest.approx(0.91)


def test_laminate_matches_closed_form():
    """8 x 4 x 4 two-phase laminate, layers normal to x, E = 1 / 0.5, nu = 0.3, gamma = 1, E_min = 0 (measured: 8e-16)"""
    ne = (8, 4, 4)
    rho = np.ones(ne)
    rho[4:] = 0.5
    res = hc.homogenize(ne, (1.0 / 8, 1.0 / 4, 1.0 / 4), hc.isotropic_D(1.0, 0.3), rho)
    lam, mu = hc.lame(1.0, 0.3)
    exact = hc.laminate_closed_form([(lam, mu), (0.5 * lam, 0.5 * mu)], [0.5, 0.5])
    assert np.abs(res["Eh"] - exact).max() < 1e-12


def test_energy_identity():
    """sum_e E_e G_e = Eh at the exact solution (measured: 3e-15)"""
    ne = (4, 4, 4)
    rho = np.random.default_rng(3).uniform(0.2, 1.0, size=ne)
    res = hc.homogenize(ne, (0.25, 0.25, 0.25), mr.material_file_D(mr.ANISO_3D), rho, 1.0, 1e-3, 3.0)
    assert _relmax(np.einsum("e,eqr->qr", res["E"], res["G"]), res["Eh"]) < 1e-12


def test_gradient_matches_central_differences():
    """a central difference in one density of a random 4^3 cell (gamma = 3, E_min = 1e-3, step 1e-6) against dE/drho G_e"""
    ne, h, D = (4, 4, 4), (0.25, 0.25, 0.25), hc.isotropic_D(1.0, 0.3)
    rho = np.random.default_rng(4).uniform(0.2, 1.0, size=ne)
    res = hc.homogenize(ne, h, D, rho, 1.0, 1e-3, 3.0)
    e, step = 27, 1e-6
    Eh = []
    for sgn in (1.0, -1.0):
        r2 = rho.copy().reshape(-1)
        r2[e] += sgn * step
        Eh.append(hc.homogenize(ne, h, D, r2, 1.0, 1e-3, 3.0)["Eh"])
    fd = (Eh[0] - Eh[1]) / (2.0 * step)
    assert _relmax(res["dE"][e] * res["G"][e], fd) < 1e-7


def test_pcg_agrees_with_direct_solve():
    """the restatement's own block-Jacobi PCG reaches its tolerance and the direct solution (2-D and 3-D)"""
    for ne, h, D in (((6, 5, 4), (0.2, 0.25, 0.3), mr.material_file_D(mr.ANISO_3D)), ((8, 6), (0.125, 0.2), mr.material_file_D(mr.ANISO_2D))):
        rho = np.random.default_rng(5).uniform(0.3, 1.0, size=ne)
        res = hc.homogenize(ne, h, D, rho, 1.0, 1e-3, 3.0)
        W, its = hc.pcg_columns(res["K"], res["b"], len(ne), 1e-10)
        assert all(0 < i < res["K"].shape[0] for i in its)
        for q in range(len(W)):
            r = res["b"][q] - res["K"] @ W[q]
            assert np.linalg.norm(r) <= 1.01e-10 * np.linalg.norm(res["b"][q])       # (the recurrence residual met 1e-10)
        assert _relmax(W, res["W"]) < 1e-7


def test_full_grid_fields_repeat_on_opposite_faces():
    ne = (3, 4)
    W = np.arange(3 * 12 * 2, dtype=np.float64).reshape(3, 24)
    F = hc.to_full(ne, W).reshape(3, 4, 5, 2)
    assert np.array_equal(F[:, 0], F[:, 3]) and np.array_equal(F[:, :, 0], F[:, :, 4])
    assert np.array_equal(F[:, :3, :4].reshape(3, 24), W)


def test_closest_isotropic_tensor():
    from ndr_amd import ElasticityTensor
    from ndr_amd.homogenization import closestIsotropicTensor
    for dim in (2, 3):
        iso = ElasticityTensor(2.5, 0.3, dim=dim)
        assert np.abs(closestIsotropicTensor(iso).D - iso.D).max() < 1e-14 * np.abs(iso.D).max()
    ortho = ElasticityTensor(dim=3)
    ortho.setOrthotropic(2.0, 1.0, 1.5, 0.2, 0.25, 0.3, 0.5, 0.6, 0.4)
    rot = ortho.transform(hc.rotation((1.0, 2.0, 3.0), 0.7))
    c = closestIsotropicTensor(rot)
    D = c.D
    lam, mu = D[0, 1], D[3, 3]
    assert np.abs(D - hc_isotropic_lame(lam, mu)).max() < 1e-14
    assert mu > 0 and lam + 2 * mu / 3 > 0
    # the projection is invariant under rotation of the argument, idempotent, and orthogonal: <C - Ciso, Ciso> = 0
    assert np.abs(closestIsotropicTensor(ortho).D - D).max() < 1e-13
    assert np.abs(closestIsotropicTensor(c).D - D).max() < 1e-14
    full, fiso = rot.fullTensor(), c.fullTensor()
    assert abs(np.sum((full - fiso) * fiso)) < 1e-12 * np.sum(fiso * fiso)
    with pytest.raises(TypeError):
        closestIsotropicTensor(np.eye(6))


def hc_isotropic_lame(lam, mu):
    D = np.zeros((6, 6))
    D[:3, :3] = lam
    D[np.arange(3), np.arange(3)] = lam + 2.0 * mu
    D[np.arange(3, 6), np.arange(3, 6)] = mu
    return D
