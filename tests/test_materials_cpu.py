"""CPU checks of the material layer: the ``ElasticityTensor`` value class and the material-file parser (ndr_amd/materials.py)
against closed forms and against tests/material_ref.py, and material_ref's own K0 against the oracle and against the structure
the tuned kernels assume (45 mode-space entries, 36 magnitudes, mirror symmetry)."""
import json

import numpy as np
import pytest

import material_ref as mr
from ndr_amd import ElasticityTensor
from ndr_amd.materials import read_material

H = (1.0, 0.7, 1.3)                                         # a non-cubic box voxel


def rot_z(deg, dim=3):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    if deg % 90 == 0:                                       # exact quarter turns
        c, s = float(round(c)), float(round(s))
    R = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return R[:dim, :dim]


def _write(tmp_path, obj, name="m.material"):
    p = tmp_path / name
    p.write_text(json.dumps(obj))
    return str(p)


@pytest.mark.parametrize("kind", ["isotropic_material", "isotropic", "orthotropic_material", "orthotropic", "symmetric_material",
                                  "anisotropic"])
@pytest.mark.parametrize("dim", [2, 3])
def test_all_six_type_strings_parse(tmp_path, kind, dim):
    ortho = json.load(open(mr.ORTHO_3D if dim == 3 else mr.ORTHO_2D))
    if kind.startswith("isotropic"):
        obj, want = {"type": kind, "young": 2.0, "poisson": 0.25}, ElasticityTensor(2.0, 0.25, dim=dim).D
    elif kind.startswith("orthotropic"):
        obj, want = dict(ortho, type=kind), mr.compliance_matrix_inverse(ortho["young"], ortho["poisson"], ortho["shear"])
    else:
        want = mr.material_file_D(mr.ANISO_3D if dim == 3 else mr.ANISO_2D)
        obj = {"type": kind, "material_matrix": want.tolist()}
    t = read_material(_write(tmp_path, obj), dim)
    assert t.dim == dim and t.D.shape == want.shape
    assert np.abs(t.D - want).max() <= 1e-14 * np.abs(want).max()
    assert ElasticityTensor(_write(tmp_path, obj), dim=dim) == t


@pytest.mark.parametrize("path,dim", [(mr.ORTHO_3D, 3), (mr.ORTHO_2D, 2)])
def test_orthotropic_file_is_the_inverse_compliance(path, dim):
    m = json.load(open(path))
    D = read_material(path, dim).D
    want = mr.compliance_matrix_inverse(m["young"], m["poisson"], m["shear"])
    assert np.abs(D - want).max() <= 1e-14 * np.abs(want).max()
    assert np.array_equal(D, D.T)
    n = dim
    assert np.all(D[:n, n:] == 0) and np.all(D[n:, n:] == np.diag(np.diag(D[n:, n:])))
    # shear rows hold tensor components: C_yzyz = mu_yz, no factor 2 (3-D file order yz, zx, xy = flattened rows 3, 4, 5)
    assert np.allclose(np.diag(D)[n:], m["shear"], rtol=1e-15)


def test_isotropic_is_the_lame_form():
    E, nu = 1.7, 0.31
    lam, mu = nu * E / ((1 + nu) * (1 - 2 * nu)), E / (2 + 2 * nu)
    D = ElasticityTensor(E, nu).D
    want = np.zeros((6, 6))
    want[:3, :3] = lam
    want[np.arange(3), np.arange(3)] = lam + 2 * mu
    want[np.arange(3, 6), np.arange(3, 6)] = mu
    assert np.array_equal(D, want)
    lam2 = nu * E / (1 - nu * nu)                           # plane stress
    D2 = ElasticityTensor(E, nu, dim=2).D
    assert np.array_equal(D2, np.array([[lam2 + 2 * mu, lam2, 0], [lam2, lam2 + 2 * mu, 0], [0, 0, mu]]))
    ident = ElasticityTensor()
    assert np.array_equal(ident.D, np.diag([1, 1, 1, 0.5, 0.5, 0.5])) and ident == ElasticityTensor(1.0, 0.0)
    t = ElasticityTensor(E, nu)
    assert t(0, 0, 0, 0) == lam + 2 * mu and t(0, 0, 1, 1) == lam and t(1, 2, 2, 1) == mu and t(0, 1, 2, 2) == 0.0
    t.setIdentity()
    assert t == ident
    assert "ElasticityTensor3D" in repr(t) and "ElasticityTensor2D" in repr(ElasticityTensor(dim=2))


def test_transform_quarter_turn_swaps_x_and_y():
    Ex, Ey, Ez, nuYX, nuZX, nuZY, muYZ, muZX, muXY = read_material(mr.ORTHO_3D, 3).getOrthotropicParameters()
    t = ElasticityTensor()
    t.setOrthotropic(Ex, Ey, Ez, nuYX, nuZX, nuZY, muYZ, muZX, muXY)
    swapped = ElasticityTensor()
    nuXY = nuYX * Ex / Ey                                   # what was nu_xy becomes nu_yx of the turned material
    swapped.setOrthotropic(Ey, Ex, Ez, nuXY, nuZY, nuZX, muZX, muYZ, muXY)
    got = t.transform(rot_z(90)).D
    assert np.abs(got - swapped.D).max() <= 1e-14 * np.abs(swapped.D).max()
    t2 = read_material(mr.ORTHO_2D, 2)
    Ex, Ey, nuYX, muXY = t2.getOrthotropicParameters()
    s2 = ElasticityTensor(dim=2)
    s2.setOrthotropic(Ey, Ex, nuYX * Ex / Ey, muXY)
    assert np.abs(t2.transform(rot_z(90, 2)).D - s2.D).max() <= 1e-14 * np.abs(s2.D).max()


@pytest.mark.parametrize("path,dim", [(mr.ORTHO_3D, 3), (mr.ORTHO_2D, 2)])
def test_transform_there_and_back_and_the_stored_anisotropic_fixture(path, dim):
    t = read_material(path, dim)
    turned = t.transform(rot_z(30, dim))
    back = turned.transform(rot_z(-30, dim))
    assert np.abs(back.D - t.D).max() <= 1e-14 * np.abs(t.D).max()
    stored = read_material(mr.ANISO_3D if dim == 3 else mr.ANISO_2D, dim)
    assert np.abs(stored.D - turned.D).max() <= 1e-14 * np.abs(turned.D).max()
    # a rotation keeps the eigenvalues of the operator on symmetric matrices (shear columns doubled)
    w = np.diag([1.0] * dim + [np.sqrt(2.0)] * (len(t.D) - dim))
    assert np.allclose(np.linalg.eigvalsh(w @ t.D @ w), np.linalg.eigvalsh(w @ turned.D @ w), rtol=1e-12)
    with pytest.raises(RuntimeError):
        t.transform(np.eye(dim) * 2.0)


def test_orthotropic_parameters_round_trip():
    p3 = [1.0, 0.6, 1.7, 0.18, 0.34, 0.425, 0.3, 0.45, 0.25]
    t = ElasticityTensor()
    t.setOrthotropic(*p3)
    assert np.allclose(t.getOrthotropicParameters(), p3, rtol=1e-14, atol=0)
    p2 = [1.0, 0.6, 0.18, 0.25]
    t2 = ElasticityTensor(dim=2)
    t2.setOrthotropic(*p2)
    assert np.allclose(t2.getOrthotropicParameters(), p2, rtol=1e-14, atol=0)
    with pytest.raises(RuntimeError, match="setOrthotropic2D call on non-2D tensor"):
        t.setOrthotropic(*p2)
    with pytest.raises(RuntimeError, match="setOrthotropic3D call on non-3D tensor"):
        t2.setOrthotropic(*p3)


def test_refusals_carry_the_reference_messages(tmp_path):
    with pytest.raises(RuntimeError, match="Asymmetric material_matrix"):
        read_material(mr.ASYMMETRIC, 3)
    with pytest.raises(RuntimeError, match="Orthotopic parameters violate symmetry"):
        read_material(mr.INCONSISTENT, 3)
    with pytest.raises(RuntimeError, match="Orthotopic parameters violate symmetry"):
        read_material(_write(tmp_path, {"type": "orthotropic", "young": [1.0, 0.6], "poisson": [0.3, 0.2], "shear": [0.25]}), 2)
    with pytest.raises(RuntimeError, match="Invalid type."):
        read_material(_write(tmp_path, {"type": "hyperelastic", "young": 1.0, "poisson": 0.3}), 3)
    with pytest.raises(RuntimeError, match="Failed to parse vector of size 6"):
        read_material(_write(tmp_path, {"type": "orthotropic", "young": [1, 1, 1], "poisson": [0.3, 0.3], "shear": [1, 1, 1]}), 3)
    with pytest.raises(RuntimeError, match="Failed to parse material_matrix"):
        read_material(_write(tmp_path, {"type": "anisotropic", "material_matrix": np.eye(3).tolist()}), 3)
    with pytest.raises(RuntimeError, match="Couldn't open material"):
        read_material(str(tmp_path / "missing.material"), 3)


def test_indefinite_tensors_are_refused(tmp_path):
    D = mr.material_file_D(mr.ANISO_3D)
    w, V = np.linalg.eigh(D)
    bad = D - (w[0] + 0.05) * np.outer(V[:, 0], V[:, 0])     # the smallest eigenvalue moved to -0.05, still symmetric
    with pytest.raises(RuntimeError, match="not positive definite"):
        read_material(_write(tmp_path, {"type": "symmetric_material", "material_matrix": bad.tolist()}), 3)
    # nu_yx nu_xy > 1: symmetric parameters, indefinite tensor
    with pytest.raises(RuntimeError, match="not positive definite"):
        read_material(_write(tmp_path, {"type": "orthotropic", "young": [1.0, 1.0], "poisson": [1.2, 1.2], "shear": [0.4]}), 2)


# ---- material_ref's K0 ----

def _materials_3d():
    return {"orthotropic": mr.material_file_D(mr.ORTHO_3D), "anisotropic": mr.material_file_D(mr.ANISO_3D),
            "isotropic": ElasticityTensor(1.0, 0.3).D}


@pytest.mark.parametrize("name", ["isotropic", "orthotropic", "anisotropic"])
@pytest.mark.parametrize("p", [1, 2])
def test_reference_k0_is_symmetric_with_translations_in_its_null_space(name, p):
    K0 = mr.reference_stiffness(_materials_3d()[name], H, p)
    scale = np.abs(K0).max()
    assert np.abs(K0 - K0.T).max() <= 1e-14 * scale
    npe = (p + 1) ** 3
    for c in range(3):
        t = np.zeros((npe, 3))
        t[:, c] = 1.0
        assert np.abs(K0 @ t.reshape(-1)).max() <= 1e-13 * scale
    w = np.linalg.eigvalsh(0.5 * (K0 + K0.T))
    assert w.min() > -1e-13 * scale and (w > 1e-10 * scale).sum() == 3 * npe - 6      # six rigid-body modes, nothing else


@pytest.mark.parametrize("N,p", [(3, 1), (3, 2), (2, 1), (2, 2)])
def test_reference_k0_of_an_isotropic_tensor_is_the_oracles(N, p):
    from oracle import generic_oracle as go
    from oracle import vfem_oracle as vo
    lam, mu = vo.lame(1.3, 0.27, N)
    want = go.reference_stiffness(N, p, np.array(H[:N]), lam, mu)
    got = mr.reference_stiffness(ElasticityTensor(1.3, 0.27, dim=N).D, H[:N], p)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


def test_k0_structure_orthotropic_has_it_anisotropic_does_not():
    mats = _materials_3d()
    iso = mr.reference_stiffness(mats["isotropic"], H)
    assert (mr.mode_space_nonzeros(iso), mr.distinct_magnitudes(iso)) == (45, 36) and mr.mirror_residual(iso) < 1e-14
    for D in (mats["orthotropic"], ElasticityTensor.fromD(mats["orthotropic"]).transform(rot_z(90)).D):
        K0 = mr.reference_stiffness(D, H)
        assert mr.mode_space_nonzeros(K0) == 45
        assert mr.distinct_magnitudes(K0) == 36
        assert mr.mirror_residual(K0) < 1e-14
    K0 = mr.reference_stiffness(mats["anisotropic"], H)
    assert mr.mode_space_nonzeros(K0) > 45
    assert mr.distinct_magnitudes(K0) > 36
    assert mr.mirror_residual(K0) > 1e-3


def test_constant_strain_load_reference_reduces_to_the_isotropic_one():
    from oracle import vfem_oracle as vo
    ne, dom = (3, 2, 4), ([0, 0, 0], [3 * H[0], 2 * H[1], 4 * H[2]])
    o = vo.OracleSim(dom, ne)
    o.set_lame(*vo.lame(1.0, 0.3, 3))
    rho = np.random.default_rng(2).uniform(0.1, 1.0, size=24)
    o.set_densities(rho)
    eps = np.array([[0.3, 0.1, -0.2], [0.4, -0.5, 0.4], [-0.2, 0.1, 1.0]])
    sym = 0.5 * (eps + eps.T)
    got = mr.constant_strain_load(ElasticityTensor(1.0, 0.3).D, eps, H, ne, rho)
    want = o.constant_strain_load(sym)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(ElasticityTensor(1.0, 0.3).doubleContract(eps) - mr.stress_of(ElasticityTensor(1.0, 0.3).D, eps)).max() < 1e-15
