"""-m gpu: periodic homogenisation (ndr_amd/homogenization.py, vfem_hom_*) against tests/homogenization_cpu.py, the numpy / scipy
restatement that integrates its own K0 and L and solves the assembled periodic matrix by SuperLU.

Cells: ``3d`` is 12 x 10 x 6 on the domain [1.5, 1, 0.5] (non-cubic voxels) with an orthotropic tensor turned about (1, 2, 3) by
0.7 rad, ``2d`` is 16 x 12 on [2, 1] with the anisotropic material file; both with random densities in [0.3, 1], E_min = 1e-3,
gamma = 3.

Tolerances of the solved quantities (TOL_W, TOL_EH): ten times the restatement's own PCG-versus-direct difference at tol = 1e-10
on these two cells, measured on the CPU (relative to the largest entry):
    3d   w 1.53e-10   Eh 1.44e-12   (PCG iterations 161 .. 164)
    2d   w 1.78e-10   Eh 2.33e-12   (PCG iterations 134 .. 137)
The factor ten is for the device's different summation order.  The multi-workgroup cells (no CPU solve) use the 3-D bound.
Measured on an MI355X: 3d w 1.52e-10, Eh 1.28e-12 (161 .. 163 iterations); 2d w 2.34e-10, Eh 3.97e-12 (134 .. 137); apply
1.2e-16 .. 5.8e-16; gradient 6.9e-16 / 9.1e-16; laminate 48 x 20 x 12: 1.9e-15; rolled field 7.3e-13; energy identity 4.0e-13."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import homogenization_cpu as hc
import material_ref as mr

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor, _lib                      # noqa: E402
from ndr_amd import homogenization as hom                      # noqa: E402  (fails here without the feature)
from ndr_amd import pyVoxelFEM as pv                           # noqa: E402

TOL_APPLY = 1e-12                                   # relative to the largest entry: the bound of the existing apply tests
TOL_W = {"3d": 10 * 1.53e-10, "2d": 10 * 1.78e-10}
TOL_EH = {"3d": 10 * 1.44e-12, "2d": 10 * 2.33e-12}
TOL_GRADIENT = 1e-10
SOLVER_TOL = 1e-10


def _rotated_orthotropic():
    t = ElasticityTensor(dim=3)
    t.setOrthotropic(2.0, 1.0, 1.5, 0.2, 0.25, 0.3, 0.5, 0.6, 0.4)
    return t.transform(hc.rotation((1.0, 2.0, 3.0), 0.7))


def _tensor(kind):
    if kind == "rotated":
        return _rotated_orthotropic()
    if kind == "aniso2d":
        return ElasticityTensor(mr.ANISO_2D, dim=2)
    return ElasticityTensor(1.0, 0.3, dim=int(kind[-1]))         # "iso2" / "iso3"


CELLS = {"3d": ((12, 10, 6), (1.5, 1.0, 0.5), "rotated", 11), "2d": ((16, 12), (2.0, 1.0), "aniso2d", 12)}
APPLY_CELLS = {"2x2x2": ((2, 2, 2), (1.0, 0.8, 1.2), "iso3", 21), "2x2": ((2, 2), (1.0, 0.7), "iso2", 22),
               "5x3x7": ((5, 3, 7), (1.0, 0.9, 1.4), "iso3", 23), "3d": CELLS["3d"], "2d": CELLS["2d"]}


def _rho(ne, seed):
    return np.random.default_rng(seed).uniform(0.3, 1.0, size=ne)


def _sim(ne, dom, tensor, rho, gamma=3.0, Emin=1e-3):
    t = pv.TensorProductSimulator([1] * len(ne), [np.zeros(len(ne)), np.array(dom, dtype=np.float64)], list(ne))
    t.ETensor = tensor
    t.E_0, t.E_min, t.gamma = 1.0, Emin, gamma
    t.setElementDensities(np.asarray(rho, dtype=np.float64).reshape(-1))
    return t


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the restatement's direct solution of one cell, computed once and shared (tests leave it unchanged)"""
    ne, dom, kind, seed = APPLY_CELLS[name]
    h = [dom[d] / ne[d] for d in range(len(ne))]
    return hc.homogenize(ne, h, _tensor(kind).D, _rho(ne, seed), 1.0, 1e-3, 3.0)


def _make(name):
    ne, dom, kind, seed = APPLY_CELLS[name]
    return _sim(ne, dom, _tensor(kind), _rho(ne, seed))


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("name", list(APPLY_CELLS))
def test_periodic_apply_matches_assembled_matrix(name):
    """vfem_hom_apply with the simulator's own K0 against the restatement's assembled matrix (its own K0): 2 x 2 (x 2) reaches every
    neighbour twice through the wrap, so duplicates must accumulate; odd unequal extents; non-cubic voxels with a rotated tensor"""
    ne = APPLY_CELLS[name][0]
    ref = _reference(name)
    c = hom._Cell(_make(name))
    assert _relmax(c.K0, ref["K0"]) < 1e-13 and _relmax(c.L, ref["L"]) < 1e-13
    assert _relmax(c.E.cpu().numpy(), ref["E"]) < 1e-15
    W = np.random.default_rng(7).standard_normal((c.S, c.pn * c.N))
    Win = torch.from_numpy(W).cuda()
    Wout = torch.full_like(Win, float("nan"))
    _lib.check(_lib.load().vfem_hom_apply(*c.head(), pv._ptr(Win), pv._ptr(Wout), pv._stream()))
    expect = np.stack([ref["K"] @ w for w in W])
    err = _relmax(Wout.cpu().numpy(), expect)
    print("apply %s: %.2e" % (name, err))
    assert err < TOL_APPLY
    assert np.array_equal(Wout.cpu().numpy()[:, :c.N], W[:, :c.N])               # the pin row is the identity
    assert ne == tuple(c.ne)


@pytest.mark.parametrize("name", list(CELLS))
def test_cell_problems_and_tensor_match_direct_solve(name):
    ne = CELLS[name][0]
    ref = _reference(name)
    sim = _make(name)
    w = hom.solveCellProblems(sim, tol=SOLVER_TOL)
    S, N = len(w), len(ne)
    assert S == (3 if N == 2 else 6) and all(a.shape == (sim.numNodes(), N) for a in w)
    # a condition on the solver: a wrong preconditioner or pin shows as iterations, not as a wrong answer
    _, its_cpu = hc.pcg_columns(ref["K"], ref["b"], N, SOLVER_TOL)
    print("iterations %s: device %s, restatement %s" % (name, hom.last_iterations, its_cpu))
    assert len(hom.last_iterations) == S and all(0 < g <= 2 * c for g, c in zip(hom.last_iterations, its_cpu))
    assert all(r <= SOLVER_TOL for r in hom.last_relative_residuals)
    err_w = _relmax(np.stack(w), hc.to_full(ne, ref["W"]))
    Eh = hom.homogenizedElasticityTensor(w, sim)
    err_e = _relmax(Eh.D, ref["Eh"])
    print("%s: w %.2e, Eh %.2e" % (name, err_w, err_e))
    assert err_w < TOL_W[name]
    assert err_e < TOL_EH[name]
    assert isinstance(Eh, ElasticityTensor) and Eh.dim == N
    # baseCellVolume replaces |Y|
    Eh2 = hom.homogenizedElasticityTensor(w, sim, baseCellVolume=2.0 * float(np.prod(CELLS[name][1])))
    assert _relmax(2.0 * Eh2.D, Eh.D) < 1e-14
    # the energy identity on the device's own fields and moduli (covers the 2-D gradient kernel as well)
    G = hom.homogenizedElasticityTensorGradient(w, sim)
    assert G.shape == (sim.numElements(), S, S)
    assert _relmax(np.einsum("e,eqr->qr", ref["E"] / ref["dE"], G), Eh.D) < TOL_EH[name]


@pytest.mark.parametrize("name", list(CELLS))
def test_gradient_matches_restatement(name):
    """the gradient kernel on the restatement's own (direct) fields"""
    ne = CELLS[name][0]
    ref = _reference(name)
    G = hom.homogenizedElasticityTensorGradient(list(hc.to_full(ne, ref["W"])), _make(name))
    expect = ref["dE"][:, None, None] * ref["G"]
    err = _relmax(G, expect)
    print("gradient %s: %.2e" % (name, err))
    assert err < TOL_GRADIENT
    assert np.array_equal(G, np.transpose(G, (0, 2, 1)))                          # the upper triangle mirrored


def _device_tensor(sim):
    W = hom.solveCellProblems_device(sim, tol=SOLVER_TOL)
    return W, hom.homogenizedElasticityTensor_device(W, sim).D


def test_large_laminate_matches_closed_form():
    """48 x 20 x 12 (45 workgroups), layers normal to x, E = 1 / 0.5, nu = 0.3, gamma = 1, E_min = 0"""
    ne = (48, 20, 12)
    rho = np.ones(ne)
    rho[24:] = 0.5
    sim = _sim(ne, (4.0, 2.0, 1.0), ElasticityTensor(1.0, 0.3, dim=3), rho, gamma=1.0, Emin=0.0)
    _, Eh = _device_tensor(sim)
    lam, mu = hc.lame(1.0, 0.3)
    exact = hc.laminate_closed_form([(lam, mu), (0.5 * lam, 0.5 * mu)], [0.5, 0.5])
    err = _relmax(Eh, exact)
    print("laminate 48x20x12: %.2e, iterations %s" % (err, hom.last_iterations))
    assert err < TOL_EH["3d"]


def test_translation_invariance_and_energy_identity():
    """24 x 20 x 12: Eh of the density field rolled by (3, 5, 2) equals Eh of the original (wrap and pin errors away from the origin
    would show), and sum_e E_e G_e = Eh"""
    ne, dom = (24, 20, 12), (1.2, 1.0, 0.9)
    rho = _rho(ne, 31)
    sim = _sim(ne, dom, _rotated_orthotropic(), rho)
    W, Eh = _device_tensor(sim)
    _, Eh_rolled = _device_tensor(_sim(ne, dom, _rotated_orthotropic(), np.roll(rho, (3, 5, 2), axis=(0, 1, 2))))
    err = _relmax(Eh_rolled, Eh)
    G = hom.homogenizedElasticityTensorGradient_device(W, sim)
    E, dE = hc.moduli(rho, 1.0, 1e-3, 3.0)
    err_id = _relmax(np.einsum("e,eqr->qr", E / dE, G.cpu().numpy()), Eh)
    print("24x20x12: rolled %.2e, energy identity %.2e, iterations %s" % (err, err_id, hom.last_iterations))
    assert err < TOL_EH["3d"]
    assert err_id < TOL_EH["3d"]


def test_two_solves_are_bit_identical():
    W1, E1 = _device_tensor(_make("3d"))
    W2, E2 = _device_tensor(_make("3d"))
    assert torch.equal(W1, W2) and np.array_equal(E1, E2)


def test_errors_and_the_simulator_is_left_alone():
    dom3 = [np.zeros(3), np.ones(3)]
    with pytest.raises(RuntimeError, match="degree-1"):
        hom.solveCellProblems(pv.TensorProductSimulator([2, 2, 2], dom3, [4, 4, 4]))
    with pytest.raises(RuntimeError, match="padding"):
        hom.solveCellProblems(pv.TensorProductSimulator1_1_1(dom3, [4, 4, 4], _element_padding=(1, 1)))
    with pytest.raises(RuntimeError, match="at least 2 elements"):
        hom.solveCellProblems(pv.TensorProductSimulator([1, 1, 1], dom3, [4, 1, 4]))
    # the C boundary refuses the same on its own
    c = hom._Cell(_make("2x2"))
    bad = np.array([2, 1], dtype=np.int64)
    head = (c.N, bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) + c.head()[2:]
    x = torch.zeros(64, dtype=torch.float64, device="cuda")
    assert _lib.load().vfem_hom_apply(*head, pv._ptr(x), pv._ptr(x.clone()), pv._stream()) == 1
    assert b"at least 2 elements" in _lib.load().vfem_last_error()

    sim = pv.TensorProductSimulator([1, 1, 1], [np.zeros(3), np.array([2.0, 1.0, 1.0])], [16, 8, 8])
    clamp = np.zeros((sim.numNodes(), 3), dtype=bool)
    clamp[:81] = True                                                            # the face x = 0 clamped
    sim.dirichletMask = clamp
    sim.E_min = 1e-3
    sim.setElementDensities(_rho((16, 8, 8), 41).reshape(-1))
    rho = sim.getDensities()
    u = np.random.default_rng(2).standard_normal((sim.numNodes(), 3))
    Ku = sim.applyK(u)                                                           # (reads the Dirichlet mask held on the device)
    with pytest.raises(RuntimeError, match=r"no convergence in 3 iterations.*\|r\|/\|b\| = "):
        hom.solveCellProblems(sim, maxIter=3)
    assert hom.last_iterations == [3] * 6 and all(r > 1e-10 for r in hom.last_relative_residuals)
    w = hom.solveCellProblems(sim)
    assert np.array_equal(sim.dirichletMask, clamp)
    assert np.array_equal(rho, sim.getDensities()) and np.array_equal(Ku, sim.applyK(u))
    assert np.abs(np.stack(w)[:, 0]).max() == 0.0                                # pinned, Dirichlet conditions ignored


def test_homogenised_tensor_feeds_a_macro_scale_simulator():
    sim = _make("3d")
    Eh = hom.homogenizedElasticityTensor(hom.solveCellProblems(sim), sim)
    sym = ElasticityTensor.fromD(0.5 * (Eh.D + Eh.D.T))
    assert sym.isPositiveDefinite()
    macro = pv.TensorProductSimulator([1, 1, 1], [np.zeros(3), np.ones(3)], [6, 5, 4])
    macro.ETensor = sym
    macro.setUniformDensities(1.0)
    assert np.array_equal(macro.ETensor.D, sym.D)
    u = np.random.default_rng(3).standard_normal((macro.numNodes(), 3))
    Ku = macro.applyK(u)
    assert np.all(np.isfinite(Ku)) and float(np.sum(u * Ku)) > 0.0
    # an isotropic projection of it is accepted as well
    macro.ETensor = hom.closestIsotropicTensor(sym)
    assert np.all(np.isfinite(macro.applyK(u)))
