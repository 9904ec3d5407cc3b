"""-m gpu: design of periodic cells on the device (ndr_amd.microstructure): the contracted tensor gradient
(vfem_hom_tensor_gradient_contract), the periodic box filter (vfem_box_filter_periodic), the objective J = - Cs : Eh in the package's
OC loop and the autograd node, against tests/microstructure_cpu.py.

Bounds.  Every figure named "restatement" was measured on the CPU with tests/microstructure_cpu.py, its PCG against its direct solve.
  Contraction against einsum("qr,eqr->e", C, G) of vfem_hom_tensor_gradient: 1e-12 of the largest |g| (the same fp64 sums in another
    order: the bound k_hom_apply is held to).  C and C^T, and two runs, agree bit for bit; an antisymmetric C gives exactly 0.
  Filter values 1e-13 absolute (at most 343 additions of values <= 1 and one division: about 4e-14); x . F y = y . F x and
    mean(F x) = mean(x) to 1e-12 relative.
  Objective at tol = 1e-10, random densities in [0.05, 1]: the restatement's PCG differs from its direct solve by
      16 x 12    block Jacobi  J 2.34e-11, gradient 2.61e-10 of its largest entry;  multigrid  J 5.03e-12, gradient 1.81e-10
      8 x 8 x 6  block Jacobi  J 1.33e-12, gradient 6.91e-11;                        multigrid  J 4.10e-13, gradient 8.76e-11
    the bounds are ten times these (J never below 1e-12, the order-of-summation bound above).
  OC loop at tol = 1e-10, block Jacobi: the restatement's PCG trajectory differs from its direct-solve trajectory by 6.27e-11 in J
    (relative) and 1.34e-11 in the design over 12 steps on 16 x 12, by 7.14e-14 and 7.43e-13 over 6 steps on 8 x 8 x 6; the bounds are
    ten times these, J never below 1e-12.
  Autograd, loss = |Eh - T|^2 / |T|^2 with T isotropic (E = 0.3, nu = 0.3), tol = 1e-10: the restatement's PCG gradient differs from
    its direct-solve gradient by 2.23e-10 (16 x 12, float64 densities), 2.38e-10 (float32), 5.65e-11 and 5.65e-11 (8 x 8 x 6) of the
    largest entry, its loss by 5.53e-12, 6.85e-12, 1.98e-12 and 2.06e-12 relative; bounds ten times these, plus half a float32 unit
    in the last place of each entry where the result is float32.
  Central difference of the loss along one random direction, step 1e-5, solves to 1e-12: the restatement's PCG mismatch is 2.18e-8
    (16 x 12) and 1.79e-10 (8 x 8 x 6) relative; bounds ten times these, not below 1e-7.

Measured on an MI355X:
  contraction 1.8e-16 .. 5.0e-16, C / C^T / second run bit-identical, antisymmetric C exactly 0; filter values 0 (the restatement
  adds in the same order), self-adjointness at most 7.7e-16, mean at most 2.2e-16.
  objective: 16 x 12 J 1.81e-11 (block Jacobi, 183 182 182 iterations) / 5.04e-12 (multigrid, 29 29 29), gradient 2.20e-10 / 1.81e-10;
    8 x 8 x 6 J 1.38e-12 / 4.11e-13, gradient 6.90e-11 / 8.76e-11 (108 .. 113 and 18 .. 19 iterations).
  OC loop: 16 x 12 J -0.3456403288 -> -0.3595904656, against the restatement J 6.20e-11, design 1.31e-11; 8 x 8 x 6
    J -0.9423126777 -> -0.9438163403, J 6.56e-14, design 7.47e-13; the clipped filter moves the final design's mean by 1.14e-4 / 6.03e-4.
  autograd: gradient 1.78e-10 (16 x 12) and 5.65e-11 (8 x 8 x 6) of the largest entry, float32 within its rounding; central difference
    2.28e-8 / 3.03e-10; peak of torch's device memory in backward 2048 .. 4608 bytes against 13824 / 110592 of the block array.
  Against the parent commit every test fails: the module and the two entry points do not exist.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import design_update_cpu as du
import homogenization_cpu as hc
import homogenization_mg_cpu as mg
import microstructure_cpu as ms

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor, _lib                      # noqa: E402
from ndr_amd import homogenization as hom                      # noqa: E402
from ndr_amd import microstructure as mic                      # noqa: E402
from ndr_amd import pyVoxelFEM as pv                           # noqa: E402
from test_gpu_homogenization import _rotated_orthotropic       # noqa: E402
from test_gpu_homogenization_blocks import _make as _make_block                                  # noqa: E402
from test_gpu_homogenization_mg import _relmax, _sim            # noqa: E402

TOL_CONTRACT = 1e-12
TOL_FILTER, TOL_FILTER_IDENTITY = 1e-13, 1e-12
SOLVER_TOL = 1e-10
FLOOR = 1e-12
TOL_OBJECTIVE = {("16x12", "jacobi"): (10 * 2.34e-11, 10 * 2.61e-10), ("16x12", "multigrid"): (10 * 5.03e-12, 10 * 1.81e-10),
                 ("8x8x6", "jacobi"): (10 * 1.33e-12, 10 * 6.91e-11), ("8x8x6", "multigrid"): (max(10 * 4.10e-13, FLOOR), 10 * 8.76e-11)}
TOL_TRAJECTORY = {"16x12": (10 * 6.27e-11, 10 * 1.34e-11), "8x8x6": (max(10 * 7.14e-14, FLOOR), 10 * 7.43e-13)}
TOL_AUTOGRAD = {("16x12", torch.float64): 10 * 2.23e-10, ("16x12", torch.float32): 10 * 2.38e-10,
                ("8x8x6", torch.float64): 10 * 5.65e-11, ("8x8x6", torch.float32): 10 * 5.65e-11}
TOL_LOSS = {("16x12", torch.float64): 10 * 5.53e-12, ("16x12", torch.float32): 10 * 6.85e-12,
            ("8x8x6", torch.float64): 10 * 1.98e-12, ("8x8x6", torch.float32): 10 * 2.06e-12}
FD_STEP, FD_SOLVER_TOL = 1e-5, 1e-12
TOL_FD = {"16x12": max(10 * 2.18e-8, 1e-7), "8x8x6": max(10 * 1.79e-10, 1e-7)}
DESIGN_CELLS = {"16x12": ((16, 12), ms.BULK_2D, 12, 81), "8x8x6": ((8, 8, 6), ms.BULK_3D, 6, 82)}      # elements, weights, OC steps, seed


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ---- the contracted gradient ----

def _contraction_sim(name):
    if name in mg.BLOCK_CELLS:
        return _make_block(name)
    ne, dom, tensor, seed = {"2x2": ((2, 2), (1.0, 0.7), ElasticityTensor(1.0, 0.3, dim=2), 21),
                             "2x2x2": ((2, 2, 2), (1.0, 0.8, 1.3), ElasticityTensor(1.0, 0.3, dim=3), 22),
                             "5x3x7": ((5, 3, 7), (1.5, 1.0, 0.5), ElasticityTensor(1.0, 0.3, dim=3), 23),
                             "5x3x7-rotated": ((5, 3, 7), (1.5, 1.0, 0.5), _rotated_orthotropic(), 24)}[name]
    return _sim(ne, dom, tensor, np.random.default_rng(seed).uniform(0.05, 1.0, size=ne))


def _contract(c, Wp, C, scaled):
    g = torch.full((c.pn,), float("nan"), dtype=torch.float64, device="cuda")
    C = np.ascontiguousarray(C, dtype=np.float64)
    _lib.check(_lib.load().vfem_hom_tensor_gradient_contract(*c.head(), _p(Wp), c.cell_volume, _p(c.dE) if scaled else None,
                                                             hom._dp(C), _p(g), pv._stream()))
    return g


def _blocks(c, Wp, scaled):
    G = torch.empty((c.pn, c.S, c.S), dtype=torch.float64, device="cuda")
    _lib.check(_lib.load().vfem_hom_tensor_gradient(*c.head(), _p(Wp), c.cell_volume, _p(c.dE) if scaled else None, _p(G),
                                                    pv._stream()))
    return G.cpu().numpy()


@pytest.mark.parametrize("name", ["2x2", "2x2x2", "5x3x7", "5x3x7-rotated", "2d-blocks", "3d-blocks"])
@pytest.mark.parametrize("scaled", [True, False], ids=["dE", "dE-null"])
def test_contraction_equals_the_contracted_blocks(name, scaled):
    c = hom._Cell(_contraction_sim(name))
    rng = np.random.default_rng(31)
    Wp = torch.from_numpy(rng.standard_normal((c.S, c.pn, c.N))).cuda()          # random fields, not solutions
    C = rng.standard_normal((c.S, c.S))                                           # not symmetric
    g = _contract(c, Wp, C, scaled)
    expect = np.einsum("qr,eqr->e", C, _blocks(c, Wp, scaled))
    err = _relmax(g.cpu().numpy(), expect)
    print("contraction %s, %s: %.2e of max|g| = %.3e" % (name, "dE" if scaled else "dE = NULL", err, np.abs(expect).max()))
    assert err < TOL_CONTRACT
    assert torch.equal(g, _contract(c, Wp, C, scaled))                            # run to run
    assert torch.equal(g, _contract(c, Wp, C.T, scaled))                          # only the symmetric part acts
    anti = _contract(c, Wp, C - C.T, scaled)
    assert torch.equal(anti, torch.zeros_like(anti))
    # a sparse weight matrix (pairs with weight zero are skipped)
    bulk = np.zeros((c.S, c.S))
    bulk[:c.N, :c.N] = 1.0
    err = _relmax(_contract(c, Wp, bulk, scaled).cpu().numpy(), np.einsum("qr,eqr->e", bulk, _blocks(c, Wp, scaled)))
    assert err < TOL_CONTRACT


def test_contraction_refuses_bad_arguments():
    c = hom._Cell(_contraction_sim("2x2"))
    Wp = torch.zeros((c.S, c.pn, c.N), dtype=torch.float64, device="cuda")
    g = torch.zeros(c.pn, dtype=torch.float64, device="cuda")
    lib = _lib.load()
    C = np.eye(c.S)
    bad = C.copy()
    bad[1, 2] = np.nan
    assert lib.vfem_hom_tensor_gradient_contract(*c.head(), _p(Wp), c.cell_volume, None, hom._dp(bad), _p(g), pv._stream()) == 1
    assert "not finite" in lib.vfem_last_error().decode()
    assert lib.vfem_hom_tensor_gradient_contract(*c.head(), _p(Wp), c.cell_volume, None, None, _p(g), pv._stream()) == 1
    assert lib.vfem_hom_tensor_gradient_contract(*c.head(), None, c.cell_volume, None, hom._dp(C), _p(g), pv._stream()) == 1
    assert lib.vfem_hom_tensor_gradient_contract(*c.head(), _p(Wp), c.cell_volume, None, hom._dp(C), None, pv._stream()) == 1
    assert lib.vfem_hom_tensor_gradient_contract(*c.head(), _p(Wp), 0.0, None, hom._dp(C), _p(g), pv._stream()) == 1
    assert "cell volume" in lib.vfem_last_error().decode()
    with pytest.raises(ValueError):
        hom.homogenizedElasticityTensorGradientContracted_device(torch.zeros((c.S, 9, c.N)), _contraction_sim("2x2"), np.eye(c.S + 1))


def test_contracted_gradient_of_the_public_interface():
    sim = _contraction_sim("5x3x7-rotated")
    w = hom.solveCellProblems_device(sim, tol=SOLVER_TOL)
    C = np.random.default_rng(32).standard_normal((6, 6))
    G = hom.homogenizedElasticityTensorGradient(list(w.cpu().numpy()), sim)
    g = hom.homogenizedElasticityTensorGradientContracted(list(w.cpu().numpy()), sim, C)
    assert g.shape == (sim.numElements(),)
    assert _relmax(g, np.einsum("qr,eqr->e", C, G)) < TOL_CONTRACT
    assert np.array_equal(g, hom.homogenizedElasticityTensorGradientContracted_device(w, sim, torch.from_numpy(C)).cpu().numpy())


# ---- the periodic filter ----

FILTER_CASES = [((4, 4), 2), ((4, 4), 3), ((5, 3, 7), 1), ((3, 5, 2), 2), ((72, 64), 3), ((28, 24, 28), 2),
                ((1032, 1024), 1)]                      # the last: 4129 workgroups for a grid capped at 4096, a ragged second pass


def _filter(grid, r):
    f = mic.PeriodicSmoothingFilter()
    f.radius = r
    f._set_grid(grid)
    return f


@pytest.mark.parametrize("grid, r", FILTER_CASES)
def test_periodic_filter_matches_the_restatement(grid, r):
    n = int(np.prod(grid))
    rng = np.random.default_rng(41)
    x, y = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    f = _filter(grid, r)
    Fx, Fy = f.apply(x), f.apply(y)
    err = float(np.abs(Fx - ms.periodic_box_filter(x, grid, r)).max())
    adj = abs(x @ Fy - y @ Fx) / abs(x @ Fy)
    mean = abs(Fx.mean() - x.mean()) / x.mean()
    print("periodic filter %s r = %d: values %.2e, self-adjoint %.2e, mean %.2e" % ("x".join(map(str, grid)), r, err, adj, mean))
    assert err <= TOL_FILTER
    assert adj <= TOL_FILTER_IDENTITY and mean <= TOL_FILTER_IDENTITY
    assert np.array_equal(f.backprop(x, y), Fx)                                   # its own transpose: the same launch


def test_periodic_filter_refuses_bad_arguments():
    lib = _lib.load()
    x = torch.zeros(16, dtype=torch.float64, device="cuda")
    out = torch.zeros_like(x)
    n = (ctypes.c_int64 * 3)(4, 4, 1)
    assert lib.vfem_box_filter_periodic(n, -1, _p(x), _p(out), pv._stream()) == 1
    assert lib.vfem_box_filter_periodic(n, 1, _p(x), _p(x), pv._stream()) == 1
    assert lib.vfem_box_filter_periodic(n, 1, None, _p(out), pv._stream()) == 1
    assert lib.vfem_box_filter_periodic(n, 1 << 20, _p(x), _p(out), pv._stream()) == 1
    assert "neighbourhood too large" in lib.vfem_last_error().decode()
    assert lib.vfem_box_filter_periodic((ctypes.c_int64 * 3)(4, 0, 4), 1, _p(x), _p(out), pv._stream()) == 1
    f = _filter((4, 4), 1)
    with pytest.raises(RuntimeError, match="does not match the grid"):
        f.apply(np.zeros(15))


# ---- the objective ----

def _design_sim(name, rho):
    ne = DESIGN_CELLS[name][0]
    return _sim(ne, [1.0] * len(ne), ElasticityTensor(1.0, 0.3, dim=len(ne)), rho, ms.GAMMA, ms.EMIN)


def _random_densities(name):
    ne, _, _, seed = DESIGN_CELLS[name]
    return np.random.default_rng(seed).uniform(0.05, 1.0, int(np.prod(ne)))


@functools.lru_cache(maxsize=None)
def _objective_cpu(name):
    """(J, dJ/drho) of the restatement's direct solve at the random densities, computed once and left unchanged"""
    ne, h, D = ms.standard_cell(DESIGN_CELLS[name][0])
    return ms.objective(ne, h, D, _random_densities(name), DESIGN_CELLS[name][1])


@pytest.mark.parametrize("name", list(DESIGN_CELLS))
@pytest.mark.parametrize("preconditioner", ["jacobi", "multigrid"])
def test_objective_matches_the_direct_solve(name, preconditioner):
    rho = _random_densities(name)
    weights = DESIGN_CELLS[name][1]
    sim = _design_sim(name, np.full(rho.size, 0.5))
    obj = mic.HomogenizedTensorObjective(sim, weights + np.triu(np.ones_like(weights), 1) - np.tril(np.ones_like(weights), -1),
                                         tol=SOLVER_TOL, preconditioner=preconditioner, skipSolve=True)    # + an antisymmetric part
    assert np.array_equal(obj.weights, weights)
    with pytest.raises(RuntimeError, match="updateCache"):
        obj.evaluate()
    J = obj.evaluate(rho)                                                          # sets the densities and solves
    assert np.array_equal(sim.getDensities(), rho)
    assert len(hom.last_iterations) == weights.shape[0] and min(hom.last_iterations) > 0
    g = obj.gradient()
    J_cpu, g_cpu = _objective_cpu(name)
    err_J, err_g = abs(J - J_cpu) / abs(J_cpu), _relmax(g, g_cpu)
    print("objective %s, %s: J = %.10f, error %.2e, gradient %.2e of max; iterations %s"
          % (name, preconditioner, J, err_J, err_g, hom.last_iterations))
    tol_J, tol_g = TOL_OBJECTIVE[(name, preconditioner)]
    assert err_J <= tol_J and err_g <= tol_g
    assert np.all(g <= 0.0)
    assert J == -float(np.sum(weights * obj.tensor().D))
    assert torch.equal(obj.gradient_device().cpu(), torch.from_numpy(g))
    Eh = hom.homogenizedElasticityTensor_device(obj.w_device(), sim).D
    assert np.array_equal(Eh, obj.tensor().D)


def test_objective_solves_on_construction_and_refuses_indefinite_weights():
    name = "16x12"
    sim = _design_sim(name, _random_densities(name))
    obj = mic.HomogenizedTensorObjective(sim, ms.BULK_2D, tol=SOLVER_TOL)
    J_cpu, _ = _objective_cpu(name)
    assert abs(obj.evaluate() - J_cpu) <= TOL_OBJECTIVE[(name, "jacobi")][0] * abs(J_cpu)
    with pytest.raises(ValueError, match="positive semidefinite"):
        mic.HomogenizedTensorObjective(sim, np.diag([1.0, -1.0, 0.0]), skipSolve=True)
    with pytest.raises(ValueError, match="positive semidefinite"):
        mic.HomogenizedTensorObjective(sim, [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], skipSolve=True)   # Eh_xxyy alone
    with pytest.raises(ValueError, match="3 x 3"):
        mic.HomogenizedTensorObjective(sim, ms.BULK_3D, skipSolve=True)


# ---- the design loop through the existing classes ----

@functools.lru_cache(maxsize=None)
def _trajectory_cpu(name):
    ne, weights, steps, _ = DESIGN_CELLS[name]
    return ms.trajectory(ne, weights, steps)


def _problem(name, smoothing_filter):
    ne, weights, _, _ = DESIGN_CELLS[name]
    sim = _design_sim(name, np.full(int(np.prod(ne)), ms.VOLUME_FRACTION))
    obj = mic.HomogenizedTensorObjective(sim, weights, tol=SOLVER_TOL, skipSolve=True)
    smoothing_filter.radius = ms.RADIUS
    return pv.TopologyOptimizationProblem(sim, obj, [pv.TotalVolumeConstraint(ms.VOLUME_FRACTION)], [smoothing_filter]), obj


@pytest.mark.parametrize("name", list(DESIGN_CELLS))
def test_oc_loop_lowers_the_objective_and_follows_the_restatement(name):
    ne, _, steps, _ = DESIGN_CELLS[name]
    problem, obj = _problem(name, mic.PeriodicSmoothingFilter())
    problem.setVars(ms.standard_design(ne))
    oc = pv.OCOptimizer(problem)
    J = [problem.evaluateObjective()]
    for _ in range(steps):
        oc.step(ms.MOVE, ms.CTOL)
        J.append(problem.evaluateObjective())
        assert abs(problem.evaluateConstraints()[0]) <= ms.CTOL
    J, x = np.array(J), problem.getVars()
    J_cpu, x_cpu = _trajectory_cpu(name)
    err_J, err_x = float(np.abs((J - J_cpu) / J_cpu).max()), float(np.abs(x - x_cpu).max())
    print("OC loop %s: J = %s; against the restatement: J %.2e, design %.2e" % (name, " ".join("%.10f" % v for v in J), err_J, err_x))
    assert np.all(np.diff(J) < 0.0)
    tol_J, tol_x = TOL_TRAJECTORY[name]
    assert err_J <= tol_J and err_x <= tol_x
    assert obj.tensor().dim == len(ne)
    # the periodic filter keeps the design's volume; the clipped one does not, by far more than the OC step resolves
    clipped, _ = _problem(name, pv.SmoothingFilter())
    clipped.setVars(x)
    drift = abs(clipped.getDensities().mean() - x.mean())
    kept = abs(problem.getDensities().mean() - x.mean())
    print("volume change of the final design: periodic filter %.2e, clipped filter %.2e" % (kept, drift))
    assert kept <= TOL_FILTER_IDENTITY * x.mean()
    assert drift > 10 * ms.CTOL * ms.VOLUME_FRACTION
    assert abs(drift - abs(du.box_filter(x, ne, ms.RADIUS).mean() - x.mean())) <= 1e-12


# ---- the autograd node ----

def _target(N):
    return hc.isotropic_D(0.3, 0.3, N)


def _loss_cpu(name, rho, **how):
    """(loss, d loss / d rho) of the restatement"""
    ne, h, D = ms.standard_cell(DESIGN_CELLS[name][0])
    T = _target(len(ne))
    Eh, _ = ms.tensor_and_gradient(ne, h, D, rho, np.zeros_like(T), **how)
    _, g = ms.tensor_and_gradient(ne, h, D, rho, 2.0 * (Eh - T) / np.sum(T * T), **how)
    return float(np.sum((Eh - T) ** 2) / np.sum(T * T)), g


def _loss(Eh, T):
    return ((Eh - T) ** 2).sum() / (T ** 2).sum()


@pytest.mark.parametrize("name", list(DESIGN_CELLS))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_autograd_backward_matches_the_direct_solve(name, dtype):
    ne = DESIGN_CELLS[name][0]
    S = 3 if len(ne) == 2 else 6
    rho = torch.from_numpy(_random_densities(name)).to(dtype).cuda().requires_grad_(True)
    sim = _design_sim(name, np.full(rho.numel(), 0.5))
    T = torch.from_numpy(_target(len(ne))).cuda()
    Eh = mic.homogenizedTensor(rho, sim, tol=SOLVER_TOL)
    assert Eh.dtype == torch.float64 and tuple(Eh.shape) == (S, S) and Eh.is_cuda
    loss = _loss(Eh, T)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert rho.grad.dtype == dtype and rho.grad.shape == rho.shape
    loss_cpu, g_cpu = _loss_cpu(name, rho.detach().cpu().double().numpy())
    g = rho.grad.cpu().double().numpy()
    rounding = 2.0 ** -24 * np.abs(g_cpu) if dtype == torch.float32 else 0.0
    excess = float((np.abs(g - g_cpu) - rounding).max() / np.abs(g_cpu).max())
    print("autograd %s %s: loss %.10f (restatement %.10f), gradient %.2e of max beyond rounding, peak %d bytes of %d"
          % (name, dtype, float(loss.detach()), loss_cpu, excess, peak, rho.numel() * S * S * 8))
    assert abs(float(loss.detach()) - loss_cpu) <= TOL_LOSS[(name, dtype)] * abs(loss_cpu)
    assert excess <= TOL_AUTOGRAD[(name, dtype)]
    assert peak < rho.numel() * S * S * 8                                         # the [numElements, S, S] array is not formed


@pytest.mark.parametrize("name", list(DESIGN_CELLS))
def test_autograd_backward_matches_a_central_difference(name):
    ne = DESIGN_CELLS[name][0]
    base = _random_densities(name)
    d = np.random.default_rng(DESIGN_CELLS[name][3] + 10).standard_normal(base.size)
    sim = _design_sim(name, np.full(base.size, 0.5))
    T = torch.from_numpy(_target(len(ne))).cuda()

    def loss_at(values, grad):
        rho = torch.from_numpy(values).cuda().requires_grad_(grad)
        return rho, _loss(mic.homogenizedTensor(rho, sim, tol=FD_SOLVER_TOL), T)

    rho, loss = loss_at(base, True)
    loss.backward()
    analytic = float(rho.grad.cpu().numpy() @ d)
    fd = (float(loss_at(base + FD_STEP * d, False)[1]) - float(loss_at(base - FD_STEP * d, False)[1])) / (2.0 * FD_STEP)
    err = abs(fd - analytic) / abs(analytic)
    print("autograd central difference %s: %.10e against %.10e, relative %.2e" % (name, fd, analytic, err))
    assert err <= TOL_FD[name]
