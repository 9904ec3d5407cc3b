"""-m gpu: natural frequencies on the device (ndr_amd.modal, vfem_modal_*, vfem_block_*): the mass operator, the Gram matrix and the
linear combination of tall blocks, the block eigensolver, the mean-eigenvalue objective, its autograd node and its use as an MMA
constraint, against tests/modal_cpu.py.

Bounds.  Every figure named "restatement" was measured on the CPU with tests/modal_cpu.py (tests/test_modal_cpu.py prints them).
  Mass apply: 1e-12 of the largest entry (TOL_KERNEL): an entry is a sum of at most 27 x 8 products.
  Gram: 1e-12 sum |a_i b_i| per entry.  The longest chain of additions behind an entry has L = ceil(n / (1024 x 256)) + 22 terms
    (the thread's own rows, 6 shuffle steps and 3 additions across the block's waves, then 4 + 6 + 3 over the 1024 partials): 24 at
    n = 300 001, so that L 2^-53 = 2.7e-15 stays below the bound; the reference is numpy in extended precision.
  Combine: 1e-14 sum_i |C_ij| |A_i| per entry (24 fused multiply-adds: 24 x 2^-53 = 2.7e-15).
  eigenmodes at tol 1e-9, four modes, two guard columns: the restatement's LOBPCG differs from scipy.linalg.eigh by 1.8e-14 (16 x 12)
    and 4.2e-14 (8 x 8 x 6) of the largest of the four eigenvalues, by 1.2e-15 / 2.0e-15 in |phi_ref^T M phi| and by 2.3e-15 / 3.8e-15
    in Phi^T M Phi - I: ten times these is below the floor 1e-12.  It takes 14 iterations on either fixture: the cap is 28.
  Objective at tol 1e-9: the restatement's LOBPCG differs from eigh by J 5.0e-13 / 1.7e-13 (relative) and gradient 1.8e-12 / 3.8e-12
    of the largest entry; the bounds are ten times these.
  Central difference of J along one random direction, step 1e-5, solves to 1e-12: the restatement's mismatch (dense solves) is
    6.57e-8 (16 x 12) and 9.19e-9 (8 x 8 x 6); bounds ten times these, not below 1e-7.

Measured on an MI355X:
  mass apply 1.5e-16 .. 3.8e-16 of the largest entry over the sixteen cases; off-line buffers and a second run bit-identical.
  Gram 3.8e-19 / 1.5e-18 / 2.1e-18 of sum |a b| (k = 1 / 5 / 24), combine 1.1e-16 / 3.8e-16 / 6.2e-16 of sum |C| |A|; run twice: the same bits.
  eigenmodes 16 x 12 (band factor): 15 iterations, eigenvalues 6.2e-14, 1 - overlap 1.1e-15, Phi^T M Phi - I 1.6e-15, residuals 9.9e-10;
    8 x 8 x 6 (band factor): 13 iterations, 7.2e-14, 1.0e-15, 8.9e-16, 1.9e-10; 8 x 8 x 6 (2-level V-cycle): 17 iterations, 5.7e-14,
    6.7e-16, 1.1e-15, 4.8e-10; P dropped 2 / 1 / 1 times; every warm start from the converged block: 0 iterations.
  objective: J 7.7e-13 / 4.8e-14, gradient 4.6e-12 / 3.0e-12 (16 x 12 / 8 x 8 x 6); central difference 1.1e-10 / 3.9e-9.
  three MMA steps on 16 x 12: J 51.596 -> 31.386 under the bound 54.176, the restatement at the final densities within 3.0e-13.
  The whole file runs in under 7 s (2 s of it the extended-precision reference of the 24-column blocks).
  Against the parent commit every test fails at import: the module and the entry points do not exist.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import modal_cpu as mc
import stress_cpu as sc

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor, _lib, mma, modal         # noqa: E402
from ndr_amd import pyVoxelFEM as pv                           # noqa: E402

TOL_KERNEL = 1e-12
FLOOR = 1e-12
TOL_SOLVE = 1e-9
TOL_LAMBDA = {"16x12": max(10 * 1.8e-14, FLOOR), "8x8x6": max(10 * 4.2e-14, FLOOR)}
TOL_OVERLAP = {"16x12": max(10 * 1.2e-15, FLOOR), "8x8x6": max(10 * 2.0e-15, FLOOR)}
MAX_ITERATIONS = 2 * 14
TOL_J = {"16x12": max(10 * 5.0e-13, FLOOR), "8x8x6": max(10 * 1.7e-13, FLOOR)}
TOL_GRADIENT = {"16x12": max(10 * 1.8e-12, FLOOR), "8x8x6": max(10 * 3.8e-12, FLOOR)}
FD_STEP = 1e-5
TOL_FD = {"16x12": max(10 * 6.57e-8, 1e-7), "8x8x6": max(10 * 9.19e-9, 1e-7)}

# 40 x 37 and 12 x 10 x 9 span several workgroups of the node kernel (64 lanes along the last axis by 4 rows, one block per layer
# of axis 0 in 3-D): 41 x 38 nodes are 11 blocks of rows, 13 x 11 x 10 nodes are 13 layers of 3 blocks; no extent is a multiple of 4
SHAPES = [(7, 5), (40, 37), (6, 4, 5), (12, 10, 9)]
EDGES = {2: (0.5, 0.3), 3: (0.5, 0.3, 0.7)}
N_BLOCK = 300001


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _name(ne):
    return "x".join(map(str, ne))


def _dev(a, off=False):
    """a device copy; off: a view that starts 8 bytes off a 16-byte line"""
    a = np.ascontiguousarray(a)
    if not off:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    view = buf[1:].reshape(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8
    return view


def _head(ne, h):
    n, hh = np.asarray(ne, dtype=np.int64), np.ascontiguousarray(h, dtype=np.float64)
    return (len(ne), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(hh)), (n, hh)           # (the arrays stay alive with the tuple)


# ---- the mass operator ----

@functools.lru_cache(maxsize=None)
def _mass_case(ne):
    N = len(ne)
    rng = np.random.default_rng(200 + int(np.prod(ne)))
    nn = sc.num_nodes(ne)
    m = rng.uniform(0.05, 1.0, size=int(np.prod(ne)))
    X = rng.standard_normal((3, nn * N))
    fixed = rng.uniform(size=(nn, N)) < 0.2
    bits = np.zeros(nn, dtype=np.uint8)
    for c in range(N):
        bits |= fixed[:, c].astype(np.uint8) << c
    h = EDGES[N]
    return dict(ne=ne, N=N, h=h, m=m, X=X, fixed=fixed, bits=bits, M=mc.assemble_mass(ne, h, m), MP=mc.assemble_mass(ne, h, m, fixed))


def _run_mass(c, ncols, masked, off=False):
    args, keep = _head(c["ne"], c["h"])
    X, m = _dev(c["X"][:ncols], off), _dev(c["m"], off)
    Y = _dev(np.full((ncols, c["X"].shape[1]), np.nan), off)
    mask = torch.from_numpy(c["bits"]).cuda() if masked else None
    _lib.check(_lib.load().vfem_modal_mass_apply(*args, _p(m), _p(mask), ncols, _p(X), _p(Y), pv._stream()))
    torch.cuda.synchronize()
    return Y


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_mass_apply_matches_the_assembled_matrix(ne, ncols, masked):
    c = _mass_case(ne)
    Y = _run_mass(c, ncols, masked)
    ref = ((c["MP"] if masked else c["M"]) @ c["X"][:ncols].T).T
    err = np.abs(Y.cpu().numpy() - ref).max() / np.abs(ref).max()
    print("mass apply %s, %d columns, %s: %.2e" % (_name(ne), ncols, "masked" if masked else "free", err))
    assert err < TOL_KERNEL
    if masked:
        assert not Y.cpu().numpy()[:, c["fixed"].reshape(-1)].any()
    assert torch.equal(_run_mass(c, ncols, masked), Y)                                 # run to run


@pytest.mark.parametrize("ne", [(40, 37), (12, 10, 9)], ids=_name)
def test_mass_apply_on_buffers_8_bytes_off_a_16_byte_line(ne):
    c = _mass_case(ne)
    assert torch.equal(_run_mass(c, 3, True, off=True), _run_mass(c, 3, True))


def test_public_mass_operator():
    sim = _simulator("8x8x6")
    ne, h, D, rho, fixed = mc.case("8x8x6")
    mass = dict(massDensity=2.0, massExponent=1.0, lowDensityCut=0.5)
    X = np.random.default_rng(5).standard_normal((2, sim.numNodes(), 3))
    m = mc.mass_multipliers(rho, **mass)[0]
    ref = (mc.assemble_mass(ne, h, m, fixed) @ X.reshape(2, -1).T).T
    assert np.abs(modal.applyM(sim, X, mass).reshape(2, -1) - ref).max() < TOL_KERNEL * np.abs(ref).max()
    one = modal.applyM_device(sim, torch.from_numpy(X[0]).cuda(), mass, project=False)
    assert one.shape == (sim.numNodes(), 3)
    ref = mc.assemble_mass(ne, h, m) @ X[0].reshape(-1)
    assert np.abs(one.cpu().numpy().reshape(-1) - ref).max() < TOL_KERNEL * np.abs(ref).max()
    got, dgot = modal.massMultipliers(sim, **mass)
    want, dwant = mc.mass_multipliers(rho, **mass)
    assert np.abs(got.cpu().numpy() - want).max() < 1e-14 * want.max() and np.abs(dgot.cpu().numpy() - dwant).max() < 1e-14 * dwant.max()


# ---- Gram matrix and linear combination ----

@functools.lru_cache(maxsize=None)
def _blocks(k):
    rng = np.random.default_rng(300 + k)
    A, B, C = rng.standard_normal((k, N_BLOCK)), rng.standard_normal((k, N_BLOCK)), rng.standard_normal((k, k))
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    G = np.array([[np.sum(Al[i] * Bl[j]) for j in range(k)] for i in range(k)])
    Gabs = np.abs(A) @ np.abs(B).T
    comb = np.array([np.sum(C[:, j].astype(np.longdouble)[:, None] * Al, axis=0) for j in range(k)])
    cabs = np.abs(C).T @ np.abs(A)
    return dict(A=A, B=B, C=C, G=G, Gabs=Gabs, comb=comb, cabs=cabs)


@pytest.mark.parametrize("k", [1, 5, 24])
def test_gram_matches_numpy(k):
    c = _blocks(k)
    chain = -(-N_BLOCK // (1024 * 256)) + 22
    assert chain * 2.0 ** -53 < 1e-12
    A, B = _dev(c["A"]), _dev(c["B"])
    lib = _lib.load()
    out = []
    for _ in range(2):
        G = torch.full((k, k), float("nan"), dtype=torch.float64, device="cuda")
        host = np.full((k, k), np.nan)
        _lib.check(lib.vfem_block_gram(N_BLOCK, k, _p(A), k, _p(B), _p(G), _dp(host), pv._stream()))
        assert np.array_equal(G.cpu().numpy(), host)
        out.append(host)
    err = (np.abs(out[0].astype(np.longdouble) - c["G"]).astype(np.float64) / c["Gabs"]).max()
    print("gram k = %d: %.2e of sum |a b|" % (k, err))
    assert err < 1e-12
    assert np.array_equal(out[0], out[1])                                              # bit for bit
    host = np.full((k, k), np.nan)                                                     # no device output asked for
    _lib.check(lib.vfem_block_gram(N_BLOCK, k, _p(A), k, _p(B), None, _dp(host), pv._stream()))
    assert np.array_equal(host, out[0])


def test_gram_of_blocks_of_different_widths():
    c5, c24 = _blocks(5), _blocks(24)
    A, B = _dev(c5["A"]), _dev(c24["B"][:11])
    host = np.full((5, 11), np.nan)
    _lib.check(_lib.load().vfem_block_gram(N_BLOCK, 5, _p(A), 11, _p(B), None, _dp(host), pv._stream()))
    assert (np.abs(host - c5["A"] @ c24["B"][:11].T) < 1e-12 * (np.abs(c5["A"]) @ np.abs(c24["B"][:11]).T)).all()


@pytest.mark.parametrize("k", [1, 5, 24])
def test_combine_matches_numpy(k):
    c = _blocks(k)
    A = _dev(c["A"])
    C = np.ascontiguousarray(c["C"])
    out = []
    for _ in range(2):
        B = torch.full((k, N_BLOCK), float("nan"), dtype=torch.float64, device="cuda")
        _lib.check(_lib.load().vfem_block_combine(N_BLOCK, k, k, _p(A), _dp(C), _p(B), pv._stream()))
        torch.cuda.synchronize()
        out.append(B.cpu().numpy())
    err = (np.abs(out[0].astype(np.longdouble) - c["comb"]).astype(np.float64) / c["cabs"]).max()
    print("combine k = %d: %.2e of sum |C| |A|" % (k, err))
    assert err < 1e-14
    assert np.array_equal(out[0], out[1])


# ---- the eigensolver ----

def _simulator(name, loads=False):
    ne, h, D, rho, fixed = mc.case(name)
    N = len(ne)
    sim = pv.TensorProductSimulator([1] * N, [np.zeros(N), np.array(ne) * np.array(h)], list(ne))
    sim.ETensor = ElasticityTensor(*mc.CASES[name][2], dim=N)
    sim.E_0, sim.E_min, sim.gamma = mc.E0, mc.EMIN, mc.GAMMA
    sim.setElementDensities(rho)
    sim.dirichletMask = fixed
    if loads:
        sim.setLoads_device(torch.from_numpy(sc.cantilever(ne)[1]).cuda())
    return sim


def _mass_matrix(name):
    ne, h, D, rho, fixed = mc.case(name)
    return mc.assemble_mass(ne, h, mc.reference(name)["op"]["m"], fixed)


@pytest.mark.parametrize("name,preconditioner", [("16x12", "auto"), ("8x8x6", "auto"), ("8x8x6", "multigrid")])
def test_eigenmodes_match_the_dense_solver(name, preconditioner):
    ref = mc.reference(name)
    sim = _simulator(name)
    T = sim.multigridSolver(1) if preconditioner == "multigrid" else "auto"
    lam, Phi, info = modal.eigenmodes(sim, mc.NUM_MODES, tol=TOL_SOLVE, preconditioner=T)
    assert isinstance(lam, np.ndarray) and lam.shape == (mc.NUM_MODES,) and (np.diff(lam) > 0).all()
    assert Phi.shape == (mc.NUM_MODES, sim.numNodes(), sim.N) and Phi.is_cuda
    P = Phi.cpu().numpy().reshape(mc.NUM_MODES, -1).T
    M = _mass_matrix(name)
    err = np.abs(lam - ref["lam"]).max() / ref["lam"].max()
    overlap = np.abs(np.einsum("ni,ni->i", ref["Phi"], M @ P))
    orth = np.abs(P.T @ (M @ P) - np.eye(mc.NUM_MODES)).max()
    print("eigenmodes %s %s: %d iterations (P dropped %d times), eigenvalues %.2e, 1 - overlap %.2e, orthonormality %.2e, residuals %.2e"
          % (name, preconditioner, info["iterations"], info["droppedP"], err, np.abs(1.0 - overlap).max(), orth, info["residuals"].max()))
    assert err < TOL_LAMBDA[name]
    assert np.abs(1.0 - overlap).max() < TOL_OVERLAP[name] and orth < FLOOR
    assert info["residuals"].shape == (mc.NUM_MODES,) and info["residuals"].max() <= TOL_SOLVE
    assert info["iterations"] <= MAX_ITERATIONS
    fixed = mc.case(name)[4].reshape(-1)
    assert not P[fixed].any()
    # the residuals the solver reports are those of what it returns
    ne, h, D, rho, _ = mc.case(name)
    KP = np.stack([sim.applyK(Phi[i]).reshape(-1) for i in range(mc.NUM_MODES)], 1)
    MP = M @ P
    res = np.linalg.norm(np.where(fixed[:, None], 0.0, KP - MP * lam), axis=0) / (lam * np.linalg.norm(MP, axis=0))
    assert res.max() <= 2.0 * TOL_SOLVE
    # a warm start from the converged block
    lam2, Phi2, info2 = modal.eigenmodes(sim, mc.NUM_MODES, tol=TOL_SOLVE, preconditioner=T, X0=info["X"])
    print("  warm start: %d iterations" % info2["iterations"])
    assert info2["iterations"] <= 2 and np.abs(lam2 - lam).max() < FLOOR * lam.max()
    # and the same bits from the same start
    lam3, Phi3, _ = modal.eigenmodes(sim, mc.NUM_MODES, tol=TOL_SOLVE, preconditioner=T)
    assert np.array_equal(lam3, lam) and torch.equal(Phi3, Phi)


def test_eigenmodes_that_do_not_converge_raise_and_name_the_residual():
    sim = _simulator("16x12")
    with pytest.raises(RuntimeError, match=r"no convergence in 2 iterations: the worst residual is \d\.\d+e-\d+"):
        modal.eigenmodes(sim, 2, tol=1e-12, maxIter=2)


# ---- the objective ----

def _objective(name, tol=TOL_SOLVE):
    sim = _simulator(name)
    return sim, modal.MeanEigenvalueObjective(sim, numModes=mc.NUM_MODES, tol=tol)


@pytest.mark.parametrize("name", ["16x12", "8x8x6"])
def test_objective_matches_the_restatement(name):
    ref = mc.reference(name)
    sim, obj = _objective(name)
    J = obj.evaluate()
    g = obj.gradient()
    errs = abs(J - ref["J"]) / ref["J"], np.abs(g - ref["gradient"]).max() / np.abs(ref["gradient"]).max()
    print("objective %s: J %.2e gradient %.2e (bounds %.1e %.1e); %d positive and %d negative entries"
          % (name, errs[0], errs[1], TOL_J[name], TOL_GRADIENT[name], (g > 0).sum(), (g < 0).sum()))
    assert errs[0] < TOL_J[name] and errs[1] < TOL_GRADIENT[name]
    assert (g > 0).any() and (g < 0).any()
    assert np.array_equal(obj.eigenvalues(), obj.eigenvalues()) and J == float(np.sum(1.0 / obj.eigenvalues()))
    assert np.allclose(obj.frequencies(), np.sqrt(ref["lam"]) / (2.0 * np.pi), rtol=1e-11, atol=0.0)
    assert obj.modes_device().shape == (mc.NUM_MODES, sim.numNodes(), sim.N)
    assert torch.equal(obj.gradient_device(), obj.gradient_device())
    # an update at the same densities is a warm start
    obj.updateCache(torch.from_numpy(mc.case(name)[3]).cuda())
    assert obj.info()["iterations"] <= 2 and abs(obj.evaluate() - J) < FLOOR * J


def test_objective_with_a_mass_law_of_its_own():
    ne, h, D, rho, fixed = mc.case("16x12")
    mass = dict(massDensity=2.0, massExponent=1.0, lowDensityCut=0.5)
    op = mc.operators(ne, h, D, rho, fixed, mass)
    lam, Phi, _ = mc.dense_modes(op, 3)
    obj = modal.MeanEigenvalueObjective(_simulator("16x12"), numModes=3, tol=TOL_SOLVE, **mass)
    want = mc.gradient(op, lam, Phi)
    assert abs(obj.evaluate() - mc.objective(lam)) < TOL_J["16x12"] * mc.objective(lam)
    assert np.abs(obj.gradient() - want).max() < TOL_GRADIENT["16x12"] * np.abs(want).max()


@pytest.mark.parametrize("name", ["16x12", "8x8x6"])
def test_central_difference_of_the_objective(name):
    sim, obj = _objective(name, tol=1e-12)
    rho0 = torch.from_numpy(mc.case(name)[3]).cuda()
    d = torch.from_numpy(np.random.default_rng(17).standard_normal(rho0.numel())).cuda()
    an = float(obj.gradient_device() @ d)
    fd = (obj.evaluate(rho0 + FD_STEP * d) - obj.evaluate(rho0 - FD_STEP * d)) / (2.0 * FD_STEP)
    err = abs(fd - an) / abs(an)
    print("central difference %s: %.2e (directional derivative %.6e)" % (name, err, an))
    assert err < TOL_FD[name]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_backward_is_the_gradient_times_the_incoming_gradient(dtype):
    name = "16x12"
    ne = mc.CASES[name][0]
    sim, obj = _objective(name)
    rho = torch.from_numpy(mc.case(name)[3]).cuda().to(dtype).reshape(ne).requires_grad_(True)
    J = modal.meanEigenvalue(rho, obj)
    (2.5 * J).backward()
    assert rho.grad.dtype == dtype and rho.grad.shape == rho.shape and J.dtype == torch.float64
    assert float(J.detach()) == obj.evaluate()
    assert torch.equal(rho.grad.reshape(-1), (2.5 * obj.gradient_device()).to(dtype))
    J2 = modal.meanEigenvalue(rho.detach().clone().requires_grad_(True), obj)
    obj.updateCache(None)
    with pytest.raises(RuntimeError, match="updated between forward and backward"):
        J2.backward()


# ---- as a constraint of the MMA optimiser ----

def test_objective_constraint_and_three_mma_steps():
    name = "16x12"
    ne, h, D, rho, fixed = mc.case(name)
    sim = _simulator(name, loads=True)
    obj = modal.MeanEigenvalueObjective(sim, numModes=mc.NUM_MODES, tol=TOL_SOLVE)
    J0 = obj.evaluate()
    bound = 1.05 * J0
    cap = mma.ObjectiveConstraint(obj, bound)
    x0 = torch.from_numpy(rho).cuda()
    value = cap.evaluate_dev(x0)                                   # its first use updates the objective: a warm start
    assert value == 1.0 - obj.evaluate() / bound and abs(obj.evaluate() - J0) < FLOOR * J0
    assert torch.equal(cap.backprop_dev(x0), obj.gradient_device() * (-1.0 / bound))
    compliance = pv.ComplianceObjective(sim)
    problem = pv.TopologyOptimizationProblem(sim, compliance, [pv.TotalVolumeConstraint(0.6), cap], [])
    problem.setVars(x0)
    opt = mma.MMAOptimizer(problem, xmin=0.2, xmax=1.0, move=0.1)
    for _ in range(3):
        change = opt.step()
        assert 0.0 < change <= 0.1 * 0.8 + 1e-15
    x = problem.getVars_device()
    value = cap.evaluate_dev(x)                                    # solves at the final densities
    J = obj.evaluate()
    assert value == 1.0 - J / bound and torch.equal(sim.getDensities_device()[:x.numel()], x)
    op = mc.operators(ne, h, D, x.cpu().numpy(), fixed)
    want = mc.objective(mc.dense_modes(op, mc.NUM_MODES)[0])
    print("after three MMA steps: J %.6f (start %.6f, bound %.6f), restatement %.2e" % (J, J0, bound, abs(J - want) / want))
    assert abs(J - want) < TOL_J[name] * want


# ---- refusals ----

def test_refusals():
    with pytest.raises(RuntimeError, match="degree-1"):
        modal.eigenmodes(pv.TensorProductSimulator([2, 2], [np.zeros(2), np.ones(2)], [2, 2]), 1)
    padded = pv.TensorProductSimulator1_1_1([np.zeros(3), np.ones(3)], [2, 2, 2], _element_padding=(1, 0))
    with pytest.raises(RuntimeError, match="padding"):
        modal.eigenmodes(padded, 1)
    with pytest.raises(RuntimeError, match="padding"):
        modal.MeanEigenvalueObjective(padded)
    free = pv.TensorProductSimulator([1, 1], [np.zeros(2), np.ones(2)], [4, 4])
    with pytest.raises(RuntimeError, match="rigid modes"):
        modal.eigenmodes(free, 1)
    sim = _simulator("16x12")
    for k in (0, 9):
        with pytest.raises(RuntimeError, match="numModes must be 1 to 8"):
            modal.eigenmodes(sim, k)
        with pytest.raises(RuntimeError, match="numModes must be 1 to 8"):
            modal.MeanEigenvalueObjective(sim, numModes=k)
    with pytest.raises(RuntimeError, match="numGuard"):
        modal.eigenmodes(sim, 7, numGuard=2)
    with pytest.raises(RuntimeError, match="preconditioner"):
        modal.eigenmodes(sim, 2, preconditioner="jacobi")
    values = np.zeros((sim.numNodes(), 2))
    values[0, 0] = 0.5
    sim.dirichletValues = values
    with pytest.raises(RuntimeError, match="nonzero Dirichlet"):
        modal.eigenmodes(sim, 2)


def test_the_c_boundary_refuses_before_any_device_call():
    c = _mass_case((7, 5))
    lib = _lib.load()
    args, keep = _head(c["ne"], c["h"])
    nn = sc.num_nodes(c["ne"])
    X, m = _dev(c["X"]), _dev(c["m"])
    Y = _dev(np.full((3, nn * 2), np.nan))
    s = pv._stream()
    assert lib.vfem_modal_mass_apply(*args, None, None, 3, _p(X), _p(Y), s) == 1
    assert "null" in lib.vfem_last_error().decode()
    assert lib.vfem_modal_mass_apply(*args, _p(m), None, 3, None, _p(Y), s) == 1
    assert lib.vfem_modal_mass_apply(*args, _p(m), None, 3, _p(X), None, s) == 1
    for ncols in (0, 25):
        assert lib.vfem_modal_mass_apply(*args, _p(m), None, ncols, _p(X), _p(Y), s) == 1
        assert "ncols must be 1 to 24" in lib.vfem_last_error().decode()
        assert lib.vfem_modal_project(*args, None, ncols, _p(Y), s) == 1
    assert lib.vfem_modal_mass_apply(*args, _p(m), None, 3, _p(X), _p(X), s) == 1
    assert "aliases" in lib.vfem_last_error().decode()
    assert lib.vfem_modal_mass_apply(4, *args[1:], _p(m), None, 3, _p(X), _p(Y), s) == 1
    assert "dim" in lib.vfem_last_error().decode()
    bad, keep2 = _head((7, 0), c["h"])
    assert lib.vfem_modal_mass_apply(*bad, _p(m), None, 3, _p(X), _p(Y), s) == 1
    bad, keep3 = _head((7, 5), (0.5, 0.0))
    assert lib.vfem_modal_mass_apply(*bad, _p(m), None, 3, _p(X), _p(Y), s) == 1
    # the block operations
    A = _dev(np.ones((3, 100)))
    B = _dev(np.full((3, 100), np.nan))
    G = _dev(np.full((3, 3), np.nan))
    host, C = np.full((3, 3), -7.0), np.eye(3)
    assert lib.vfem_block_gram(100, 3, None, 3, _p(A), _p(G), _dp(host), s) == 1
    assert lib.vfem_block_gram(100, 3, _p(A), 3, _p(A), None, None, s) == 1
    assert lib.vfem_block_gram(0, 3, _p(A), 3, _p(A), _p(G), _dp(host), s) == 1
    for k in (0, 25):
        assert lib.vfem_block_gram(100, k, _p(A), 3, _p(A), _p(G), _dp(host), s) == 1
        assert lib.vfem_block_gram(100, 3, _p(A), k, _p(A), _p(G), _dp(host), s) == 1
        assert lib.vfem_block_combine(100, k, 3, _p(A), _dp(C), _p(B), s) == 1
        assert lib.vfem_block_combine(100, 3, k, _p(A), _dp(C), _p(B), s) == 1
    assert lib.vfem_block_combine(100, 3, 3, None, _dp(C), _p(B), s) == 1
    assert lib.vfem_block_combine(100, 3, 3, _p(A), None, _p(B), s) == 1
    assert lib.vfem_block_combine(100, 3, 3, _p(A), _dp(C), None, s) == 1
    assert lib.vfem_block_combine(100, 3, 3, _p(A), _dp(C), _p(A), s) == 1                 # the output is the input
    assert "aliases" in lib.vfem_last_error().decode()
    assert lib.vfem_block_combine(100, 2, 2, _p(A), _dp(np.eye(2)), _p(A[1:]), s) == 1     # the output starts inside the input
    assert lib.vfem_block_combine(100, 3, 3, _p(A), _dp(np.full((3, 3), np.nan)), _p(B), s) == 1
    # the gradient
    g = _dev(np.full(35, np.nan))
    K0, co = np.eye(8), np.ones(8)
    Phi, dE = _dev(c["X"][:2]), _dev(c["m"])
    for nmodes in (0, 9):
        assert lib.vfem_modal_gradient(*args, nmodes, _dp(K0), _dp(co), _dp(co), _p(dE), _p(dE), _p(Phi), _p(g), s) == 1
        assert "nmodes must be 1 to 8" in lib.vfem_last_error().decode()
    assert lib.vfem_modal_gradient(*args, 2, None, _dp(co), _dp(co), _p(dE), _p(dE), _p(Phi), _p(g), s) == 1
    assert lib.vfem_modal_gradient(*args, 2, _dp(K0), _dp(co), _dp(co), _p(dE), _p(dE), None, _p(g), s) == 1
    assert lib.vfem_modal_gradient(*args, 2, _dp(K0), _dp(co), _dp(co), _p(dE), _p(dE), _p(Phi), None, s) == 1
    torch.cuda.synchronize()
    for t in (Y, B, G, g):
        assert torch.isnan(t).all()
    assert (host == -7.0).all()
