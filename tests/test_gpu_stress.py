"""-m gpu: element stresses on the device (ndr_amd.stress, vfem_stress_*): the strain / stress / von Mises field, the p-norm measure,
its adjoint load and density gradient, the objective and the autograd node, against tests/stress_cpu.py.

Bounds.  Every figure named "restatement" was measured on the CPU with tests/stress_cpu.py.
  Pure kernels (fields, adjoint load, gradient kernel with a random lambda; no solve): 1e-12 of the largest entry, the bound a
    reordered fp64 sum is held to (k_hom_apply).  Requested alone, from views 8 bytes off a 16-byte line, and run twice: the same bits.
  Measure: 1e-13 relative for P in {1, 8, 64} on 300 001 values scaled to 1e6 and to 1e-6; the zero field gives exactly 0.
  Objective, random densities in [0.2, 1], isotropic E = 1, nu = 0.3, E_min = 1e-3, gamma = 3, q = 0.5, P = 8, cantilever:
      16 x 12 through ComplianceObjective (band factor): the restatement's two direct solves (COLAMD and natural ordering) differ by
        J 6.0e-15, vm 1.3e-14, lambda 1.5e-14, gradient 2.2e-14 of the largest entry: ten times these is below the floor 1e-12
      8 x 8 x 6 through MultigridComplianceObjective at tol = 1e-10: the restatement's CG at 1e-10 differs from its direct solve by
        J 1.95e-12, vm 2.99e-11, lambda 3.59e-11, gradient 1.11e-11; the bounds are ten times these
  Autograd: the same gradient bounds, plus half a float32 unit in the last place of each entry where the densities are float32.
  Central difference of compliance + 0.1 J along one random direction, step 1e-5, solves to 1e-12: the restatement's mismatch is
    1.49e-8 (16 x 12, direct) and 4.43e-10 (8 x 8 x 6, CG at 1e-12); bounds ten times these, not below 1e-7.

Measured on an MI355X:
  fields 0 .. 6.8e-16, adjoint load 3.2e-16 .. 2.9e-15, gradient kernel 2.0e-16 .. 1.8e-15 of the largest entry; alone / off-line
  views / second run bit-identical; measure: 0 (the same bits as the restatement) in all twelve cases.
  objective 16 x 12: J 1.04e-14, vm 1.14e-14, lambda 1.09e-14, gradient 1.41e-14; 8 x 8 x 6: J 3.48e-12, vm 1.11e-11, lambda 9.32e-12,
    gradient 1.35e-11; no factorisation added by the adjoint solve, a fresh objective on the same solve returns the same bits.
  backward: 1.41e-14 / 1.35e-11 (float64), 3.6e-8 / 3.8e-8 (float32: its rounding); central difference 1.55e-9 / 3.92e-10.
  The whole file runs in under 4 s.
  Against the parent commit every test fails at import: the module and the four entry points do not exist.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import homogenization_cpu as hc
import stress_cpu as sc

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor, _lib                     # noqa: E402
from ndr_amd import pyVoxelFEM as pv                           # noqa: E402
from ndr_amd import stress                                     # noqa: E402

TOL_KERNEL = 1e-12
TOL_MEASURE = 1e-13
FLOOR = 1e-12
P_NORM, Q = 8.0, 0.5
E0, EMIN, GAMMA = 1.0, 1e-3, 3.0
# J (relative), vm, lambda, gradient (of the largest entry): ten times the restatement's figures, not below the floor
TOL_OBJECTIVE = {"16x12": tuple(max(10 * v, FLOOR) for v in (6.0e-15, 1.3e-14, 1.5e-14, 2.2e-14)),
                 "8x8x6": tuple(max(10 * v, FLOOR) for v in (1.95e-12, 2.99e-11, 3.59e-11, 1.11e-11))}
FD_STEP = 1e-5
TOL_FD = {"16x12": max(10 * 1.49e-8, 1e-7), "8x8x6": max(10 * 4.43e-10, 1e-7)}

# 3 x 5 x 70 and 6 x 70 exceed one workgroup along every axis the kernels tile: a block is 64 lanes along the last axis by 4 rows of
# the axis before it, and in 3-D one block per layer of axis 0.  70 is one full 64-lane row and a partial second one, 5 and 6 are
# no multiples of 4; the node grids (4 x 6 x 71, 7 x 71) do the same for the node-wise adjoint load.  3 x 70 has its first axis
# inside one block.
SHAPES = [(1, 1), (2, 1), (5, 3), (3, 70), (6, 70), (1, 1, 1), (2, 1, 3), (3, 5, 70)]
EDGES = {2: (0.5, 0.3), 3: (0.5, 0.3, 0.7)}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


def _tensor(N):
    """a rotated orthotropic material: every entry of D is non-zero"""
    t = ElasticityTensor(dim=N)
    if N == 2:
        t.setOrthotropic(2.0, 1.0, 0.25, 0.45)
        c, s = np.cos(0.6), np.sin(0.6)
        return t.transform(np.array([[c, -s], [s, c]]))
    t.setOrthotropic(2.0, 1.0, 1.5, 0.2, 0.25, 0.3, 0.5, 0.6, 0.4)
    return t.transform(hc.rotation((1.0, 2.0, 3.0), 0.7))


class _Head:
    """the leading arguments of the vfem_stress_* grid calls (the arrays stay alive with the object)"""

    def __init__(self, ne, h, D):
        self.n = np.asarray(ne, dtype=np.int64)
        self.h = np.ascontiguousarray(h, dtype=np.float64)
        self.D = np.ascontiguousarray(D, dtype=np.float64)
        self.N = len(ne)

    def args(self):
        return (self.N, self.n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(self.h), _dp(self.D))


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


def _out(shape, off=False):
    return _dev(np.full(shape, np.nan), off)


@functools.lru_cache(maxsize=None)
def _kernel_case(ne):
    """random displacement, densities, Dirichlet mask and lambda on one grid with the restatement's results; shared, left unchanged"""
    N = len(ne)
    h, D = EDGES[N], _tensor(N).D
    rng = np.random.default_rng(100 + int(np.prod(ne)))
    nn, nel = sc.num_nodes(ne), int(np.prod(ne))
    u = rng.standard_normal(nn * N)
    rho = rng.uniform(0.05, 1.0, size=nel)
    fixed = rng.uniform(size=(nn, N)) < 0.2
    lam = rng.standard_normal(nn * N)
    m, dm = sc.multiplier(rho, E0, EMIN, Q)
    dE = hc.moduli(rho, E0, EMIN, GAMMA)[1]
    eps, sig, vm = sc.fields(ne, h, D, m, u)
    J = sc.pnorm(vm, P_NORM)
    a = sc.adjoint_load(ne, h, D, m, u, P_NORM, fixed)
    K0 = hc.element_constants(D, h)[0]
    dofs = sc.element_dofs(ne)
    vm0 = sc.von_mises((eps * sc.mult(N)) @ D.T)
    grad = sc.weights(vm, J, P_NORM) * dm * vm0 - dE * np.einsum("ek,kl,el->e", lam[dofs], K0, u[dofs])
    bits = np.zeros(nn, dtype=np.uint8)
    for c in range(N):
        bits |= fixed[:, c].astype(np.uint8) << c
    return dict(ne=ne, N=N, h=h, D=D, u=u, m=m, dm=dm, dE=dE, lam=lam, fixed=fixed, bits=bits, K0=K0, strain=eps, stress=sig, vm=vm,
                J=J, a=a, grad=grad)


def _run_fields(c, strain, stress_, vm, off=False, u=None):
    head = _Head(c["ne"], c["h"], c["D"])
    S = 3 if c["N"] == 2 else 6
    nel = int(np.prod(c["ne"]))
    ud, md = _dev(c["u"] if u is None else u, off), _dev(c["m"])
    outs = (_out((nel, S), off) if strain else None, _out((nel, S), off) if stress_ else None, _out((nel,), off) if vm else None)
    _lib.check(_lib.load().vfem_stress_fields(*head.args(), _p(md), _p(ud), _p(outs[0]), _p(outs[1]), _p(outs[2]), pv._stream()))
    torch.cuda.synchronize()
    return outs


def _run_adjoint(c, off=False, u=None, m=None, J=None, masked=True):
    head = _Head(c["ne"], c["h"], c["D"])
    a = _out((sc.num_nodes(c["ne"]), c["N"]), off)
    mask = torch.from_numpy(c["bits"]).cuda() if masked else None
    md, ud = _dev(c["m"] if m is None else m), _dev(c["u"] if u is None else u, off)         # (named: alive until the kernel has run)
    work = _out((int(np.prod(c["ne"])), 3 if c["N"] == 2 else 6), off)
    _lib.check(_lib.load().vfem_stress_adjoint_load(*head.args(), _p(md), _p(ud), float(c["J"] if J is None else J), P_NORM, _p(mask),
                                                    _p(work), _p(a), pv._stream()))
    torch.cuda.synchronize()
    return a


def _run_gradient(c, off=False):
    head = _Head(c["ne"], c["h"], c["D"])
    g = _out((int(np.prod(c["ne"])),), off)
    K0 = np.ascontiguousarray(c["K0"])
    md, dmd, dEd, ud, ld = _dev(c["m"]), _dev(c["dm"]), _dev(c["dE"]), _dev(c["u"], off), _dev(c["lam"], off)
    _lib.check(_lib.load().vfem_stress_pnorm_gradient(*head.args(), _dp(K0), _p(md), _p(dmd), _p(dEd), _p(ud), _p(ld), float(c["J"]),
                                                      P_NORM, _p(g), pv._stream()))
    torch.cuda.synchronize()
    return g


def _name(ne):
    return "x".join(map(str, ne))


# ---- the pure kernels ----

@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_fields_match_the_restatement(ne):
    c = _kernel_case(ne)
    strain, stress_, vm = _run_fields(c, True, True, True)
    for got, name in ((strain, "strain"), (stress_, "stress"), (vm, "vm")):
        err = _relmax(got.cpu().numpy(), c[name])
        print("%s %s: %.2e" % (name, _name(ne), err))
        assert err < TOL_KERNEL
    # every output requested alone, a second run, and views 8 bytes off a 16-byte line: the same bits
    assert torch.equal(_run_fields(c, True, False, False)[0], strain)
    assert torch.equal(_run_fields(c, False, True, False)[1], stress_)
    assert torch.equal(_run_fields(c, False, False, True)[2], vm)
    again, off = _run_fields(c, True, True, True), _run_fields(c, True, True, True, off=True)
    for k in range(3):
        assert torch.equal(again[k], (strain, stress_, vm)[k]) and torch.equal(off[k], (strain, stress_, vm)[k])


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_adjoint_load_is_the_derivative_of_the_measure(ne):
    c = _kernel_case(ne)
    a = _run_adjoint(c)
    got = a.cpu().numpy().reshape(-1)
    err = _relmax(got, c["a"])
    print("adjoint load %s: %.2e" % (_name(ne), err))
    assert err < TOL_KERNEL
    fixed = c["fixed"].reshape(-1)
    assert np.array_equal(got[fixed], np.zeros(int(fixed.sum())))
    assert torch.equal(_run_adjoint(c), a) and torch.equal(_run_adjoint(c, off=True), a)
    free = _run_adjoint(c, masked=False).cpu().numpy().reshape(-1)                # no mask: nothing is zeroed
    assert _relmax(free, sc.adjoint_load(ne, c["h"], c["D"], c["m"], c["u"], P_NORM)) < TOL_KERNEL


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_gradient_kernel_matches_the_restatement(ne):
    c = _kernel_case(ne)
    g = _run_gradient(c)
    err = _relmax(g.cpu().numpy(), c["grad"])
    print("gradient kernel %s: %.2e" % (_name(ne), err))
    assert err < TOL_KERNEL
    assert torch.equal(_run_gradient(c), g) and torch.equal(_run_gradient(c, off=True), g)


@pytest.mark.parametrize("ne", [(5, 5), (4, 4, 4)], ids=_name)
def test_an_unstrained_element_has_zero_stress_and_finite_derivatives(ne):
    c = dict(_kernel_case(ne))
    N = len(ne)
    e = int(np.ravel_multi_index(tuple(n // 2 for n in ne), ne))
    u = c["u"].copy().reshape(-1, N)
    u[sc.element_dofs(ne)[e][::N] // N] = 0.0
    u = u.reshape(-1)
    strain, stress_, vm = (t.cpu().numpy() for t in _run_fields(c, True, True, True, u=u))
    assert vm[e] == 0.0 and not strain[e].any() and not stress_[e].any()
    assert np.isfinite(strain).all() and np.isfinite(stress_).all() and np.isfinite(vm).all()
    J = sc.pnorm(vm, P_NORM)
    a = _run_adjoint(c, u=u, J=J).cpu().numpy().reshape(-1)
    assert np.isfinite(a).all()
    assert _relmax(a, sc.adjoint_load(ne, c["h"], c["D"], c["m"], u, P_NORM, c["fixed"])) < TOL_KERNEL
    # no stress anywhere: the measure is 0 and the load is exactly 0
    zero = _run_adjoint(c, u=np.zeros_like(u), J=0.0)
    assert torch.equal(zero, torch.zeros_like(zero))


# ---- the measure ----

def _measure(vm, P):
    J, vmax = ctypes.c_double(-1.0), ctypes.c_double(-1.0)
    _lib.check(_lib.load().vfem_stress_pnorm(vm.numel(), _p(vm), float(P), ctypes.byref(J), ctypes.byref(vmax), pv._stream()))
    return J.value, vmax.value


@functools.lru_cache(maxsize=None)
def _measure_values():
    return np.random.default_rng(55).uniform(0.0, 1.0, size=300001)         # more values than the 1024 x 256 threads of a stage


@pytest.mark.parametrize("scale", [1e6, 1e-6])
@pytest.mark.parametrize("P", [1.0, 8.0, 64.0])
def test_measure_matches_the_restatement(P, scale):
    vm = _measure_values() * scale
    for off in (False, True):
        d = _dev(vm, off)
        J, vmax = _measure(d, P)
        err = abs(J - sc.pnorm(vm, P)) / sc.pnorm(vm, P)
        print("measure P = %g, scale %g: %.2e" % (P, scale, err))
        assert err < TOL_MEASURE and vmax == vm.max()
        assert _measure(d, P) == (J, vmax)                                   # run to run


def test_measure_of_the_zero_field_is_exactly_zero():
    assert _measure(torch.zeros(1000, dtype=torch.float64, device="cuda"), 8.0) == (0.0, 0.0)


# ---- the public field functions ----

@pytest.mark.parametrize("ne", [(5, 3), (3, 2, 4)], ids=_name)
def test_public_fields_of_an_anisotropic_simulator(ne):
    c = _kernel_case(ne)
    N = len(ne)
    sim = pv.TensorProductSimulator([1] * N, [np.zeros(N), np.array(ne) * np.array(c["h"])], list(ne))
    sim.ETensor = _tensor(N)
    sim.E_0, sim.E_min, sim.gamma = E0, EMIN, GAMMA
    rho = ((c["m"] - EMIN) / (E0 - EMIN)) ** (1.0 / Q)
    sim.setElementDensities(rho)
    u = c["u"].reshape(-1, N)
    assert _relmax(stress.elementStrains(sim, u), c["strain"]) < TOL_KERNEL
    assert _relmax(stress.elementStresses(sim, u, stressExponent=Q), c["stress"]) < 10 * TOL_KERNEL      # rho went through a root
    assert _relmax(stress.vonMises(sim, u, stressExponent=Q), c["vm"]) < 10 * TOL_KERNEL
    physical = sc.fields(ne, c["h"], c["D"], sc.multiplier(rho, E0, EMIN, GAMMA)[0], c["u"])[2]          # None: q = gamma
    assert _relmax(stress.vonMises_device(sim, torch.from_numpy(u).cuda()).cpu().numpy(), physical) < TOL_KERNEL


# ---- the objective ----

def _simulator(name):
    ne, h, D, rho, f, fixed = sc.case(name)
    N = len(ne)
    sim = pv.TensorProductSimulator([1] * N, [np.zeros(N), np.array(ne) * np.array(h)], list(ne))
    sim.ETensor = ElasticityTensor(*sc.CASES[name][2], dim=N)
    sim.E_0, sim.E_min, sim.gamma = E0, EMIN, GAMMA
    sim.setElementDensities(rho)
    sim.dirichletMask = fixed
    sim.setLoads_device(torch.from_numpy(f).cuda())
    return sim


def _objective(name, tol=1e-10):
    sim = _simulator(name)
    if name == "16x12":
        solved = pv.ComplianceObjective(sim)
    else:
        solved = pv.MultigridComplianceObjective(sim.multigridSolver(1))
        solved.tol, solved.cgIter, solved.zeroInit = tol, 500, True
        solved.updateCache(None)
    return sim, stress.PNormStressObjective(solved, P=P_NORM, stressExponent=Q)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype="float64"):
    """the restatement's direct solution of a case, computed once and shared (tests leave it unchanged)"""
    ne, h, D, rho, f, fixed = sc.case(name)
    rho = rho.astype(dtype).astype(np.float64)
    return sc.evaluate(ne, h, D, rho, f, fixed, E0, EMIN, GAMMA, Q, P_NORM)


@pytest.mark.parametrize("name", ["16x12", "8x8x6"])
def test_objective_matches_the_restatement(name):
    ref = _reference(name)
    sim, obj = _objective(name)
    tJ, tvm, tlam, tg = TOL_OBJECTIVE[name]
    before = sim.numDirectFactorizations()
    J = obj.evaluate()
    errs = (abs(J - ref["J"]) / ref["J"], _relmax(obj.vonMises_device().cpu().numpy(), ref["vm"]),
            _relmax(obj.adjoint_device().cpu().numpy().reshape(-1), ref["lam"]), _relmax(obj.gradient(), ref["gradient"]))
    print("objective %s: J %.2e vm %.2e lambda %.2e gradient %.2e (bounds %.1e %.1e %.1e %.1e)" % ((name,) + errs + TOL_OBJECTIVE[name]))
    assert errs[0] < tJ and errs[1] < tvm and errs[2] < tlam and errs[3] < tg
    assert obj.maxVonMises() == float(obj.vonMises_device().max()) and obj.maxVonMises() <= J
    assert sim.numDirectFactorizations() == before                               # the adjoint solve reuses what the primal solve built
    assert (before > 0) == (name == "16x12")
    g = obj.gradient_device()
    assert torch.equal(obj.gradient_device(), g)
    fresh = stress.PNormStressObjective(obj.solved, P=P_NORM, stressExponent=Q)   # nothing cached: the kernels and the solve run again
    assert torch.equal(fresh.gradient_device(), g) and fresh.evaluate() == J
    assert sim.numDirectFactorizations() == before


def test_an_unloaded_design_has_zero_measure_and_zero_gradient():
    sim = _simulator("16x12")
    sim.setLoads_device(torch.zeros((sim.numNodes(), 2), dtype=torch.float64, device="cuda"))
    obj = stress.PNormStressObjective(pv.ComplianceObjective(sim), P=P_NORM, stressExponent=Q)
    assert obj.evaluate() == 0.0 and obj.maxVonMises() == 0.0
    g, lam = obj.gradient_device(), obj.adjoint_device()
    assert torch.equal(g, torch.zeros_like(g)) and torch.equal(lam, torch.zeros_like(lam))


# ---- autograd ----

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("name", ["16x12", "8x8x6"])
def test_backward_is_the_gradient_times_the_incoming_gradient(name, dtype):
    ne = sc.CASES[name][0]
    ref = _reference(name, "float64" if dtype == torch.float64 else "float32")
    sim, obj = _objective(name)
    rho = torch.from_numpy(sc.case(name)[3]).cuda().to(dtype).reshape(ne).requires_grad_(True)
    J = stress.pNormStress(rho, obj)
    (2.5 * J).backward()
    assert rho.grad.dtype == dtype and rho.grad.shape == rho.shape and J.dtype == torch.float64
    assert abs(float(J.detach()) - ref["J"]) / ref["J"] < TOL_OBJECTIVE[name][0]
    expect = 2.5 * ref["gradient"]
    slack = TOL_OBJECTIVE[name][3] * np.abs(expect).max()
    if dtype == torch.float32:
        slack = slack + 0.5 * np.spacing(np.abs(expect).astype(np.float32)).astype(np.float64)
    err = np.abs(rho.grad.cpu().numpy().astype(np.float64).reshape(-1) - expect)
    print("backward %s %s: %.2e of the largest entry" % (name, dtype, err.max() / np.abs(expect).max()))
    assert (err <= slack).all()
    # both outputs of the joint node
    rho2 = rho.detach().clone().requires_grad_(True)
    both = stress.complianceAndPNormStress(rho2, obj)
    (both[0] + 0.1 * both[1]).backward()
    expect = ref["compliance_gradient"] + 0.1 * ref["gradient"]
    assert abs(float(both[0].detach()) - ref["compliance"]) / ref["compliance"] < TOL_OBJECTIVE[name][0]
    slack = 2.0 * TOL_OBJECTIVE[name][3] * np.abs(expect).max()
    if dtype == torch.float32:
        slack = slack + 0.5 * np.spacing(np.abs(expect).astype(np.float32)).astype(np.float64)
    assert (np.abs(rho2.grad.cpu().numpy().astype(np.float64).reshape(-1) - expect) <= slack).all()


@pytest.mark.parametrize("name", ["16x12", "8x8x6"])
def test_central_difference_of_compliance_plus_stress(name):
    sim, obj = _objective(name, tol=1e-12)
    rho0 = torch.from_numpy(sc.case(name)[3]).cuda()
    d = torch.from_numpy(np.random.default_rng(17).standard_normal(rho0.numel())).cuda()

    def loss(r):
        out = stress.complianceAndPNormStress(r, obj)
        return out[0] + 0.1 * out[1]

    rho = rho0.clone().requires_grad_(True)
    loss(rho).backward()
    an = float(rho.grad @ d)
    with torch.no_grad():
        fd = float(loss(rho0 + FD_STEP * d) - loss(rho0 - FD_STEP * d)) / (2.0 * FD_STEP)
    err = abs(fd - an) / abs(an)
    print("central difference %s: %.2e (directional derivative %.6e)" % (name, err, an))
    assert err < TOL_FD[name]


# ---- refusals ----

def test_refusals_leave_the_result_buffers_alone():
    with pytest.raises(RuntimeError, match="degree-1"):
        stress.vonMises_device(pv.TensorProductSimulator([2, 2], [np.zeros(2), np.ones(2)], [2, 2]), torch.zeros(25, 2))
    padded = pv.TensorProductSimulator1_1_1([np.zeros(3), np.ones(3)], [2, 2, 2], _element_padding=(1, 0))
    with pytest.raises(RuntimeError, match="padding"):
        stress.elementStrains_device(padded, torch.zeros(27, 3))
    sim = _simulator("16x12")
    with pytest.raises(RuntimeError, match="Invalid input size"):
        stress.elementStresses_device(sim, torch.zeros(10, 2))
    with pytest.raises(RuntimeError, match="at least 1"):
        stress.PNormStressObjective(pv.ComplianceObjective(sim), P=0.5)
    # the C boundary: P < 1, a non-finite P, dim, extents, h and null pointers are refused before any device call
    c = _kernel_case((5, 3))
    lib, head = _lib.load(), _Head(c["ne"], c["h"], c["D"])
    u, m = _dev(c["u"]), _dev(c["m"])
    a, vm, work = _out((24, 2)), _out((15,)), _out((15, 3))
    J = ctypes.c_double(-7.0)
    for P in (0.5, float("nan"), float("inf")):
        assert lib.vfem_stress_pnorm(15, _p(m), P, ctypes.byref(J), None, pv._stream()) == 1
        assert "at least 1" in lib.vfem_last_error().decode()
        assert lib.vfem_stress_adjoint_load(*head.args(), _p(m), _p(u), 1.0, P, None, _p(work), _p(a), pv._stream()) == 1
    assert lib.vfem_stress_adjoint_load(*head.args(), _p(m), _p(u), -1.0, 8.0, None, _p(work), _p(a), pv._stream()) == 1
    assert lib.vfem_stress_adjoint_load(*head.args(), None, _p(u), 1.0, 8.0, None, _p(work), _p(a), pv._stream()) == 1
    assert lib.vfem_stress_adjoint_load(*head.args(), _p(m), _p(u), 1.0, 8.0, None, None, _p(a), pv._stream()) == 1
    assert lib.vfem_stress_fields(4, *head.args()[1:], _p(m), _p(u), None, None, _p(vm), pv._stream()) == 1
    assert "dim" in lib.vfem_last_error().decode()
    assert lib.vfem_stress_fields(*head.args(), _p(m), None, None, None, _p(vm), pv._stream()) == 1
    assert lib.vfem_stress_fields(*head.args(), _p(m), _p(u), None, None, None, pv._stream()) == 1
    assert lib.vfem_stress_fields(*head.args(), None, _p(u), None, None, _p(vm), pv._stream()) == 1
    assert lib.vfem_stress_fields(*_Head((5, 0), c["h"], c["D"]).args(), _p(m), _p(u), None, None, _p(vm), pv._stream()) == 1
    assert lib.vfem_stress_fields(*_Head((5, 3), (0.5, 0.0), c["D"]).args(), _p(m), _p(u), None, None, _p(vm), pv._stream()) == 1
    torch.cuda.synchronize()
    assert J.value == -7.0 and torch.isnan(a).all() and torch.isnan(vm).all() and torch.isnan(work).all()
