"""-m gpu: load cases on the device (ndr_amd.loadcases, vfem_loads_*): the two kernels, the public assembly, the objective over a direct
and a multigrid solver, its case views beside the stress and buckling measures, the design loops and the autograd node, against
tests/loadcases_cpu.py.

Bounds.  Every figure named "restatement" was measured on the CPU with tests/loadcases_cpu.py (tests/test_loadcases_cpu.py prints them).
  Kernels (assemble, gradient): the reference is the restatement evaluated in np.longdouble; the rounding floor of the formula is what
    the same restatement in float64 differs from it, relative to the largest entry, and the bound is 16 times that floor (another
    summation order), computed per case and printed with it.  ``assembleLoad`` against the torch ``_stress_load``: the same bound.
  Direct chain (J, every c_i, the gradient): 1e-11 of the largest entry, the bound tests/test_gpu_buckling.py uses for its direct chain.
  Multigrid chain (block3even, 2 levels, PCG to a relative residual of 1e-12): the restatement's chain with conjugate-gradient solves to
    1e-12 (stress_cpu.solve_cg) differs from its dense chain by 8.9e-14 in the values (J and the c_i, relative; the largest over both
    aggregates) and by 5.7e-14 of the largest entry in the gradient (loadcases_cpu.CG_*_MEASURED, computed and pinned by
    tests/test_loadcases_cpu.py); the bounds are ten times these: 8.9e-13 and 5.7e-13.
  Free thermal expansion: ten times the restatement's figures (tests/test_loadcases_cpu.py: u 1.8e-13 / 1.2e-13 on 16 x 6, 7.9e-13 /
    3.9e-13 on 6 x 4 x 3, isotropic / orthotropic); c 2.2e-14 on 16 x 6 isotropic, and ndof x 2^-52 (5.3e-14 / 9.3e-14) for the three
    cases whose restatement figure is no more than one rounding of c (loadcases_cpu.free_c_bound has the reason).

Measured on an MI355X (DESIGN 3.15 has the same figures):
  assemble, 72 cases: 1.1e-16 .. 3.2e-16 of the largest entry against floors of 1.2e-16 .. 3.7e-16 (at most 1.9 floors); gradient, 36
    cases: 1.0e-16 .. 4.0e-16 against floors of 2.3e-16 .. 1.7e-15 (at most 1.2 floors); in place, off-line buffers and a second run
    bit-identical.  assembleLoad against _stress_load 1.0e-16 (7 x 5) / 3.9e-16 (12 x 10 x 9), bounds 1.8e-15 / 2.6e-15.
  one fixed case: evaluate() bit-identical to ComplianceObjective's, gradient against complianceGradient_device 6.8e-16 (bound 2.6e-13).
  direct chain: arch2 J 2.6e-15 / 3.4e-15, c 4.1e-15, gradient 1.2e-14 (sum / pnorm); block3 J 8.0e-14 / 9.5e-14, c 9.7e-14, gradient
    2.1e-13 / 2.0e-13; arch2 has 52 / 56 positive and 44 / 40 negative entries, block3 37 / 46 and 59 / 50.
  multigrid chain: J 9.4e-14 / 5.3e-14, c 2.3e-13, gradient 1.2e-13 / 9.6e-14; 15 / 15 / 12 iterations, 0 / 0 / 0 on the second update.
  free expansion: u 1.6e-13 / 4.8e-13 (16 x 6, isotropic / orthotropic), 1.1e-12 / 1.5e-12 (6 x 4 x 3); c 8.2e-15 at worst.
  three OC steps (two traffic loads): J 43.41 -> 22.70 -> 16.03 -> 13.63, the restatement at the final densities within 2.8e-14; three MMA
    steps on the arch under its own weight and two traffic loads: J 31.89 -> 18.67 -> 11.91 -> 8.14, within 4.4e-15; the sum beside one
    constraint per case view: c 21.70 -> 9.58 under the bounds 20.62, multipliers 43.4 (volume), 0, 0, one factorisation per step.
  The whole file runs in 4 s.
  Against the parent commit every test fails at import: the module and the entry points do not exist.
"""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

import loadcases_cpu as lc
import stress_cpu as sc

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor, _lib, buckling, loadcases, mma, stress         # noqa: E402
from ndr_amd import pyVoxelFEM as pv                                                 # noqa: E402
from ndr_amd.loadcases import LoadCase, LoadCaseComplianceObjective                  # noqa: E402

MARGIN = 16.0
TOL_DIRECT = 1e-11
TOL_MG_VALUE, TOL_MG_GRADIENT = 10 * lc.CG_VALUE_MEASURED, 10 * lc.CG_GRADIENT_MEASURED

# 40 x 37 and 12 x 10 x 9 span several workgroups of the cell kernels (64 lanes along the last axis by 4 rows, one block per layer of
# axis 0 in 3-D); 5 x 70 and 3 x 3 x 70 have 71 nodes along the last axis and so cross the block edge at 64
SHAPES = [(7, 5), (40, 37), (5, 70), (6, 4, 5), (12, 10, 9), (3, 3, 70)]
EDGES = {2: (0.5, 0.3), 3: (0.5, 0.3, 0.7)}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


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
    return (len(ne), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(hh)), (n, hh)      # (the arrays stay alive)


def _rel(got, ref):
    """the largest difference relative to the largest entry of the (longdouble) reference"""
    return float(np.abs(np.asarray(got, dtype=np.longdouble) - ref).max() / np.abs(ref).max())


# ---- the two kernels against the restatement in extended precision ----

@functools.lru_cache(maxsize=None)
def _kernel_case(ne):
    N = len(ne)
    rng = np.random.default_rng(500 + int(np.prod(ne)))
    nn, nel, ke = sc.num_nodes(ne), int(np.prod(ne)), N * 2 ** N
    c = dict(ne=ne, N=N, h=EDGES[N], K0=lc.hc.element_constants(lc.hc.isotropic_D(1.3, 0.3, N), EDGES[N])[0],
             Lb=rng.standard_normal((8, ke)), Lt=rng.standard_normal((8, ke)), m=rng.uniform(0.05, 1.0, size=nel),
             E=rng.uniform(0.05, 1.0, size=nel), dE=rng.uniform(0.05, 1.0, size=nel), dm=rng.uniform(0.05, 1.0, size=nel),
             f=rng.standard_normal(nn * N), U=rng.standard_normal((8, nn * N)), cK=rng.standard_normal(8), cB=rng.standard_normal(8),
             cT=rng.standard_normal(8), fixed=rng.uniform(size=(nn, N)) < 0.2)
    bits = np.zeros(nn, dtype=np.uint8)
    for a in range(N):
        bits |= c["fixed"][:, a].astype(np.uint8) << a
    c["bits"] = bits
    return c


def _assemble_args(c, which, with_f, masked):
    return (c["ne"], c["Lb"][0] if which in ("body", "both") else None, c["Lt"][0] if which in ("eigen", "both") else None, c["m"], c["E"],
            c["fixed"] if masked else None, c["f"] if with_f else None)


def _run_assemble(c, which, with_f, masked, off=False, in_place=False):
    args, keep = _head(c["ne"], c["h"])
    Lb, Lt = (np.ascontiguousarray(c[k][0]) if use else None for k, use in (("Lb", which in ("body", "both")), ("Lt", which in ("eigen", "both"))))
    m, E = (_dev(c[k], off) if L is not None else None for k, L in (("m", Lb), ("E", Lt)))
    f_in = _dev(c["f"], off) if with_f else None
    out = f_in if in_place else _dev(np.full(c["f"].shape, np.nan), off)
    mask = torch.from_numpy(c["bits"]).cuda() if masked else None
    _lib.check(_lib.load().vfem_loads_assemble(*args, _dp(Lb), _dp(Lt), _p(m), _p(E), _p(mask), _p(f_in), _p(out), pv._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("with_f", [False, True], ids=["alone", "added"])
@pytest.mark.parametrize("which", ["body", "eigen", "both"])
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_assemble_kernel_matches_the_restatement(ne, which, with_f, masked):
    c = _kernel_case(ne)
    args = _assemble_args(c, which, with_f, masked)
    ref = lc.kernel_assemble(*args, dtype=np.longdouble)
    floor = _rel(lc.kernel_assemble(*args), ref)
    out = _run_assemble(c, which, with_f, masked)
    err = _rel(out.cpu().numpy(), ref)
    print("assemble %s %s %s %s: %.2e (floor %.2e, bound %.2e)" % (_name(ne), which, "added" if with_f else "alone",
                                                                   "masked" if masked else "free", err, floor, MARGIN * floor))
    assert err < MARGIN * floor
    if masked:
        assert not out.cpu().numpy()[c["fixed"].reshape(-1)].any()
    assert torch.equal(_run_assemble(c, which, with_f, masked), out)                                   # run to run


@pytest.mark.parametrize("ne", [(40, 37), (12, 10, 9)], ids=_name)
def test_assemble_in_place_and_on_buffers_8_bytes_off_a_16_byte_line(ne):
    c = _kernel_case(ne)
    out = _run_assemble(c, "both", True, True)
    assert torch.equal(_run_assemble(c, "both", True, True, in_place=True), out)
    assert torch.equal(_run_assemble(c, "both", True, True, off=True), out)
    assert torch.equal(_run_assemble(c, "both", True, True, off=True, in_place=True), out)


def _gradient_args(c, k, patterns):
    return (c["ne"], c["K0"], c["Lb"][:k] if patterns else None, c["Lt"][:k] if patterns else None, c["dE"], c["dm"], c["U"][:k],
            c["cK"][:k], c["cB"][:k], c["cT"][:k])


def _run_gradient(c, k, patterns, off=False):
    args, keep = _head(c["ne"], c["h"])
    dE, U = _dev(c["dE"], off), _dev(c["U"][:k], off)
    dm = _dev(c["dm"], off) if patterns else None
    g = _dev(np.full(c["m"].shape, np.nan), off)
    K0, cK = np.ascontiguousarray(c["K0"]), np.ascontiguousarray(c["cK"][:k])
    cB, cT, Lb, Lt = (np.ascontiguousarray(c[n][:k]) if patterns else None for n in ("cB", "cT", "Lb", "Lt"))
    _lib.check(_lib.load().vfem_loads_gradient(*args, k, _dp(K0), _dp(cK), _dp(cB), _dp(cT), _dp(Lb), _dp(Lt), _p(dE), _p(dm), _p(U), _p(g),
                                               pv._stream()))
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("patterns", [False, True], ids=["stiffness", "patterns"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_gradient_kernel_matches_the_restatement(ne, k, patterns):
    c = _kernel_case(ne)
    args = _gradient_args(c, k, patterns)
    ref = lc.kernel_gradient(*args, dtype=np.longdouble)
    floor = _rel(lc.kernel_gradient(*args), ref)
    g = _run_gradient(c, k, patterns)
    err = _rel(g.cpu().numpy(), ref)
    print("gradient %s, %d cases, %s: %.2e (floor %.2e, bound %.2e)" % (_name(ne), k, "patterns" if patterns else "stiffness", err, floor,
                                                                        MARGIN * floor))
    assert err < MARGIN * floor
    assert torch.equal(_run_gradient(c, k, patterns), g)                                               # run to run


@pytest.mark.parametrize("ne", [(40, 37), (12, 10, 9)], ids=_name)
def test_gradient_on_buffers_8_bytes_off_a_16_byte_line(ne):
    c = _kernel_case(ne)
    assert torch.equal(_run_gradient(c, 3, True, off=True), _run_gradient(c, 3, True))


def test_gradient_with_one_kind_of_pattern():
    """the body-force patterns (with dm) and the eigenstrain patterns may each be absent on their own"""
    c = _kernel_case((6, 4, 5))
    args, keep = _head(c["ne"], c["h"])
    dE, dm, U = _dev(c["dE"]), _dev(c["dm"]), _dev(c["U"][:3])
    K0, co, Lb, Lt = np.ascontiguousarray(c["K0"]), np.ascontiguousarray(c["cK"][:3]), np.ascontiguousarray(c["Lb"][:3]), np.ascontiguousarray(c["Lt"][:3])
    zero = np.zeros_like(Lb)
    for body in (True, False):
        g = _dev(np.full(c["m"].shape, np.nan))
        _lib.check(_lib.load().vfem_loads_gradient(*args, 3, _dp(K0), _dp(co), _dp(co) if body else None, None if body else _dp(co),
                                                   _dp(Lb) if body else None, None if body else _dp(Lt), _p(dE), _p(dm) if body else None,
                                                   _p(U), _p(g), pv._stream()))
        ref = lc.kernel_gradient(c["ne"], c["K0"], Lb if body else zero, zero if body else Lt, c["dE"], c["dm"], c["U"][:3], co, co, co,
                                 dtype=np.longdouble)
        floor = _rel(lc.kernel_gradient(c["ne"], c["K0"], Lb if body else zero, zero if body else Lt, c["dE"], c["dm"], c["U"][:3], co, co, co), ref)
        assert _rel(g.cpu().numpy(), ref) < MARGIN * floor


# ---- simulators of the restatement's problems ----

def _simulator(p, tensor=None):
    ne, h = p["ne"], p["h"]
    N = len(ne)
    sim = pv.TensorProductSimulator([1] * N, [np.zeros(N), np.array(ne) * np.array(h)], list(ne))
    sim.ETensor = ElasticityTensor(1.0, 0.3, dim=N) if tensor is None else tensor
    sim.E_0, sim.E_min, sim.gamma = lc.E0, lc.EMIN, lc.GAMMA
    sim.setElementDensities(p["rho"])
    sim.dirichletMask = np.asarray(p["fixed"], dtype=bool).reshape(-1, N)
    return sim


def _cases(p):
    return [LoadCase(loads=0 if c.get("F") is None else c["F"], acceleration=c.get("g"), eigenstrain=c.get("eps"), weight=c.get("w", 1.0))
            for c in p["cases"]]


def _objective(name, aggregate="sum", **kw):
    p = lc.problem(name)
    sim = _simulator(p)
    return sim, LoadCaseComplianceObjective(sim, _cases(p), aggregate=aggregate, P=lc.P_NORM, **kw)


# ---- the public assembly ----

@pytest.mark.parametrize("ne", [(7, 5), (12, 10, 9)], ids=_name)
def test_assemble_load_of_an_eigenstrain_matches_the_torch_stress_load(ne):
    N = len(ne)
    h = EDGES[N]
    rng = np.random.default_rng(77)
    rho = rng.uniform(0.2, 1.0, size=int(np.prod(ne)))
    A = rng.standard_normal((3 if N == 2 else 6,) * 2)
    D = lc.hc.isotropic_D(1.3, 0.3, N) + 0.05 * (A + A.T)
    eps = rng.standard_normal((N, N))
    eps = eps + eps.T
    p = dict(ne=ne, h=h, rho=rho, fixed=np.zeros((sc.num_nodes(ne), N), dtype=bool))
    sim = _simulator(p, ElasticityTensor.fromD(D, N))
    got = loadcases.assembleLoad_device(sim, LoadCase(loads=0, eigenstrain=eps))
    E = lc.hc.moduli(rho, lc.E0, lc.EMIN, lc.GAMMA)[0]
    Lt = lc.eigenstrain_pattern(sim.ETensor.D, h, eps)
    ref = lc.kernel_assemble(ne, None, Lt, None, E, dtype=np.longdouble)
    floor = _rel(lc.kernel_assemble(ne, None, Lt, None, E), ref)
    sigma = sim.ETensor.doubleContract(eps)
    Edev = (lc.EMIN + sim.getDensities_device()[:rho.size] ** lc.GAMMA * (lc.E0 - lc.EMIN)).reshape(ne)
    old = pv._stress_load(sigma, np.array(h), 1, Edev)
    scale = float(np.abs(ref).max())
    err = float((got - old).abs().max()) / scale
    print("assembleLoad %s: against _stress_load %.2e, against the restatement %.2e and %.2e (floor %.2e, bound %.2e)"
          % (_name(ne), err, _rel(got.cpu().numpy().reshape(-1), ref), _rel(old.cpu().numpy().reshape(-1), ref), floor, MARGIN * floor))
    assert got.shape == (sim.numNodes(), N) and err < MARGIN * floor
    assert _rel(got.cpu().numpy().reshape(-1), ref) < MARGIN * floor
    assert np.array_equal(loadcases.assembleLoad(sim, LoadCase(loads=0, eigenstrain=eps)), got.cpu().numpy())


def test_assemble_load_of_every_kind_and_loads_from_file(tmp_path):
    p = lc.problem("arch2")
    r = lc.reference("arch2")
    sim = _simulator(p)
    for i, case in enumerate(_cases(p)):
        f = loadcases.assembleLoad(sim, case).reshape(-1)
        assert np.abs(f - r["f"][i]).max() < 1e-14 * np.abs(r["f"][i]).max(), i
        assert not f[r["fixed"]].any()
    # the simulator's own load vector, zero, and the mass law
    sim.setLoads_device(torch.from_numpy(p["cases"][0]["F"]).cuda())
    assert np.abs(loadcases.assembleLoad(sim, LoadCase()).reshape(-1) - r["f"][0]).max() < 1e-14 * np.abs(r["f"][0]).max()
    assert not loadcases.assembleLoad(sim, LoadCase(loads=0)).any()
    law = dict(massDensity=2.5, massExponent=2.0, lowDensityCut=0.4)
    m = lc.mass_law(p["rho"], **law)[0]
    want = lc.kernel_assemble(p["ne"], lc.body_pattern(p["h"], (0.3, -1.0)), None, m, None, r["fixed"])
    got = loadcases.assembleLoad(sim, LoadCase(loads=0, acceleration=(0.3, -1.0)), mass=law).reshape(-1)
    assert np.abs(got - want).max() < 1e-14 * np.abs(want).max()
    assert np.array_equal(loadcases.thermalStrain(1.5e-5, 40.0, 3), 1.5e-5 * 40.0 * np.eye(3))
    # the force regions of a boundary-condition file, without touching the simulator
    bc = str(tmp_path / "bridge.json")
    box = lambda lo, hi: {"minCorner": lo, "maxCorner": hi}
    with open(bc, "w") as fh:                                           # the regions of bcs/2d/bridge.bc and a second, partial force region
        json.dump({"regions": [{"type": "dirichlet", "value": [0, 0, 0], "box%": box([-0.0001, -0.0001, 0], [0.0001, 1.0001, 0])},
                               {"type": "dirichletx", "value": [0, 0, 0], "box%": box([0.9999, -0.0001, 0], [1.0001, 1.0001, 0])},
                               {"type": "force", "value": [0, -1, 0], "box%": box([-0.0001, 0.9999, 0], [1.0001, 1.0001, 0])},
                               {"type": "force", "value": [0.5, 0, 0], "box": box([1.9, 0.2, 0], [2.1, 0.6, 0])}]}, fh)
    a =pv.TensorProductSimulator([1, 1], [np.zeros(2), np.array([2.0, 1.0])], [16, 8])
    b = pv.TensorProductSimulator([1, 1], [np.zeros(2), np.array([2.0, 1.0])], [16, 8])
    F = loadcases.loadsFromFile(a, bc)
    assert not a.dirichletMask.any() and not a.buildLoadVector().any()
    b.applyDisplacementsAndLoadsFromFile(bc)
    assert F.is_cuda and torch.equal(F, b.buildLoadVector_device()) and abs(float(F[:, 1].sum()) + 1.0) < 1e-14


# ---- the objective ----

def test_one_fixed_case_is_the_compliance_objective():
    ne, h, D, rho, f, fixed = sc.case("16x12")
    p = dict(ne=ne, h=h, rho=rho, fixed=fixed)
    sim = _simulator(p)
    sim.setLoads_device(torch.from_numpy(f).cuda())
    ref = pv.ComplianceObjective(sim)
    obj = LoadCaseComplianceObjective(sim, [LoadCase()])
    assert obj.evaluate() == ref.evaluate() == obj.case(0).evaluate()                                 # bit for bit
    assert torch.equal(obj._u, ref._u)
    g, want = obj.gradient_device(), sim.complianceGradient_device(ref._u)
    u = ref._u.cpu().numpy().reshape(1, -1)
    dE = lc.hc.moduli(rho, lc.E0, lc.EMIN, lc.GAMMA)[1]
    args = (ne, lc.hc.element_constants(D, h)[0], None, None, dE, None, u, [-0.5], None, None)
    long = lc.kernel_gradient(*args, dtype=np.longdouble)
    floor = _rel(lc.kernel_gradient(*args), long)
    err = float((g - want).abs().max() / want.abs().max())
    print("one fixed case: gradient against complianceGradient_device %.2e, against the restatement %.2e (floor %.2e, bound %.2e)"
          % (err, _rel(g.cpu().numpy(), long), floor, MARGIN * floor))
    assert err < MARGIN * floor and bool((g <= 0).all())
    assert torch.equal(obj.case(0).gradient_device(), g)


@pytest.mark.parametrize("aggregate", ["sum", "pnorm"])
@pytest.mark.parametrize("name", ["arch2", "block3"])
def test_direct_path_matches_the_dense_chain(name, aggregate):
    ref = lc.reference(name, aggregate)
    sim, obj = _objective(name, aggregate)
    J, c, g = obj.evaluate(), obj.compliances(), obj.gradient()
    errs = abs(J - ref["J"]) / ref["J"], float((np.abs(c - ref["c"]) / ref["c"]).max()), np.abs(g - ref["gradient"]).max() / np.abs(ref["gradient"]).max()
    print("direct %s %s: J %.2e, c %.2e, gradient %.2e (bound %.1e); %d positive and %d negative entries"
          % (name, aggregate, *errs, TOL_DIRECT, (g > 0).sum(), (g < 0).sum()))
    assert max(errs) < TOL_DIRECT
    assert np.abs(obj.caseCoefficients() - ref["a"]).max() < 1e-10 * ref["a"].max()
    U, F = obj.displacements_device(), obj.loads_device()
    k = len(ref["c"])
    assert U.shape == F.shape == (k, sim.numNodes(), sim.N) and obj._u.data_ptr() == U.data_ptr()
    assert np.abs(F.cpu().numpy().reshape(k, -1) - ref["f"]).max() < 1e-13 * np.abs(ref["f"]).max()
    assert np.abs(U.cpu().numpy().reshape(k, -1) - ref["u"]).max() < 1e-10 * np.abs(ref["u"]).max()
    for i in range(k):
        view = obj.case(i)
        gi = view.gradient_device().cpu().numpy()
        assert view._sim is sim and view._u is obj.case(i)._u and view.evaluate() == view.compliance() == c[i]
        assert np.abs(gi - ref["case_gradients"][i]).max() < TOL_DIRECT * np.abs(ref["case_gradients"][i]).max()
        assert view.designDependentLoad == (i > 0) and not hasattr(view, "_mg")
        assert torch.equal(view._f, F[i])
    assert (g > 0).any() and (g < 0).any()
    # one factorisation per design serves every case
    n0 = sim.numDirectFactorizations()
    for s in (0.9, 0.8):
        obj.updateCache(torch.from_numpy(s * lc.problem(name)["rho"]).cuda())
        n0 += 1
        assert sim.numDirectFactorizations() == n0
    u0 = obj._u
    obj.updateCache(torch.from_numpy(0.8 * lc.problem(name)["rho"]).cuda())                          # the same densities: the factor is kept
    assert sim.numDirectFactorizations() == n0 and obj._u is not u0
    want = lc.evaluate(lc.problem(name), 0.8 * lc.problem(name)["rho"], aggregate)
    assert abs(obj.evaluate() - want["J"]) < TOL_DIRECT * want["J"]
    assert np.abs(obj.gradient() - want["gradient"]).max() < TOL_DIRECT * np.abs(want["gradient"]).max()


@pytest.mark.parametrize("aggregate", ["sum", "pnorm"])
def test_multigrid_path(aggregate):
    name = "block3even"
    ref = lc.reference(name, aggregate)
    p = lc.problem(name)
    sim = _simulator(p)
    mg = sim.multigridSolver(1)
    obj = LoadCaseComplianceObjective(mg, _cases(p), aggregate=aggregate, P=lc.P_NORM, skipSolve=True)
    assert (obj.cgIter, obj.tol, obj.mgIterations, obj.mgSmoothingIterations, obj.fullMultigrid, obj.zeroInit) == (100, 1e-5, 1, 2, True, False)
    obj.tol, obj.cgIter = 1e-12, 400
    obj.updateCache(None)
    J, c, g = obj.evaluate(), obj.compliances(), obj.gradient()
    errs = abs(J - ref["J"]) / ref["J"], float((np.abs(c - ref["c"]) / ref["c"]).max()), np.abs(g - ref["gradient"]).max() / np.abs(ref["gradient"]).max()
    first = obj.iterations()
    print("multigrid %s: J %.2e, c %.2e (bound %.1e), gradient %.2e (bound %.1e); iterations %s"
          % (aggregate, *errs[:2], TOL_MG_VALUE, errs[2], TOL_MG_GRADIENT, first))
    assert errs[0] < TOL_MG_VALUE and errs[1] < TOL_MG_VALUE and errs[2] < TOL_MG_GRADIENT
    view = obj.case(1)
    assert view._mg is mg and (view.cgIter, view.tol, view.fullMultigrid) == (400, 1e-12, True)
    # a second update at the same densities starts every case from its own displacement
    u0 = obj._u
    obj.updateCache(torch.from_numpy(p["rho"]).cuda())
    print("  warm start: iterations %s" % obj.iterations())
    assert obj.iterations() == [0, 0, 0] and min(first) > 0 and obj._u is not u0
    assert abs(obj.evaluate() - J) < 1e-13 * J


@pytest.mark.parametrize("kind", ["isotropic", "orthotropic"])
@pytest.mark.parametrize("dim", ["2", "3"])
def test_free_thermal_expansion_on_the_device(dim, kind):
    ne, h = lc.FREE[dim]
    N = len(ne)
    D = lc.free_tensor(dim, kind)
    eu, ec, p, r = lc.free_expansion(ne, h, D, 0.01)
    sim = _simulator(p, ElasticityTensor.fromD(D, N))
    obj = LoadCaseComplianceObjective(sim, [LoadCase(loads=0, eigenstrain=loadcases.thermalStrain(0.01, 1.0, N))])
    u, c = obj._u.cpu().numpy().reshape(-1), obj.compliances()[0]
    errs = np.abs(u - r["want_u"]).max() / np.abs(r["want_u"]).max(), abs(c - r["want_c"]) / r["want_c"]
    bounds = 10.0 * lc.FREE_U_MEASURED[(dim, kind)], lc.free_c_bound(dim, kind)
    print("free expansion on the device %s %s: u %.2e (bound %.2e), c %.2e (bound %.2e)" % (dim, kind, errs[0], bounds[0], errs[1], bounds[1]))
    assert errs[0] < bounds[0] and errs[1] < bounds[1]


# ---- the design loops ----

def test_three_oc_steps_with_two_fixed_load_cases():
    name = "arch2_traffic"
    p = lc.problem(name)
    sim, obj = _objective(name)
    assert bool((obj.gradient_device() <= 0).all())
    problem = pv.TopologyOptimizationProblem(sim, obj, [pv.TotalVolumeConstraint(0.5)], [])
    problem.setVars(torch.full((sim.numElements(),), 0.5, dtype=torch.float64, device="cuda"))
    J = [problem.evaluateObjective()]
    opt = pv.OCOptimizer(problem)
    for _ in range(3):
        opt.step()
        J.append(problem.evaluateObjective())
    x = problem.getVars()
    want = lc.evaluate(p, x, want_gradient=False)["J"]
    print("three OC steps: J %s, restatement at the final densities %.2e" % (" -> ".join("%.6f" % v for v in J), abs(J[-1] - want) / want))
    assert J[3] < J[2] < J[1] < J[0]
    assert abs(J[-1] - want) < TOL_DIRECT * want and abs(x.mean() - 0.5) < 1e-5


def test_three_mma_steps_on_the_arch_under_its_own_weight_and_two_traffic_loads():
    name = "arch2_bridge"
    p = lc.problem(name)
    sim, obj = _objective(name)
    problem = pv.TopologyOptimizationProblem(sim, obj, [pv.TotalVolumeConstraint(0.4)], [])
    problem.setVars(torch.full((sim.numElements(),), 0.4, dtype=torch.float64, device="cuda"))
    g = obj.gradient()
    assert (g > 0).any() and (g < 0).any()
    J = [problem.evaluateObjective()]
    opt = mma.MMAOptimizer(problem, xmin=0.05, xmax=1.0, move=0.1)
    for _ in range(3):
        change = opt.step()
        assert 0.0 < change <= 0.1 * 0.95 + 1e-15
        J.append(problem.evaluateObjective())
    x = problem.getVars()
    want = lc.evaluate(p, x, want_gradient=False)["J"]
    print("three MMA steps: J %s, volume %.6f, restatement at the final densities %.2e" % (" -> ".join("%.6f" % v for v in J), x.mean(), abs(J[-1] - want) / want))
    assert J[-1] < J[0]
    assert abs(J[-1] - want) < TOL_DIRECT * want


def test_bound_formulation_of_min_max_compliance():
    """the stiffest design at half the volume whose two traffic cases each stay under a bound of their own: one constraint per case
    view beside the aggregate objective, one solve per step for all three"""
    name = "arch2_traffic"
    sim, obj = _objective(name)
    x0 = torch.full((sim.numElements(),), 0.5, dtype=torch.float64, device="cuda")
    obj.updateCache(x0)
    start = obj.compliances()
    bounds = 0.95 * start
    caps = [mma.ObjectiveConstraint(obj.case(i), bounds[i]) for i in range(2)]
    problem = pv.TopologyOptimizationProblem(sim, obj, [pv.TotalVolumeConstraint(0.5)] + caps, [])
    problem.setVars(x0)
    opt = mma.MMAOptimizer(problem, xmin=0.05, xmax=1.0, move=0.1)
    n0 = sim.numDirectFactorizations()
    for step in range(3):
        opt.step()
        lam = opt.lambdas
        assert lam.shape == (3,) and np.isfinite(lam).all() and (lam >= 0).all()
        assert sim.numDirectFactorizations() - n0 == step + 1               # both case views find the objective's solve
    values = problem.evaluateConstraints()
    print("bound formulation: c %s -> %s under the bounds %s, constraints %s, multipliers %s" % (start, obj.compliances(), bounds, values, lam))
    assert np.allclose(values[1:], 1.0 - obj.compliances() / bounds, rtol=0, atol=1e-15)
    assert sim.numDirectFactorizations() - n0 == 3
    for i in range(2):
        assert torch.equal(caps[i].backprop_dev(problem.getVars_device()), obj.case(i).gradient_device() * (-1.0 / bounds[i]))


# ---- beside the stress and buckling measures ----

def test_a_stress_cap_on_one_case_adds_no_primal_solve():
    p = lc.problem("arch2_traffic")
    sim = _simulator(p)
    cases = [LoadCase(loads=0, acceleration=(0.0, -1.0))] + _cases(p)
    obj = LoadCaseComplianceObjective(sim, cases)
    peak = stress.PNormStressObjective(obj.case(1))
    cap = mma.ObjectiveConstraint(peak, 2.0 * peak.evaluate())
    problem = pv.TopologyOptimizationProblem(sim, obj, [pv.TotalVolumeConstraint(0.6), cap], [])
    problem.setVars(torch.from_numpy(0.9 * p["rho"]).cuda())
    us, n0 = [obj.case(i)._u for i in range(3)], sim.numDirectFactorizations()
    values = problem.evaluateConstraints()
    rows = problem.evaluateConstraintsJacobian_device()
    assert all(obj.case(i)._u is us[i] for i in range(3)) and sim.numDirectFactorizations() == n0
    assert values[1] == 1.0 - peak.evaluate() / cap.upperBound and rows[1].shape == (sim.numElements(),)
    # the stress of case 1 is the stress of a plain compliance objective with that load
    sim2 = _simulator(dict(p, rho=0.9 * p["rho"]))
    sim2.setLoads_device(torch.from_numpy(p["cases"][0]["F"]).cuda())
    plain = stress.PNormStressObjective(pv.ComplianceObjective(sim2))
    assert abs(plain.evaluate() - peak.evaluate()) < 1e-12 * plain.evaluate()
    assert float((plain.gradient_device() - peak.gradient_device()).abs().max()) < 1e-11 * float(plain.gradient_device().abs().max())
    # measures whose adjoint gradient lacks the lambda^T df/drho term refuse a design-dependent case
    with pytest.raises(RuntimeError, match="depends on the design"):
        stress.PNormStressObjective(obj.case(0))
    with pytest.raises(RuntimeError, match="depends on the design"):
        buckling.BucklingObjective(obj.case(0))
    # and so does the objective itself, which stands for its case 0
    assert obj.designDependentLoad and not LoadCaseComplianceObjective(sim, _cases(p)).designDependentLoad
    with pytest.raises(RuntimeError, match="depends on the design"):
        stress.PNormStressObjective(obj)
    with pytest.raises(RuntimeError, match="depends on the design"):
        buckling.BucklingObjective(obj)
    assert buckling.BucklingObjective(obj.case(2), numModes=2).solved is obj.case(2)


# ---- autograd ----

@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_backward_is_the_gradient_times_the_incoming_gradient(dtype):
    name = "arch2"
    ne = lc.problem(name)["ne"]
    sim, obj = _objective(name, "pnorm")
    rho = torch.from_numpy(lc.problem(name)["rho"]).cuda().to(dtype).reshape(ne).requires_grad_(True)
    J = loadcases.aggregateCompliance(rho, obj)
    J.backward()
    assert rho.grad.dtype == dtype and rho.grad.shape == rho.shape and J.dtype == torch.float64
    assert float(J.detach()) == obj.evaluate()
    assert torch.equal(rho.grad.reshape(-1), obj.gradient_device().to(dtype))              # bit for bit
    rho2 = rho.detach().clone().requires_grad_(True)
    (2.5 * loadcases.aggregateCompliance(rho2, obj)).backward()
    assert torch.equal(rho2.grad.reshape(-1), (2.5 * obj.gradient_device()).to(dtype))
    J3 = loadcases.aggregateCompliance(rho.detach().clone().requires_grad_(True), obj)
    obj.updateCache(None)
    with pytest.raises(RuntimeError, match="updated between forward and backward"):
        J3.backward()


# ---- refusals ----

def test_refusals():
    q2 = pv.TensorProductSimulator([2, 2], [np.zeros(2), np.ones(2)], [2, 2])
    with pytest.raises(RuntimeError, match="degree-1"):
        LoadCaseComplianceObjective(q2, [LoadCase()])
    with pytest.raises(RuntimeError, match="degree-1"):
        loadcases.assembleLoad(q2, LoadCase(loads=0, acceleration=(0, -1)))
    padded = pv.TensorProductSimulator1_1_1([np.zeros(3), np.ones(3)], [2, 2, 2], _element_padding=(1, 0))
    with pytest.raises(RuntimeError, match="padding"):
        LoadCaseComplianceObjective(padded, [LoadCase()])
    with pytest.raises(RuntimeError, match="padding"):
        loadcases.assembleLoad(padded, LoadCase(loads=0, acceleration=(0, -1, 0)))
    sim, obj = _objective("arch2_traffic")
    nn = sim.numNodes()
    for cases in ([], [LoadCase()] * 9):
        with pytest.raises(RuntimeError, match="1 to 8 load cases"):
            LoadCaseComplianceObjective(sim, cases)
    for w in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="weight must be positive and finite"):
            LoadCase(weight=w)
    late = LoadCase()
    late.weight = 0.0
    with pytest.raises(RuntimeError, match="weight must be positive and finite"):
        LoadCaseComplianceObjective(sim, [late])
    for P in (0.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="P must be finite and at least 1"):
            LoadCaseComplianceObjective(sim, [LoadCase()], aggregate="pnorm", P=P)
    with pytest.raises(RuntimeError, match="aggregate"):
        LoadCaseComplianceObjective(sim, [LoadCase()], aggregate="max")
    with pytest.raises(TypeError, match="LoadCase"):
        LoadCaseComplianceObjective(sim, [np.zeros((nn, 2))])
    with pytest.raises(TypeError, match="massDensity"):
        LoadCaseComplianceObjective(sim, [LoadCase()], mass=dict(density=2.0))
    with pytest.raises(RuntimeError, match="massDensity and massExponent must be positive"):
        LoadCaseComplianceObjective(sim, [LoadCase(acceleration=(0, -1))], mass=dict(massDensity=-1.0))
    with pytest.raises(RuntimeError, match="Invalid input size"):
        LoadCaseComplianceObjective(sim, [LoadCase(loads=np.zeros((nn - 1, 2)))])
    with pytest.raises(RuntimeError, match="acceleration has 3 values"):
        LoadCaseComplianceObjective(sim, [LoadCase(acceleration=(0, -1, 0))])
    with pytest.raises(RuntimeError, match="eigenstrain is"):
        LoadCaseComplianceObjective(sim, [LoadCase(eigenstrain=np.eye(3))])
    with pytest.raises(RuntimeError, match="symmetric"):
        LoadCase(eigenstrain=[[0.0, 1.0], [0.0, 0.0]])
    with pytest.raises(IndexError):
        obj.case(2)
    lazy = LoadCaseComplianceObjective(sim, [LoadCase()], skipSolve=True)
    assert lazy._u is None
    with pytest.raises(RuntimeError, match="updateCache"):
        lazy.evaluate()
    values = np.zeros((nn, 2))
    values[0, 0] = 0.5
    sim.dirichletValues = values
    with pytest.raises(RuntimeError, match="nonzero Dirichlet"):
        LoadCaseComplianceObjective(sim, [LoadCase()])
    with pytest.raises(RuntimeError, match="nonzero Dirichlet"):
        loadcases.assembleLoad(sim, LoadCase())
