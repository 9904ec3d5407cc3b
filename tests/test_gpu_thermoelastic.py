"""-m gpu: the thermo-elastic coupling on the device (ndr_amd.thermoelastic, vfem_thermoelastic_*, LoadCase(temperature=...)): the three
kernels, the transposition identity, the uniform field, the coupled objective over the direct and the PCG paths, its case views, the
design loop and the autograd node, against tests/thermoelastic_cpu.py.

Bounds.  Every figure named "restatement" was measured on the CPU with tests/thermoelastic_cpu.py (tests/test_thermoelastic_cpu.py prints
them).
  Kernels (load, adjoint source, gradient): the reference is the restatement evaluated in np.longdouble; the rounding floor of the
    formula is what the same restatement in float64 differs from it, relative to the largest entry, and the bound is 16 times that
    floor (another summation order; the convention of tests/test_gpu_loadcases.py), computed per case and printed with it.
  Transposition x . adjoint_source(u) = u . load(x): ndof x 2^-52 of the sum of the magnitudes of all products |x_m| E_e |G_km| |u_k|
    (each side is a sum of that many rounded products; computed by the restatement from |x|, |G|, |u|).
  Uniform temperature against assembleLoad of the constant eigenstrain: 16 floors of the load restatement.
  Direct chain (J, every c_i, the gradient, the case views): max(1e-11, ten times the float64 floor of the restatement's chain, LU
    against Cholesky solves: 4.4e-13 values, 1.0e-12 gradient) = 1e-11 (thermoelastic_cpu.direct_bound).
  PCG chains (block3even, elastic multigrid-PCG on 2 levels and heat PCG, both to 1e-12): ten times what the restatement's chain with
    conjugate-gradient solves to 1e-12 differs from its dense chain by: 2.1e-13 values, 4.9e-13 gradient.
  Free expansion by the T_ref route: the bounds of tests/test_gpu_loadcases.py's free-expansion test.

Measured on an MI355X (DESIGN 3.17 has the same figures):
  load, 32 cases: 1.0e-16 .. 2.7e-16 of the largest entry against floors of 5.8e-17 .. 2.8e-16 (at most 1.8 floors); adjoint source, 48
    cases: 7.1e-17 .. 3.4e-16 against 9.4e-17 .. 7.4e-16 (at most 1.7 floors); gradient, 48 cases: 4.4e-18 .. 1.0e-16 against 1.4e-17 ..
    1.7e-15 (at most 1.0 floors).  The smallest floors are those of the 8-case gradient on 1 x 1 x 1 (3.82e-17 alone, 1.42e-17 added:
    one number, which the float64 restatement happens to round correctly), so their bounds are 6.1e-16 and 2.3e-16; the device
    writes the same double.  With the gradient kernel summing in plain fused multiply-adds these two cases were at 7.16e-16 and
    7.19e-16 and failed; the kernel now sums in twice the working precision and rounds once.
  in place, off-line buffers and a second run: bit-identical.  transposition: 2.1e-14 (40 x 37) and 5.7e-14 (12 x 10 x 9) against bounds
    of 9.5e-9 and 5.5e-8.  uniform temperature against assembleLoad: 2.6e-16 (7 x 5) / 2.2e-16 (12 x 10 x 9), bounds 1.8e-15 / 3.2e-15.
  direct chain: plate2 J 6.7e-13 / 8.4e-13, c 9.0e-13, gradient 1.6e-12 / 2.0e-12 (sum / pnorm), views 1.9e-12, 1.7e-13, 1.7e-12; block3
    J 6.9e-14 / 9.4e-14, c 9.7e-14, gradient 1.3e-13 / 2.0e-13, views 2.1e-13, 5.0e-15, 1.9e-13.
  PCG chains: J 6.4e-14 / 5.8e-14, c 1.0e-13, gradient 6.9e-14 / 7.0e-14 (heat Jacobi, 40 iterations), 6.5e-14 / 6.1e-14, 1.0e-13, 7.0e-14 /
    7.5e-14 (heat multigrid, 12 iterations); elastic 15 / 13 / 15 iterations.
  free expansion through T_ref: u 1.6e-13 / 4.7e-13 (16 x 6), 1.2e-12 / 1.5e-12 (6 x 4 x 3); c 8.4e-15 at worst.
  three MMA steps on the heated plate: J 286.75 -> 194.36 -> 151.90 -> 127.15, the restatement at the final densities within 1.1e-16;
    with the peak-temperature cap: one elastic and one thermal factorisation and three thermal solves per step.
  The whole file runs in 4 s.
  Against the parent commit every test fails at import: the module, the keyword and the entry points do not exist.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import loadcases_cpu as lc
import stress_cpu as sc
import thermal_cpu as tc
import thermoelastic_cpu as te

pytestmark = pytest.mark.gpu

from ndr_amd import ElasticityTensor, _lib, buckling, loadcases, mma, stress, thermal, thermoelastic      # noqa: E402
from ndr_amd import pyVoxelFEM as pv                                                                        # noqa: E402
from ndr_amd.loadcases import LoadCase, LoadCaseComplianceObjective                                         # noqa: E402
from ndr_amd.thermoelastic import TemperatureLoad                                                           # noqa: E402

MARGIN = 16.0
TOL_DIRECT = te.direct_bound()
TOL_CG_VALUE, TOL_CG_GRADIENT = 10 * te.CG_VALUE_MEASURED, 10 * te.CG_GRADIENT_MEASURED

# 1 x 1 and 1 x 1 x 1 have edge nodes only; 40 x 37 and 12 x 10 x 9 span several workgroups of the cell kernels along every axis (64
# lanes along the last axis by 4 rows, one block per layer of axis 0 in 3-D: 40 x 37 has 38 nodes along the last axis, so 5 x 70 and
# 3 x 3 x 70, with 71, cross the block edge at 64)
SHAPES = [(1, 1), (1, 1, 1), (7, 5), (40, 37), (5, 70), (6, 4, 5), (12, 10, 9), (3, 3, 70)]
LARGE = [(40, 37), (12, 10, 9)]
EDGES = tc.EDGES


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


# ---- the three kernels against the restatement in extended precision ----

def _draw(ne):
    N = len(ne)
    rng = np.random.default_rng(900 + int(np.prod(ne)) + N)
    nn, nel, ke, npe = sc.num_nodes(ne), int(np.prod(ne)), N * 2 ** N, 2 ** N
    c = dict(ne=ne, N=N, h=EDGES[N], G=rng.standard_normal((8, ke, npe)), E=rng.uniform(0.05, 1.0, size=nel),
             dE=rng.uniform(0.05, 1.0, size=nel), T=rng.standard_normal(nn), f=rng.standard_normal(nn * N), g=rng.standard_normal(nel),
             U=rng.standard_normal((8, nn * N)), a=rng.standard_normal(8), tref=rng.standard_normal(8),
             fixed=rng.uniform(size=(nn, N)) < 0.2, fixed_T=rng.uniform(size=nn) < 0.2)
    bits = np.zeros(nn, dtype=np.uint8)
    for a in range(N):
        bits |= c["fixed"][:, a].astype(np.uint8) << a
    c["bits"] = bits
    return c


VARIANTS = [("load", with_f, masked) for with_f in (False, True) for masked in (False, True)] + \
    [("source", k, masked) for k in (1, 3, 8) for masked in (False, True)] + [("gradient", k, added) for k in (1, 3, 8) for added in (False, True)]


@functools.lru_cache(maxsize=None)
def _kernel_case(ne):
    """the random data of a grid with the longdouble reference and the float64 floor of every variant, computed once and shared"""
    c = _draw(ne)
    c["ref"], c["floor"] = {}, {}
    for key in VARIANTS:
        fn, args = {"load": (te.kernel_load, _load_args), "source": (te.kernel_adjoint_source, _source_args),
                    "gradient": (te.kernel_gradient, _gradient_args)}[key[0]]
        c["ref"][key] = fn(*args(c, key[1], key[2]), dtype=np.longdouble)
        c["floor"][key] = _rel(fn(*args(c, key[1], key[2])), c["ref"][key])
    return c


def _load_args(c, with_f, masked):
    return (c["ne"], c["G"][0], c["tref"][0], c["E"], c["T"], c["fixed"] if masked else None, c["f"] if with_f else None)


def _run_load(c, with_f, masked, off=False, in_place=False):
    args, keep = _head(c["ne"], c["h"])
    G = np.ascontiguousarray(c["G"][0])
    E, T = _dev(c["E"], off), _dev(c["T"], off)
    f_in = _dev(c["f"], off) if with_f else None
    out = f_in if in_place else _dev(np.full(c["f"].shape, np.nan), off)
    mask = torch.from_numpy(c["bits"]).cuda() if masked else None
    _lib.check(_lib.load().vfem_thermoelastic_load(*args, _dp(G), float(c["tref"][0]), _p(E), _p(T), _p(mask), _p(f_in), _p(out),
                                                   pv._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("with_f", [False, True], ids=["alone", "added"])
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_load_kernel_matches_the_restatement(ne, with_f, masked):
    c = _kernel_case(ne)
    ref, floor = c["ref"][("load", with_f, masked)], c["floor"][("load", with_f, masked)]
    out = _run_load(c, with_f, masked)
    err = _rel(out.cpu().numpy(), ref)
    print("load %s %s %s: %.2e (floor %.2e, bound %.2e)" % (_name(ne), "added" if with_f else "alone", "masked" if masked else "free", err,
                                                          floor, MARGIN * floor))
    assert err < MARGIN * floor
    if masked:
        assert not out.cpu().numpy()[c["fixed"].reshape(-1)].any()
    assert torch.equal(_run_load(c, with_f, masked), out)                                             # run to run


@pytest.mark.parametrize("ne", LARGE, ids=_name)
def test_load_in_place_and_on_buffers_8_bytes_off_a_16_byte_line(ne):
    c = _kernel_case(ne)
    out = _run_load(c, True, True)
    assert torch.equal(_run_load(c, True, True, in_place=True), out)
    assert torch.equal(_run_load(c, True, True, off=True), out)
    assert torch.equal(_run_load(c, True, True, off=True, in_place=True), out)


def _source_args(c, k, masked):
    return (c["ne"], c["a"][:k], c["G"][:k], c["E"], c["U"][:k], c["fixed_T"] if masked else None)


def _run_source(c, k, masked, off=False):
    args, keep = _head(c["ne"], c["h"])
    a, G = np.ascontiguousarray(c["a"][:k]), np.ascontiguousarray(c["G"][:k])
    E, U = _dev(c["E"], off), _dev(c["U"][:k], off)
    fixed = torch.from_numpy(c["fixed_T"].astype(np.uint8)).cuda() if masked else None
    q = _dev(np.full(c["T"].shape, np.nan), off)
    _lib.check(_lib.load().vfem_thermoelastic_adjoint_source(*args, k, _dp(a), _dp(G), _p(E), _p(U), _p(fixed), _p(q), pv._stream()))
    torch.cuda.synchronize()
    return q


@pytest.mark.parametrize("masked", [False, True], ids=["free", "fixed"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_adjoint_source_kernel_matches_the_restatement(ne, k, masked):
    c = _kernel_case(ne)
    ref, floor = c["ref"][("source", k, masked)], c["floor"][("source", k, masked)]
    q = _run_source(c, k, masked)
    err = _rel(q.cpu().numpy(), ref)
    print("adjoint source %s, %d cases, %s: %.2e (floor %.2e, bound %.2e)" % (_name(ne), k, "fixed" if masked else "free", err, floor,
                                                                             MARGIN * floor))
    assert err < MARGIN * floor
    if masked:
        assert not q.cpu().numpy()[c["fixed_T"]].any()
    assert torch.equal(_run_source(c, k, masked), q)                                                  # run to run


@pytest.mark.parametrize("ne", LARGE, ids=_name)
def test_adjoint_source_on_buffers_8_bytes_off_a_16_byte_line(ne):
    c = _kernel_case(ne)
    assert torch.equal(_run_source(c, 3, True, off=True), _run_source(c, 3, True))


def _gradient_args(c, k, added):
    return (c["ne"], c["a"][:k], c["G"][:k], c["tref"][:k], c["dE"], c["T"], c["U"][:k], c["g"] if added else None)


def _run_gradient(c, k, added, off=False, in_place=False):
    args, keep = _head(c["ne"], c["h"])
    a, G, tref = (np.ascontiguousarray(c[n][:k]) for n in ("a", "G", "tref"))
    dE, T, U = _dev(c["dE"], off), _dev(c["T"], off), _dev(c["U"][:k], off)
    g_in = _dev(c["g"], off) if added else None
    out = g_in if in_place else _dev(np.full(c["g"].shape, np.nan), off)
    _lib.check(_lib.load().vfem_thermoelastic_gradient(*args, k, _dp(a), _dp(G), _dp(tref), _p(dE), _p(T), _p(U), _p(g_in), _p(out),
                                                       pv._stream()))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("added", [False, True], ids=["alone", "added"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_gradient_kernel_matches_the_restatement(ne, k, added):
    c = _kernel_case(ne)
    ref, floor = c["ref"][("gradient", k, added)], c["floor"][("gradient", k, added)]
    g = _run_gradient(c, k, added)
    err = _rel(g.cpu().numpy(), ref)
    print("gradient %s, %d cases, %s: %.2e (floor %.2e, bound %.2e)" % (_name(ne), k, "added" if added else "alone", err, floor, MARGIN * floor))
    assert err < MARGIN * floor
    assert torch.equal(_run_gradient(c, k, added), g)                                                 # run to run


@pytest.mark.parametrize("ne", LARGE, ids=_name)
def test_gradient_in_place_and_on_buffers_8_bytes_off_a_16_byte_line(ne):
    c = _kernel_case(ne)
    out = _run_gradient(c, 3, True)
    assert torch.equal(_run_gradient(c, 3, True, in_place=True), out)
    assert torch.equal(_run_gradient(c, 3, True, off=True), out)
    assert torch.equal(_run_gradient(c, 3, True, off=True, in_place=True), out)


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


def _heat(p, **kw):
    """the heat simulator of a problem and the objective that solves it (not solved yet)"""
    ne, h, ht = p["ne"], p["h"], p["heat"]
    heat = thermal.HeatConductionSimulator([np.zeros(len(ne)), np.array(ne) * np.array(h)], list(ne))
    heat.conductivity = ht.get("k", 1.0)
    heat.fixedTemperatureMask = np.asarray(ht["fixed"], dtype=bool)
    heat.setHeatSources(nodal=ht.get("nodal"), volumetric=ht.get("volumetric"))
    return heat, thermal.ThermalComplianceObjective(heat, skipSolve=True, **kw)


def _cases(p, th):
    return [LoadCase(loads=0 if c.get("F") is None else c["F"], acceleration=c.get("g"), eigenstrain=c.get("eps"), weight=c.get("w", 1.0),
                     temperature=None if c.get("alpha") is None else TemperatureLoad(th, c["alpha"], c.get("tref", 0.0)))
            for c in p["cases"]]


def _objective(name, aggregate="sum", solver=None, heat_kw=None, **kw):
    p = te.problem(name)
    sim = _simulator(p)
    heat, th = _heat(p, **(heat_kw or {}))
    obj = LoadCaseComplianceObjective(sim if solver is None else solver(sim), _cases(p, th), aggregate=aggregate, P=lc.P_NORM, **kw)
    return sim, heat, th, obj


def _errors(obj, ref):
    J, c, g = obj.evaluate(), obj.compliances(), obj.gradient()
    return (abs(J - ref["J"]) / ref["J"], float((np.abs(c - ref["c"]) / ref["c"]).max()),
            float(np.abs(g - ref["gradient"]).max() / np.abs(ref["gradient"]).max())), g


# ---- identities of the kernels ----

@pytest.mark.parametrize("ne", [(7, 5), (40, 37), (12, 10, 9)], ids=_name)
def test_the_adjoint_source_is_the_transpose_of_the_load(ne):
    c = _kernel_case(ne)
    N = c["N"]
    sim = _simulator(dict(ne=ne, h=c["h"], rho=np.full(int(np.prod(ne)), 0.5), fixed=np.zeros((sc.num_nodes(ne), N), dtype=bool)))
    x, u, G, E = c["T"], c["U"][0], c["G"][0], c["E"]
    f = thermoelastic.thermalLoad_device(sim, G, x, 0.0, E=E, masked=False)
    q = thermoelastic.adjointSource_device(sim, [1.0], G[None], u, E=E)
    lhs, rhs = float(torch.dot(_dev(x), q)), float(torch.dot(_dev(u), f.reshape(-1)))
    magnitude = float(np.abs(x) @ te.kernel_adjoint_source(ne, [1.0], np.abs(G)[None], E, np.abs(u)[None]))
    bound = u.size * 2.0 ** -52 * magnitude
    print("transposition %s: x . q = %.15e, u . f = %.15e, difference %.2e (bound %.2e)" % (_name(ne), lhs, rhs, abs(lhs - rhs), bound))
    assert f.shape == (sim.numNodes(), N) and q.shape == (sim.numNodes(),)
    assert abs(lhs - rhs) < bound


@pytest.mark.parametrize("ne", [(7, 5), (12, 10, 9)], ids=_name)
def test_a_uniform_temperature_is_the_load_of_the_constant_eigenstrain(ne):
    N = len(ne)
    h = EDGES[N]
    rng = np.random.default_rng(78)
    rho = rng.uniform(0.2, 1.0, size=int(np.prod(ne)))
    A = rng.standard_normal((3 if N == 2 else 6,) * 2)
    D = lc.hc.isotropic_D(1.3, 0.3, N) + 0.05 * (A + A.T)
    alpha, deltaT = 1.5e-2, 40.0
    fixed = rng.uniform(size=(sc.num_nodes(ne), N)) < 0.2
    sim = _simulator(dict(ne=ne, h=h, rho=rho, fixed=fixed), ElasticityTensor.fromD(D, N))
    G = thermoelastic.couplingMatrix(sim, alpha)
    T = np.full(sim.numNodes(), deltaT)
    got = thermoelastic.thermalLoad_device(sim, G, T)
    old = loadcases.assembleLoad_device(sim, LoadCase(loads=0, eigenstrain=loadcases.thermalStrain(alpha, deltaT, N)))
    E = lc.hc.moduli(rho, lc.E0, lc.EMIN, lc.GAMMA)[0]
    args = (ne, te.coupling_matrix(sim.ETensor.D, h, alpha), 0.0, E, T, fixed)
    ref = te.kernel_load(*args, dtype=np.longdouble)
    floor = _rel(te.kernel_load(*args), ref)
    err = float((got - old).abs().max()) / float(np.abs(ref).max())
    print("uniform temperature %s: against assembleLoad %.2e, against the restatement %.2e (floor %.2e, bound %.2e)"
          % (_name(ne), err, _rel(got.cpu().numpy().reshape(-1), ref), floor, MARGIN * floor))
    assert err < MARGIN * floor and _rel(got.cpu().numpy().reshape(-1), ref) < MARGIN * floor
    # T_ref takes the field off again
    assert not thermoelastic.thermalLoad_device(sim, G, T, referenceTemperature=deltaT).any()


# ---- the objective ----

@pytest.mark.parametrize("aggregate", ["sum", "pnorm"])
@pytest.mark.parametrize("name", ["plate2", "block3"])
def test_direct_path_matches_the_dense_chain(name, aggregate):
    ref = te.reference(name, aggregate)
    p = te.problem(name)
    sim, heat, th, obj = _objective(name, aggregate, skipSolve=True)
    solves = []
    inner = th._solve
    th._solve = lambda Q, last=None: (solves.append(1), inner(Q, last))[1]
    n_el, n_th = sim.numDirectFactorizations(), heat.numDirectFactorizations()
    obj.updateCache(None)
    assert (sim.numDirectFactorizations(), heat.numDirectFactorizations(), len(solves)) == (n_el + 1, n_th + 1, 1)
    errs, g = _errors(obj, ref)
    assert len(solves) == 2                                                    # one thermal adjoint solve for all cases
    obj.gradient_device()
    assert len(solves) == 2 and heat.numDirectFactorizations() == n_th + 1     # kept
    print("direct %s %s: J %.2e, c %.2e, gradient %.2e (bound %.1e); %d positive and %d negative entries"
          % (name, aggregate, *errs, TOL_DIRECT, (g > 0).sum(), (g < 0).sum()))
    assert max(errs) < TOL_DIRECT
    assert (g > 0).any() and (g < 0).any()
    assert np.abs(th.temperature() - ref["T"]).max() < 1e-10 * np.abs(ref["T"]).max()
    F = obj.loads_device().cpu().numpy().reshape(len(ref["c"]), -1)
    assert np.abs(F - ref["f"]).max() < 1e-10 * np.abs(ref["f"]).max()
    # every case view: its own gradient, with its own thermal adjoint solve for the heated one only
    for i in range(len(ref["c"])):
        view, before = obj.case(i), len(solves)
        gi = view.gradient_device().cpu().numpy()
        want = ref["case_gradients"][i]
        err = float(np.abs(gi - want).max() / np.abs(want).max())
        print("  case %d: gradient %.2e" % (i, err))
        assert err < TOL_DIRECT
        assert view.designDependentLoad == (i > 0) and len(solves) - before == (1 if i in ref["hot"] else 0)
    # another design: one elastic and one thermal factorisation, the heat simulator follows the densities
    x = torch.from_numpy(0.8 * p["rho"]).cuda()
    obj.updateCache(x)
    assert (sim.numDirectFactorizations(), heat.numDirectFactorizations()) == (n_el + 2, n_th + 2)
    assert torch.equal(heat.getDensities_device(), x)
    want = te.evaluate(p, 0.8 * p["rho"], aggregate)
    assert abs(obj.evaluate() - want["J"]) < TOL_DIRECT * want["J"]
    assert np.abs(obj.gradient() - want["gradient"]).max() < TOL_DIRECT * np.abs(want["gradient"]).max()


@pytest.mark.parametrize("preconditioner", ["jacobi", "multigrid"])
@pytest.mark.parametrize("aggregate", ["sum", "pnorm"])
def test_pcg_paths(aggregate, preconditioner):
    name = "block3even"
    ref = te.reference(name, aggregate)
    sim, heat, th, obj = _objective(name, aggregate, solver=lambda s: s.multigridSolver(1), skipSolve=True,
                                    heat_kw=dict(solver="pcg", preconditioner=preconditioner))
    obj.tol, obj.cgIter, th.tol = 1e-12, 400, 1e-12
    obj.updateCache(None)
    errs, g = _errors(obj, ref)
    print("pcg %s, heat %s: J %.2e, c %.2e (bound %.1e), gradient %.2e (bound %.1e); iterations %s, heat %d"
          % (aggregate, preconditioner, *errs[:2], TOL_CG_VALUE, errs[2], TOL_CG_GRADIENT, obj.iterations(), th.iterations))
    assert errs[0] < TOL_CG_VALUE and errs[1] < TOL_CG_VALUE and errs[2] < TOL_CG_GRADIENT
    if preconditioner == "multigrid":
        assert heat.numMultigridBuilds() == 1 and len(heat.multigridLevels()) == 2                   # the adjoint reused the hierarchy


@pytest.mark.parametrize("kind", ["isotropic", "orthotropic"])
@pytest.mark.parametrize("dim", ["2", "3"])
def test_free_expansion_through_the_reference_temperature(dim, kind):
    ne, h = lc.FREE[dim]
    N = len(ne)
    D = lc.free_tensor(dim, kind)
    eu, ec, p, r, ef = te.free_expansion(ne, h, D, 0.01)
    sim = _simulator(p, ElasticityTensor.fromD(D, N))
    heat, th = _heat(p)
    obj = LoadCaseComplianceObjective(sim, [LoadCase(loads=0, temperature=TemperatureLoad(th, 0.01, referenceTemperature=-1.0))])
    assert not th.temperature_device().any()
    u, c = obj._u.cpu().numpy().reshape(-1), obj.compliances()[0]
    errs = np.abs(u - r["want_u"]).max() / np.abs(r["want_u"]).max(), abs(c - r["want_c"]) / r["want_c"]
    bounds = 10.0 * lc.FREE_U_MEASURED[(dim, kind)], lc.free_c_bound(dim, kind)
    print("free expansion through T_ref %s %s: u %.2e (bound %.2e), c %.2e (bound %.2e)" % (dim, kind, errs[0], bounds[0], errs[1], bounds[1]))
    assert errs[0] < bounds[0] and errs[1] < bounds[1]


# ---- the design loop ----

def _plate_problem(extra=()):
    p = te.problem("plate2")
    sim, heat, th, obj = _objective("plate2", skipSolve=True)
    caps = [make(th) for make in extra]
    problem = pv.TopologyOptimizationProblem(sim, obj, [pv.TotalVolumeConstraint(0.4)] + caps, [])
    problem.setVars(torch.full((sim.numElements(),), 0.4, dtype=torch.float64, device="cuda"))
    return p, sim, heat, th, obj, problem


def test_three_mma_steps_on_a_clamped_heated_plate():
    p, sim, heat, th, obj, problem = _plate_problem()
    g = obj.gradient()
    assert (g > 0).any() and (g < 0).any()
    J = [problem.evaluateObjective()]
    opt = mma.MMAOptimizer(problem, xmin=0.05, xmax=1.0, move=0.1)
    for _ in range(3):
        change = opt.step()
        assert 0.0 < change <= 0.1 * 0.95 + 1e-15
        J.append(problem.evaluateObjective())
    x = problem.getVars()
    want = te.evaluate(p, x, want_gradient=False)["J"]
    print("three MMA steps: J %s, volume %.6f, restatement at the final densities %.2e (bound %.1e)"
          % (" -> ".join("%.6f" % v for v in J), x.mean(), abs(J[-1] - want) / want, TOL_DIRECT))
    assert abs(J[-1] - want) < TOL_DIRECT * want
    assert np.array_equal(heat.getDensities(), sim.getDensities()[:sim.numElements()])


def test_a_peak_temperature_cap_shares_the_heat_solve():
    """PNormTemperatureObjective on the thermal objective of the heated case, as a second constraint: it finds the temperature the
    load-case objective has just solved for and adds its own adjoint solve only"""
    peak = []
    def cap(th):
        peak.append(thermal.PNormTemperatureObjective(th, P=8.0))
        return mma.ObjectiveConstraint(peak[0], 1e3)
    p, sim, heat, th, obj, problem = _plate_problem([cap])
    solves = []
    inner = th._solve
    th._solve = lambda Q, last=None: (solves.append(1), inner(Q, last))[1]
    opt = mma.MMAOptimizer(problem, xmin=0.05, xmax=1.0, move=0.1)
    n_el, n_th = sim.numDirectFactorizations(), heat.numDirectFactorizations()
    for step in range(3):
        before = len(solves)
        opt.step()
        assert sim.numDirectFactorizations() - n_el == step + 1 and heat.numDirectFactorizations() - n_th == step + 1
        # per step: the temperature, the coupled adjoint of the objective and the adjoint of the cap
        assert len(solves) - before == 3
    assert peak[0]._u is th._u and peak[0].evaluate() >= peak[0].maxTemperature() > 0.0
    print("peak-temperature cap: J_8 = %.4f, max T = %.4f, %d thermal factorisations in 3 steps" % (peak[0].evaluate(), peak[0].maxTemperature(),
                                                                                                     heat.numDirectFactorizations() - n_th))


# ---- beside the other measures, autograd, refusals ----

def test_stress_and_buckling_measures_refuse_a_heated_case():
    sim, heat, th, obj = _objective("plate2")
    for i in (1, 2):
        with pytest.raises(RuntimeError, match="depends on the design"):
            stress.PNormStressObjective(obj.case(i))
        with pytest.raises(RuntimeError, match="depends on the design"):
            buckling.BucklingObjective(obj.case(i))
    assert stress.PNormStressObjective(obj.case(0)).evaluate() > 0.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_backward_is_the_gradient_times_the_incoming_gradient(dtype):
    name = "plate2"
    ne = te.problem(name)["ne"]
    sim, heat, th, obj = _objective(name, "pnorm")
    rho = torch.from_numpy(te.problem(name)["rho"]).cuda().to(dtype).reshape(ne).requires_grad_(True)
    J = loadcases.aggregateCompliance(rho, obj)
    J.backward()
    assert rho.grad.dtype == dtype and rho.grad.shape == rho.shape and J.dtype == torch.float64
    assert float(J.detach()) == obj.evaluate()
    assert torch.equal(rho.grad.reshape(-1), obj.gradient_device().to(dtype))              # bit for bit
    rho2 = rho.detach().clone().requires_grad_(True)
    (2.5 * loadcases.aggregateCompliance(rho2, obj)).backward()
    assert torch.equal(rho2.grad.reshape(-1), (2.5 * obj.gradient_device()).to(dtype))


def test_refusals():
    p = te.problem("plate2")
    sim = _simulator(p)
    heat, th = _heat(p)
    heat2, th2 = _heat(p)
    with pytest.raises(RuntimeError, match="share one ThermalComplianceObjective"):
        LoadCaseComplianceObjective(sim, [LoadCase(loads=0, temperature=TemperatureLoad(th, 0.1)),
                                          LoadCase(loads=0, temperature=TemperatureLoad(th2, 0.1))], skipSolve=True)
    # expansions and reference temperatures may differ per case
    two = LoadCaseComplianceObjective(sim, [LoadCase(loads=0, temperature=TemperatureLoad(th, 0.1)),
                                            LoadCase(loads=0, temperature=TemperatureLoad(th, [[0.2, 0.0], [0.0, 0.1]], 0.5))])
    assert two.numCases == 2 and np.isfinite(two.gradient()).all()
    other = thermal.HeatConductionSimulator([np.zeros(2), np.array([2.0, 0.75])], [16, 8])
    with pytest.raises(RuntimeError, match="grid .* is not the elastic simulator's"):
        LoadCaseComplianceObjective(sim, [LoadCase(temperature=TemperatureLoad(thermal.ThermalComplianceObjective(other, skipSolve=True), 0.1))])
    other = thermal.HeatConductionSimulator([np.zeros(2), np.array([2.0, 1.0])], [16, 6])
    with pytest.raises(RuntimeError, match="bounding box is not the elastic simulator's"):
        LoadCaseComplianceObjective(sim, [LoadCase(temperature=TemperatureLoad(thermal.ThermalComplianceObjective(other, skipSolve=True), 0.1))])
    with pytest.raises(RuntimeError, match="expansion must be"):
        TemperatureLoad(th, np.eye(3))
    with pytest.raises(RuntimeError, match="assembled by LoadCaseComplianceObjective"):
        loadcases.assembleLoad(sim, LoadCase(loads=0, temperature=TemperatureLoad(th, 0.1)))
    with pytest.raises(RuntimeError, match="Invalid input size"):
        thermoelastic.thermalLoad_device(sim, np.ones((8, 3)), np.zeros(sim.numNodes()))
    with pytest.raises(RuntimeError, match="ncases must be 1 to 8"):
        thermoelastic.adjointSource_device(sim, np.ones(9), np.ones((9, 8, 4)), np.zeros((9, sim.numNodes(), 2)))
