"""-m "not gpu": pins tests/thermoelastic_cpu.py, the restatement the GPU tests of ndr_amd.thermoelastic compare with, the closed form of
the coupling matrix, and the refusals that come before any device call (the three vfem_thermoelastic_* entry points, TemperatureLoad,
LoadCase(temperature=...)).

Measured with this file (printed by every test):
  closed-form G against the 2-point quadrature: at most 6.9e-16 of the largest entry; row sums against Lt of eps* = alpha: at most 6.2e-16
    (isotropic and orthotropic C, scalar and tensor alpha, 2-D and 3-D with unequal edges); the bound is 8 x 2^-52 = 1.8e-15.
  central differences of J, step 1e-5, entry by entry (every entry on plate2, every third on block3), relative to the largest entry of
    the gradient: plate2 sum 3.3e-8, pnorm 3.7e-8; block3 sum 5.5e-9, pnorm 7.7e-9 (the truncation error of the step: the heated
    case's load is itself a solution of the design).  The bound is 1e-6 and, pinning the figure, ten times what was measured.
    plate2 has 32 / 20 positive and 64 / 76 negative entries (sum / pnorm), block3 32 / 45 and 64 / 51; the thermal adjoint term has
    0.50 / 0.14 (plate2) and 0.57 / 0.043 (block3) of the norm of the whole gradient.
  uniform field (no source, T = 0, T_ref = -1, alpha = 0.01): the load is the constant-eigenstrain load to 2.2e-16 of its largest entry;
    u and c as tests/test_loadcases_cpu.py has them (1.9e-13 / 1.2e-13 / 8.5e-13 / 4.1e-13 and 2.2e-15 / 0 / 0 / 1.4e-16).
  the float64 floor of the chain (Cholesky against LU solves, plate2 and block3, both aggregates): values 4.4e-13, gradient 9.9e-13
    (recorded 4.4e-13 and 1.0e-12): the GPU's direct path is bounded at max(1e-11, ten times these) = 1e-11.
  chain with conjugate-gradient solves to 1e-12 (elastic and thermal) against the dense chain on block3even: values 2.0e-14, gradient
    4.8e-14 (recorded 2.1e-14 and 4.9e-14; the bounds of the PCG GPU tests are ten times the recorded figures).
"""
import ctypes
import types

import numpy as np
import pytest

import loadcases_cpu as lc
import stress_cpu as sc
import thermal_cpu as tc
import thermoelastic_cpu as te

FD_STEP = 1e-5
FD_BOUND = 1e-6
FD_MEASURED = {("plate2", "sum"): 3.3e-8, ("plate2", "pnorm"): 3.7e-8, ("block3", "sum"): 5.5e-9, ("block3", "pnorm"): 7.7e-9}
FD_STRIDE = {"plate2": 1, "block3": 3}
ADJOINT_SHARE = 1e-3


class _Voxels:
    """what ``couplingMatrix`` reads from a simulator, without a device"""

    P = 1

    def __init__(self, ne, h, tensor):
        self.N, self._ne = len(ne), np.asarray(ne)
        self._bbmin, self._bbmax = np.zeros(self.N), np.asarray(ne) * np.asarray(h, dtype=np.float64)
        self._mask = np.zeros((self.numNodes(), self.N), dtype=bool)
        self._dvals = np.zeros((self.numNodes(), self.N))
        self.ETensor = tensor

    def numElements(self):
        return int(np.prod(self._ne))

    _num_stored_elements = numElements

    def numNodes(self):
        return int(np.prod(self._ne + 1))

    def NbElementsPerDimension(self):
        return self._ne.copy()


@pytest.mark.parametrize("expansion", ["scalar", "tensor"])
@pytest.mark.parametrize("kind", ["isotropic", "orthotropic"])
@pytest.mark.parametrize("N", [2, 3])
def test_the_closed_form_of_the_coupling_matrix_is_the_quadrature(N, kind, expansion):
    from ndr_amd import ElasticityTensor, thermoelastic
    h = tc.EDGES[N]
    D = lc.hc.isotropic_D(1.3, 0.3, N) if kind == "isotropic" else lc.orthotropic_D(N)
    alpha = 0.7 if expansion == "scalar" else te.ALPHA_TENSOR[N]
    G = thermoelastic.couplingMatrix(_Voxels((3,) * N, h, ElasticityTensor.fromD(D, N)), alpha)
    want = te.coupling_matrix(D, h, alpha)
    Lt = lc.eigenstrain_pattern(D, h, te.expansion_tensor(alpha, N))
    err = np.abs(G - want).max() / np.abs(want).max()
    rows = np.abs(G.sum(axis=1) - Lt).max() / np.abs(Lt).max()
    print("coupling matrix %d-D %s %s: closed form against quadrature %.2e, row sums against Lt %.2e" % (N, kind, expansion, err, rows))
    assert G.shape == (N * 2 ** N, 2 ** N) and G.flags.c_contiguous
    assert err < 8 * 2.0 ** -52 and rows < 8 * 2.0 ** -52
    # the temperature is interpolated, not averaged: the columns differ
    assert np.abs(G - G.mean(axis=1, keepdims=True)).max() > 0.1 * np.abs(G).max()


@pytest.mark.parametrize("aggregate", ["sum", "pnorm"])
@pytest.mark.parametrize("name", ["plate2", "block3"])
def test_central_differences_of_the_aggregate(name, aggregate):
    p = te.problem(name)
    r = te.reference(name, aggregate)
    g = r["gradient"]
    J = lambda rho: te.evaluate(p, rho, aggregate, want_gradient=False)["J"]
    entries = np.arange(0, g.size, FD_STRIDE[name])
    fd = np.empty(entries.size)
    for j, e in enumerate(entries):
        d = np.zeros(g.size)
        d[e] = FD_STEP
        fd[j] = (J(p["rho"] + d) - J(p["rho"] - d)) / (2.0 * FD_STEP)
    err = float(np.abs(fd - g[entries]).max() / np.abs(g).max())
    share = float(np.linalg.norm(r["adjoint"]) / np.linalg.norm(g))
    print("central differences %s %s: %.2e of the largest entry (bounds %.0e and %.1e); %d positive and %d negative entries, the thermal "
          "adjoint term has %.2e of the norm; c = %s, a = %s" % (name, aggregate, err, FD_BOUND, 10 * FD_MEASURED[(name, aggregate)],
                                                               (g > 0).sum(), (g < 0).sum(), share, r["c"], r["a"]))
    assert err < FD_BOUND and err < 10.0 * FD_MEASURED[(name, aggregate)]
    # a missing term would not pass: both signs, and the adjoint term is no rounding of the rest
    assert (g > 0).sum() >= 10 and (g < 0).sum() >= 10 and share >= ADJOINT_SHARE
    assert np.linalg.norm(r["explicit"]) >= ADJOINT_SHARE * np.linalg.norm(g)
    assert np.allclose(g, r["a"] @ r["case_gradients"], rtol=1e-12, atol=1e-12 * np.abs(g).max())
    assert (r["c"] > 0).all() and (r["a"] > 0).all() and r["hot"] == [1]


@pytest.mark.parametrize("kind", ["isotropic", "orthotropic"])
@pytest.mark.parametrize("dim", ["2", "3"])
def test_a_uniform_field_is_the_constant_eigenstrain(dim, kind):
    ne, h = lc.FREE[dim]
    eu, ec, p, r, ef = te.free_expansion(ne, h, lc.free_tensor(dim, kind), 0.01)
    print("uniform field %s %s: load against the eigenstrain load %.2e, u %.2e (bound %.2e), c %.2e (bound %.2e)"
          % (dim, kind, ef, eu, 10 * lc.FREE_U_MEASURED[(dim, kind)], ec, lc.free_c_bound(dim, kind)))
    assert not r["T"].any()
    assert ef < 8 * 2.0 ** -52
    assert eu < 10.0 * lc.FREE_U_MEASURED[(dim, kind)] and ec < lc.free_c_bound(dim, kind)
    assert not r["u"][0][r["fixed"]].any()


def test_the_float64_floor_of_the_chain():
    """J, every c_i and the gradient once with LU solves and once with Cholesky solves: what two correct float64 evaluations of the
    same chain differ by.  The recorded figures the GPU bound is built from must be what this computes: not below it, and not more
    than twice it."""
    values, gradient = zip(*(te.chain_differences(name, aggregate, te.solve_cholesky) for name in ("plate2", "block3")
                             for aggregate in ("sum", "pnorm")))
    print("chain floor (Cholesky against LU): values %s, gradient %s (recorded %.1e, %.1e); the direct GPU bound is %.1e"
          % (" ".join("%.2e" % v for v in values), " ".join("%.2e" % v for v in gradient), te.FLOOR_VALUE_MEASURED,
             te.FLOOR_GRADIENT_MEASURED, te.direct_bound()))
    assert max(values) <= te.FLOOR_VALUE_MEASURED <= 2.0 * max(values)
    assert max(gradient) <= te.FLOOR_GRADIENT_MEASURED <= 2.0 * max(gradient)
    assert te.direct_bound() == max(1e-11, 10.0 * max(te.FLOOR_VALUE_MEASURED, te.FLOOR_GRADIENT_MEASURED))


def test_chain_with_conjugate_gradient_solves_matches_the_dense_chain():
    """what the PCG paths of the GPU tests may differ by: every solve, elastic and thermal (the adjoint too), by conjugate gradients
    to a relative residual of 1e-12 on block3even"""
    values, gradient = zip(*(te.chain_differences("block3even", aggregate, te.solve_cg) for aggregate in ("sum", "pnorm")))
    print("CG chain block3even: values %.2e / %.2e, gradient %.2e / %.2e (recorded %.1e, %.1e)"
          % (*values, *gradient, te.CG_VALUE_MEASURED, te.CG_GRADIENT_MEASURED))
    assert max(values) <= te.CG_VALUE_MEASURED <= 2.0 * max(values)
    assert max(gradient) <= te.CG_GRADIENT_MEASURED <= 2.0 * max(gradient)


def test_extended_precision_variants_agree_with_float64():
    """the longdouble forms the GPU tests use as their reference are the float64 forms to rounding, and the adjoint source is the
    transpose of the load"""
    ne = (4, 3, 5)
    rng = np.random.default_rng(12)
    nel, nn = 60, sc.num_nodes(ne)
    G = rng.standard_normal((2, 24, 8))
    E, dE, T = rng.uniform(0.1, 1, nel), rng.uniform(0.1, 1, nel), rng.standard_normal(nn)
    U, a, tref = rng.standard_normal((2, nn * 3)), rng.standard_normal(2), rng.standard_normal(2)
    for fn, args in ((te.kernel_load, (ne, G[0], tref[0], E, T, None, U[0])), (te.kernel_adjoint_source, (ne, a, G, E, U)),
                     (te.kernel_gradient, (ne, a, G, tref, dE, T, U, E))):
        v64, v80 = fn(*args), fn(*args, dtype=np.longdouble)
        assert v80.dtype == np.longdouble and np.abs(v80 - v64).max() < 1e-14 * np.abs(v64).max()
    lhs = T @ te.kernel_adjoint_source(ne, [1.0], G[:1], E, U[:1])
    rhs = U[0] @ te.kernel_load(ne, G[0], 0.0, E, T)
    assert abs(lhs - rhs) < 1e-13 * abs(rhs)


# ---- refusals that come before any device call (they run without a GPU) ----

def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _head(ne, h):
    n, hh = np.asarray(ne, dtype=np.int64), np.ascontiguousarray(h, dtype=np.float64)
    return (len(ne), n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _dp(hh)), (n, hh)


P = lambda a: ctypes.c_void_p(a)
nan = lambda a, i: (lambda b: (b.__setitem__(i, np.nan), b)[1])(a.copy())


def _grid_refusals(call, rest):
    """what every entry point says of a bad grid; ``rest``: the arguments after dim, nelems, h"""
    from ndr_amd import _lib
    err = lambda: _lib.load().vfem_last_error().decode()
    args, keep = _head((7, 5), (0.5, 0.3))
    assert call(4, *args[1:], *rest) == 1 and "dim" in err()
    assert call(2, None, args[2], *rest) == 1 and "null" in err()
    assert call(2, args[1], None, *rest) == 1 and "null" in err()
    bad, keep2 = _head((7, 0), (0.5, 0.3))
    assert call(*bad, *rest) == 1 and "extent" in err()
    for hbad in ((0.5, 0.0), (0.5, -1.0), (np.inf, 0.3)):
        bad, keep3 = _head((7, 5), hbad)
        assert call(*bad, *rest) == 1 and "edge lengths" in err()


def test_load_refuses_bad_arguments_before_any_device_call():
    """status 1 and a message; the device pointers are addresses nobody dereferences"""
    from ndr_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vfem_last_error().decode()
    args, keep = _head((7, 5), (0.5, 0.3))
    G = np.ones((8, 4))
    E, T, mask, fin, fout = P(0x100000), P(0x200000), P(0x300000), P(0x400000), P(0x500000)
    call = lambda *t: lib.vfem_thermoelastic_load(*t, None)
    full = lambda **kw: [kw.get(k, d) for k, d in (("G", _dp(G)), ("tref", 0.5), ("E", E), ("T", T), ("mask", mask), ("fin", fin), ("fout", fout))]
    for name in ("G", "E", "T", "fout"):
        assert call(*args, *full(**{name: None})) == 1 and "null" in err()
    _grid_refusals(call, full())
    for v in (np.nan, np.inf):
        Gbad = G.copy()
        Gbad[3, 1] = v
        assert call(*args, *full(G=_dp(Gbad))) == 1 and "coupling matrix is not finite" in err()
        assert call(*args, *full(tref=v)) == 1 and "reference temperature is not finite" in err()
    # overlaps: f_out is 48 nodes x 2 doubles = 768 bytes, T 48 doubles, E 35
    assert call(*args, *full(fin=P(0x500008))) == 1 and "overlaps f_in" in err()
    assert call(*args, *full(T=P(0x500000 - 47 * 8))) == 1 and "aliases the temperatures" in err()
    assert call(*args, *full(E=P(0x500000 + 760))) == 1 and "aliases the multipliers" in err()
    assert call(*args, *full(mask=P(0x500000 + 767))) == 1 and "aliases the mask" in err()


def test_adjoint_source_refuses_bad_arguments_before_any_device_call():
    from ndr_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vfem_last_error().decode()
    args, keep = _head((6, 4, 5), (0.5, 0.3, 0.7))
    a, G = np.ones(8), np.ones((8, 24, 8))
    E, U, fixed, q = P(0x100000), P(0x300000), P(0x700000), P(0x800000)
    call = lambda *t: lib.vfem_thermoelastic_adjoint_source(*t, None)
    full = lambda **kw: [kw.get(k, d) for k, d in (("n", 3), ("a", _dp(a)), ("G", _dp(G)), ("E", E), ("U", U), ("fixed", fixed), ("q", q))]
    for n in (0, 9, -1):
        assert call(*args, *full(n=n)) == 1 and "ncases must be 1 to 8" in err()
    for name in ("a", "G", "E", "U", "q"):
        assert call(*args, *full(**{name: None})) == 1 and "null" in err()
    _grid_refusals(lambda dim, ne, h, *rest: call(dim, ne, h, *rest), full())
    assert call(*args, *full(a=_dp(nan(a, 2)))) == 1 and "coefficients are not finite" in err()
    assert call(*args, *full(G=_dp(nan(G, (2, 5, 1))))) == 1 and "coupling matrices are not finite" in err()
    # overlaps: q is 7 x 5 x 6 = 210 doubles = 1680 bytes
    assert call(*args, *full(U=P(0x800000 - 3 * 210 * 3 * 8 + 8))) == 1 and "aliases the displacements" in err()
    assert call(*args, *full(E=P(0x800000 + 1672))) == 1 and "aliases the multipliers" in err()
    assert call(*args, *full(fixed=P(0x800000 - 209))) == 1 and "aliases the mask" in err()


def test_gradient_refuses_bad_arguments_before_any_device_call():
    from ndr_amd import _lib
    lib = _lib.load()
    err = lambda: lib.vfem_last_error().decode()
    args, keep = _head((6, 4, 5), (0.5, 0.3, 0.7))
    a, G = np.ones(8), np.ones((8, 24, 8))
    dE, T, U, gin, g = P(0x100000), P(0x200000), P(0x300000), P(0x700000), P(0x800000)
    call = lambda *t: lib.vfem_thermoelastic_gradient(*t, None)
    full = lambda **kw: [kw.get(k, d) for k, d in (("n", 3), ("a", _dp(a)), ("G", _dp(G)), ("tref", _dp(a)), ("dE", dE), ("T", T), ("U", U),
                                                    ("gin", gin), ("g", g))]
    for n in (0, 9, -1):
        assert call(*args, *full(n=n)) == 1 and "ncases must be 1 to 8" in err()
    for name in ("a", "G", "tref", "dE", "T", "U", "g"):
        assert call(*args, *full(**{name: None})) == 1 and "null" in err()
    _grid_refusals(call, full())
    assert call(*args, *full(a=_dp(nan(a, 2)))) == 1 and "coefficients are not finite" in err()
    assert call(*args, *full(G=_dp(nan(G, (0, 23, 7))))) == 1 and "coupling matrices are not finite" in err()
    assert call(*args, *full(tref=_dp(nan(a, 1)))) == 1 and "reference temperatures are not finite" in err()
    # overlaps: g is 120 doubles = 960 bytes
    assert call(*args, *full(gin=P(0x800008))) == 1 and "overlaps g_in" in err()
    assert call(*args, *full(dE=P(0x800000 + 952))) == 1 and "aliases an input" in err()
    assert call(*args, *full(T=P(0x800000 - 209 * 8))) == 1 and "aliases an input" in err()
    assert call(*args, *full(U=P(0x800000 - 3 * 210 * 3 * 8 + 8))) == 1 and "aliases an input" in err()


def _unsolved_thermal(N=2):
    """a ThermalComplianceObjective nobody built (its constructor needs a device): what TemperatureLoad reads of it at construction"""
    from ndr_amd import thermal
    t = object.__new__(thermal.ThermalComplianceObjective)
    t._sim = types.SimpleNamespace(N=N)
    return t


def test_temperature_load_and_load_case_refusals():
    from ndr_amd import loadcases, thermoelastic
    t = _unsolved_thermal()
    with pytest.raises(TypeError, match="ThermalComplianceObjective"):
        thermoelastic.TemperatureLoad(object(), 0.1)
    for bad in (np.nan, np.inf, [[1.0, 0.5], [0.0, 1.0]], np.eye(3), [[np.nan, 0.0], [0.0, 1.0]], [1.0, 2.0]):
        with pytest.raises(RuntimeError, match="expansion must be a finite scalar or a finite symmetric 2 x 2 matrix"):
            thermoelastic.TemperatureLoad(t, bad)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(RuntimeError, match="referenceTemperature must be finite"):
            thermoelastic.TemperatureLoad(t, 0.1, referenceTemperature=bad)
    load = thermoelastic.TemperatureLoad(t, 0.1, referenceTemperature=-2.0)
    assert np.array_equal(load.expansion, 0.1 * np.eye(2)) and load.referenceTemperature == -2.0 and load.thermal is t
    assert np.array_equal(thermoelastic.TemperatureLoad(_unsolved_thermal(3), te.ALPHA_TENSOR[3]).expansion, te.ALPHA_TENSOR[3])
    with pytest.raises(TypeError, match="TemperatureLoad"):
        loadcases.LoadCase(temperature=0.1)
    with pytest.raises(TypeError, match="TemperatureLoad"):
        loadcases.LoadCase(temperature=t)
    case = loadcases.LoadCase(loads=0, temperature=load)
    assert case.designDependent and case.temperature is load
    assert not loadcases.LoadCase().designDependent and loadcases.LoadCase().temperature is None
    # the grid and the box of the heat simulator are compared with the elastic simulator's
    ne, h = (4, 3), (0.5, 0.25)
    elastic = _Voxels(ne, h, None)
    t._sim = types.SimpleNamespace(N=2, NbElementsPerDimension=lambda: np.array(ne), _bbmin=np.zeros(2), _bbmax=np.array([2.0, 0.75]))
    load.check(elastic)
    t._sim.NbElementsPerDimension = lambda: np.array((4, 4))
    with pytest.raises(RuntimeError, match="grid .* is not the elastic simulator's"):
        load.check(elastic)
    t._sim.NbElementsPerDimension = lambda: np.array(ne)
    t._sim._bbmax = np.array([2.0, 0.8])
    with pytest.raises(RuntimeError, match="bounding box is not the elastic simulator's"):
        load.check(elastic)
    with pytest.raises(RuntimeError, match="expansion must be"):
        thermoelastic.couplingMatrix(_Voxels(ne, h, None), np.eye(3))
