"""-m gpu: the one-term (vfem_thermal_*) and the two-term (vfem_transient_*) form of the scalar heat operator share their kernels
(DESIGN 3.18), so with mb = 0 the two-term entry points must give what the one-term ones give, bit for bit.

The capacity fma of every sum adds cap[e] * 0 = +0 to the value the conduction fma left: an exact zero, whatever the finite positive
cap.  So the bound is equality (torch.equal; a -0 against a +0 compares equal), not a tolerance: apply at 1 and 8 columns, the
diagonal, the band, the Jacobi-PCG (count and x), and for a hierarchy of each form every level's operator, one sweep forward and one
backward per level, one V-cycle and the multigrid-PCG (count and x).

Shapes: the last axis of (9, 70) and (2, 5, 66) crosses the 64-lane block edge of cell_threads.h and the second-to-last the 4-row
edge; (5, 3) and (3, 2, 2) are a single block.  The hierarchies, (8, 4) and (4, 4, 8), have two levels.

Every entry point used here exists at the parent commit, where the two forms had kernels of their own: the whole file passes there
too (run on an MI355X against the parent's library: 22 passed, as here), and in 2 s.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from ndr_amd import _lib                                                            # noqa: E402
from ndr_amd import pyVoxelFEM as pv                                                # noqa: E402
from ndr_amd.thermal import conductivityMatrix                                      # noqa: E402

SHAPES = [(5, 3), (9, 70), (3, 2, 2), (2, 5, 66)]
MG_SHAPES = [(8, 4), (4, 4, 8)]
K_ANISO = np.array([[1.4, 0.3, -0.2], [0.3, 0.8, 0.1], [-0.2, 0.1, 1.1]])
EDGES = np.array([0.5, 0.25, 0.4])
TILE = 64


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _name(ne):
    return "x".join(map(str, ne))


@functools.lru_cache(maxsize=None)
def _case(ne):
    """random kappa and cap in [0.1, 1], random X, about one node in seven fixed, the anisotropic Kc0, mb = 0"""
    N = len(ne)
    rng = np.random.default_rng(3100 + int(np.prod(ne)))
    n = np.asarray(ne, dtype=np.int64)
    nn, nel = int(np.prod(n + 1)), int(np.prod(n))
    fixed = rng.uniform(size=nn) < 1.0 / 7.0
    fixed[0] = True                                     # a sink in every case
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    c = dict(ne=ne, N=N, n=n, nn=nn, Kc0=np.ascontiguousarray(conductivityMatrix(K_ANISO[:N, :N], EDGES[:N])), mb=np.zeros(N + 1),
             kappa=dev(rng.uniform(0.1, 1.0, size=nel)), cap=dev(rng.uniform(0.1, 1.0, size=nel)), fixed=dev(fixed.astype(np.uint8)),
             X=dev(rng.standard_normal((8, nn))), B=dev(rng.standard_normal(nn)))
    c["head"] = (N, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    c["one"] = c["head"] + (_dp(c["Kc0"]), _p(c["kappa"]), _p(c["fixed"]))
    c["two"] = c["head"] + (_dp(c["Kc0"]), _dp(c["mb"]), _p(c["kappa"]), _p(c["cap"]), _p(c["fixed"]))
    return c


def _out(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")


def _same(what, ne, one, two):
    torch.cuda.synchronize()
    assert bool(torch.isfinite(one).all())
    same = torch.equal(one, two)
    print("%s %s: %d values, %s" % (what, _name(ne), one.numel(), "bit-identical" if same else
                                    "largest difference %.3e" % float((one - two).abs().max())))
    assert same


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
@pytest.mark.parametrize("ncols", [1, 8])
def test_apply(ne, ncols):
    c, lib = _case(ne), _lib.load()
    X, one, two = c["X"][:ncols].contiguous(), _out(ncols, c["nn"]), _out(ncols, c["nn"])
    _lib.check(lib.vfem_thermal_apply(*c["one"], ncols, _p(X), _p(one), pv._stream()))
    _lib.check(lib.vfem_transient_apply(*c["two"], 1, ncols, _p(X), None, _p(two), pv._stream()))
    _same("apply, %d columns" % ncols, ne, one, two)


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_diagonal(ne):
    c, lib = _case(ne), _lib.load()
    one, two = _out(c["nn"]), _out(c["nn"])
    _lib.check(lib.vfem_thermal_diagonal(*c["one"], _p(one), pv._stream()))
    _lib.check(lib.vfem_transient_diagonal(*c["two"], _p(two), pv._stream()))
    _same("diagonal", ne, one, two)


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_band_assemble(ne):
    c, lib = _case(ne), _lib.load()
    n, w = 1, 0
    for a in range(c["N"] - 1, -1, -1):
        w += n
        n *= int(ne[a]) + 1
    doubles = (n + TILE - 1) // TILE * ((w + TILE - 1) // TILE + 2) * TILE * TILE
    one, two = (torch.zeros(doubles, dtype=torch.float64, device="cuda") for _ in range(2))
    _lib.check(lib.vfem_thermal_band_assemble(*c["one"], _p(one), pv._stream()))
    _lib.check(lib.vfem_transient_band_assemble(*c["two"], _p(two), pv._stream()))
    _same("band", ne, one, two)


def _pcg(call, args, b, *more):
    x = torch.zeros_like(b)
    it, rel = ctypes.c_int(0), ctypes.c_double(0.0)
    _lib.check(call(*args, _p(b), _p(x), 1e-10, 500, *more, ctypes.byref(it), ctypes.byref(rel), pv._stream()))
    return x, it.value


@pytest.mark.parametrize("ne", SHAPES, ids=_name)
def test_pcg(ne):
    c, lib = _case(ne), _lib.load()
    one, it_one = _pcg(lib.vfem_thermal_pcg, c["one"], c["B"])
    two, it_two = _pcg(lib.vfem_transient_pcg, c["two"], c["B"])
    print("pcg %s: %d and %d iterations" % (_name(ne), it_one, it_two))
    assert it_one == it_two and it_one >= 1
    _same("pcg", ne, one, two)


@pytest.mark.parametrize("ne", MG_SHAPES, ids=_name)
def test_hierarchy(ne):
    c, lib = _case(ne), _lib.load()
    h1, h2 = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        _lib.check(lib.vfem_thermal_mg_create(ctypes.byref(h1), *c["one"], -1, pv._stream()))
        _lib.check(lib.vfem_transient_mg_create(ctypes.byref(h2), *c["two"], -1, pv._stream()))
        levels = lib.vfem_thermal_mg_num_levels(h1)
        assert levels == lib.vfem_thermal_mg_num_levels(h2) == 2
        rng = np.random.default_rng(3200 + int(np.prod(ne)))
        for l in range(levels):
            dims = np.zeros(c["N"], dtype=np.int64)
            _lib.check(lib.vfem_thermal_mg_level_dims(h1, l, dims.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
            nn = int(np.prod(dims + 1))
            X, B = (torch.from_numpy(rng.standard_normal(nn)).cuda() for _ in range(2))
            one, two = _out(nn), _out(nn)
            _lib.check(lib.vfem_thermal_mg_level_apply(h1, l, _p(X), _p(one), pv._stream()))
            _lib.check(lib.vfem_thermal_mg_level_apply(h2, l, _p(X), _p(two), pv._stream()))
            _same("level %d apply" % l, ne, one, two)
            for forward in (1, 0):
                one, two = X.clone(), X.clone()
                _lib.check(lib.vfem_thermal_mg_smooth(h1, l, _p(one), _p(B), forward, pv._stream()))
                _lib.check(lib.vfem_thermal_mg_smooth(h2, l, _p(two), _p(B), forward, pv._stream()))
                _same("level %d sweep %s" % (l, "forward" if forward else "backward"), ne, one, two)
        one, two = _out(c["nn"]), _out(c["nn"])
        _lib.check(lib.vfem_thermal_mg_vcycle(h1, _p(c["B"]), _p(one), 1, pv._stream()))
        _lib.check(lib.vfem_thermal_mg_vcycle(h2, _p(c["B"]), _p(two), 1, pv._stream()))
        _same("V-cycle", ne, one, two)
        one, it_one = _pcg(lib.vfem_thermal_mg_pcg, (h1,), c["B"], 1)
        two, it_two = _pcg(lib.vfem_thermal_mg_pcg, (h2,), c["B"], 1)
        print("multigrid-pcg %s: %d and %d iterations" % (_name(ne), it_one, it_two))
        assert it_one == it_two and it_one >= 1
        _same("multigrid-pcg", ne, one, two)
    finally:
        torch.cuda.synchronize()
        for h in (h1, h2):
            if h:
                lib.vfem_thermal_mg_destroy(h)
