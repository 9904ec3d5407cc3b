"""LangelaarFilter, CPU side: the numpy restatement (tests/langelaar_cpu.py) against centred finite differences and hand
computations, and the library's C ABI for it."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import langelaar_cpu as lc  # noqa: E402


def _fd(x, dims, g, h=1e-6):
    f = lambda v: float(np.dot(g, lc.apply(v, dims)[0]))
    d = np.empty_like(x)
    for i in range(x.size):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        d[i] = (f(xp) - f(xm)) / (2 * h)
    return d


@pytest.mark.parametrize("dims", [(5, 4), (3, 4, 4), (3, 3, 5), (4, 5, 3)])
def test_restatement_gradient_matches_finite_differences(dims):
    """every entry matches d(g . apply(x))/dx, except layer 0, which carries the reference's extra factor
    dsmin_dx1(x, 1) (forward treats layer 0 as the identity; backprop still scales it)"""
    rng = np.random.default_rng(sum(dims))
    n = int(np.prod(dims))
    x = rng.uniform(0.05, 0.95, n)
    g = rng.standard_normal(n)
    grad = lc.backprop(g, x, dims).reshape(lc.grid3(dims))
    fd = _fd(x, dims, g).reshape(lc.grid3(dims))
    x3 = x.reshape(lc.grid3(dims))
    scale = np.abs(fd).max()
    assert np.abs(grad[..., 1:] - fd[..., 1:]).max() < 1e-7 * scale
    assert np.abs(grad[..., 0] - fd[..., 0] * lc.dsmin_dx1(x3[..., 0], 1.0)).max() < 1e-7 * scale


def _smin(a, b):
    return 0.5 * (a + b - math.sqrt((a - b) ** 2 + 1e-4) + math.sqrt(1e-4))


def _d1(a, b):
    return 0.5 * (1 - (a - b) / math.sqrt((a - b) ** 2 + 1e-4))


def _d2(a, b):
    return 0.5 * (1 + (a - b) / math.sqrt((a - b) ** 2 + 1e-4))


def test_hand_computed_2x2():
    """x[i][k] (k = layer): both top elements are supported by both bottom ones"""
    P, Q = 40.0, 38.42
    a, b, c, d = 1.0, 0.8, 0.5, 0.3          # x = [[a, b], [c, d]]
    S = a ** P + c ** P
    sm = S ** (1 / Q)
    out, smax = lc.apply(np.array([a, b, c, d]), (2, 2))
    assert np.allclose(out, [a, _smin(b, sm), c, _smin(d, sm)], rtol=0, atol=1e-15)
    assert np.allclose(smax, [1, sm, 1, sm], rtol=0, atol=1e-15)
    g = np.array([1.0, 2.0, 3.0, 4.0])
    w = (2.0 * _d2(b, sm) + 4.0 * _d2(d, sm)) * S ** (1 / Q - 1)
    lam_a = 1.0 + P * a ** (P - 1) / Q * w
    lam_c = 3.0 + P * c ** (P - 1) / Q * w
    expect = [lam_a * _d1(a, 1.0), 2.0 * _d1(b, sm), lam_c * _d1(c, 1.0), 4.0 * _d1(d, sm)]
    assert np.allclose(lc.backprop(g, np.array([a, b, c, d]), (2, 2)), expect, rtol=1e-14, atol=0)


def test_hand_computed_3x1x2():
    """x[i][0][k]: top element i is supported by bottom elements i-1 .. i+1 clipped to the grid"""
    P, Q = 40.0, 38.42
    bot, top = [0.9, 0.2, 0.6], [0.7, 0.95, 0.1]
    x = np.array([v for i in range(3) for v in (bot[i], top[i])])
    S = [bot[0] ** P + bot[1] ** P, bot[0] ** P + bot[1] ** P + bot[2] ** P, bot[1] ** P + bot[2] ** P]
    sm = [s ** (1 / Q) for s in S]
    out, smax = lc.apply(x, (3, 1, 2))
    expect = [v for i in range(3) for v in (bot[i], _smin(top[i], sm[i]))]
    assert np.allclose(out, expect, rtol=0, atol=1e-15)
    assert np.allclose(smax[1::2], sm, rtol=0, atol=1e-15) and np.all(smax[0::2] == 1.0)
    g = np.ones(6)
    w = [_d2(top[q], sm[q]) * S[q] ** (1 / Q - 1) for q in range(3)]
    above = [w[0] + w[1], w[0] + w[1] + w[2], w[1] + w[2]]
    grad = lc.backprop(g, x, (3, 1, 2))
    for i in range(3):
        assert abs(grad[2 * i] - (1 + P * bot[i] ** (P - 1) / Q * above[i]) * _d1(bot[i], 1.0)) < 1e-14
        assert abs(grad[2 * i + 1] - _d1(top[i], sm[i])) < 1e-15


def test_all_zero_support_contributes_the_limit():
    """a support of exact zeros gives S = 0: the adjoint stays finite (the reference gets 0 * inf = NaN there)"""
    x = np.zeros((4, 3, 5))
    x[0, 0, :2] = 0.9
    grad = lc.backprop(np.ones(x.size), x.reshape(-1), x.shape)
    assert np.all(np.isfinite(grad))


def test_library_exports_langelaar_entry_points():
    from ndr_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("vfem_langelaar_apply", "vfem_langelaar_backprop"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
