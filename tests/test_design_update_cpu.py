"""The numpy references of tests/design_update_cpu.py (the yardstick of tests/test_gpu_design_update.py) against the oracle's
sparse smoothing matrix, its projection filter and its OC step expression, at small sizes; runs without a GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import design_update_cpu as du  # noqa: E402

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("grid", [(7, 5), (1, 9), (2, 11), (6, 4, 5), (2, 1, 9), (3, 2, 1), (1, 1, 1), (9, 7, 8)])
@pytest.mark.parametrize("radius", [0, 1, 2, 3, 5, 12])
def test_box_filter_matches_smoothing_matrix(grid, radius):
    from oracle.vfem_oracle import smoothing_matrix
    rng = np.random.default_rng(radius)
    n = int(np.prod(grid))
    x, g = rng.uniform(0, 1, n), rng.standard_normal(n)
    A = smoothing_matrix(grid, radius)
    tol = 64 * (2 * radius + 1) ** len(grid) * EPS
    assert np.abs(du.box_filter(x, grid, radius) - A @ x).max() <= tol * np.abs(x).max()
    assert np.abs(du.box_filter(g, grid, radius, True) - A.T @ g).max() <= tol * np.abs(g).max()
    if radius >= max(grid):
        assert np.allclose(du.box_filter(x, grid, radius), x.mean(), rtol=0, atol=tol)
        assert np.allclose(du.box_filter(g, grid, radius, True), g.sum() / n, rtol=0, atol=tol * np.abs(g).max())


@pytest.mark.parametrize("beta", [1.0, 4.0, 16.0, 40.0, 256.0])
def test_projection_matches_oracle(beta):
    from oracle.vfem_oracle import OracleProjectionFilter
    x = np.concatenate([np.linspace(-0.1, 1.1, 241), [0.0, 0.5, 1.0]])
    g = np.random.default_rng(1).standard_normal(x.size)
    f = OracleProjectionFilter(beta)
    assert np.array_equal(du.projection(x, beta), f.apply(x))
    assert np.array_equal(du.projection_backprop(g, x, beta), f.backprop(g, x))


def test_oc_candidate_matches_oracle_step_expression():
    """the oracle's OC step inlines its candidate; run its bisection on a toy problem whose filters are the identity and
    compare the step with the restatement at the multiplier it found"""
    from oracle import vfem_oracle as vo
    rng = np.random.default_rng(2)
    n = 500
    x0 = np.concatenate([[0.0, 1.0, 0.0, 1.0], rng.uniform(0, 1, n - 4)])
    dJ = -rng.uniform(0, 2, n)
    dJ[:3] = 0.0

    class P:
        def __init__(self):
            self.cached = [x0.copy()]

        def evaluate_objective_gradient(self):
            return dJ

        def evaluate_constraints_jacobian(self):
            return np.array([np.full(n, -1.0 / (0.4 * n))])

        def evaluate_oc_constraint(self, x):
            return vo.OracleVolumeConstraint(0.4).evaluate(x)

        def set_vars(self, x):
            self.cached = [x]

        evaluate_objective = evaluate_constraints = lambda self: np.zeros(1)

    p = P()
    _, _, lam = vo.OracleOC(p).step(m=0.2)
    assert np.array_equal(p.cached[0], du.oc_candidate(x0, dJ, np.full(n, -1.0 / (0.4 * n)), lam, 0.2))


def test_oc_candidate_edges():
    x0 = np.array([0.0, 1.0, 0.5, 0.5, 0.5, 0.03])
    dJ = np.array([-1.0, -1.0, 0.0, 1.0, -1e9, -1e-9])
    dc = np.full(6, -1.0)
    ref = du.oc_candidate(x0, dJ, dc, 1.0, 0.2)
    assert np.array_equal(ref[[0, 1, 2, 4, 5]], [0.0, 1.0, 0.5 - 0.2, 0.5 + 0.2, 0.03 * np.sqrt(1e-9)])
    assert np.isnan(ref[3])                                 # dJ / (dc lam) < 0: the reference's NaN
    nf = du.oc_candidate_nan_free(x0, dJ, dc, 1.0, 0.2)
    assert nf[3] == 0.5 - 0.2 and np.array_equal(np.delete(nf, 3), np.delete(ref, 3))


def test_mean_of_nothing_is_refused_before_any_device_work():
    """vfem_mean(n < 1) fails with a message instead of returning 0 (or the reference's NaN), also on a box without a GPU"""
    import ctypes
    from ndr_amd import _lib
    lib = _lib.load()
    m = ctypes.c_double(7.0)
    for n in (0, -1):
        with pytest.raises(RuntimeError, match="empty vector"):
            _lib.check(lib.vfem_mean(n, None, ctypes.byref(m), None))
    assert m.value == 7.0
