"""not gpu: pins tests/microstructure_cpu.py, the restatement the device's microstructure design is compared with
(tests/test_gpu_microstructure.py): its periodic filter is self-adjoint and mean-preserving, the analytic gradient of
J = - Cs : Eh matches a central difference and is nowhere positive, and the optimality-criteria loop on the standard cell lowers J at
every step.

Recorded on the CPU (the restatement's direct solve):
  central difference (step 1e-6, one random direction) against the analytic directional derivative: 16 x 12 bulk 5.4e-11, shear
    1.4e-10, 8 x 8 x 6 bulk 2.1e-10 relative; the bound 1e-7 leaves the O(step^2) truncation three orders of room.
  J over the OC steps, first -> last:  16 x 12 bulk  -0.3456403288 -> -0.3595904656 (12 steps),
    16 x 12 shear  -0.0455658509 -> -0.0530146521 (12 steps),  8 x 8 x 6 bulk  -0.9423126777 -> -0.9438163403 (6 steps).
"""
import functools

import numpy as np
import pytest

import microstructure_cpu as ms

FD_STEP, FD_BOUND = 1e-6, 1e-7
CASES = {"2d-bulk": ((16, 12), ms.BULK_2D, 12), "2d-shear": ((16, 12), ms.SHEAR_2D, 12), "3d-bulk": ((8, 8, 6), ms.BULK_3D, 6)}
RECORDED = {"2d-bulk": (-0.3456403288, -0.3595904656), "2d-shear": (-0.0455658509, -0.0530146521),
            "3d-bulk": (-0.9423126777, -0.9438163403)}


@functools.lru_cache(maxsize=None)
def _trajectory(name):
    ne, weights, steps = CASES[name]
    return ms.trajectory(ne, weights, steps)


@pytest.mark.parametrize("grid, r", [((4, 4), 2), ((4, 4), 3), ((5, 3, 7), 1), ((3, 5, 2), 2), ((16, 12), 1), ((8, 8, 6), 1)])
def test_periodic_filter_is_self_adjoint_and_mean_preserving(grid, r):
    rng = np.random.default_rng(3)
    x, y = rng.uniform(0.0, 1.0, int(np.prod(grid))), rng.uniform(0.0, 1.0, int(np.prod(grid)))
    Fx, Fy = ms.periodic_box_filter(x, grid, r), ms.periodic_box_filter(y, grid, r)
    assert abs(x @ Fy - y @ Fx) <= 1e-13 * abs(x @ Fy)
    assert abs(Fx.mean() - x.mean()) <= 1e-13 * x.mean()
    # translation invariant: the filter of a shifted design is the shifted filter
    shift = tuple(1 for _ in grid)
    shifted = ms.periodic_box_filter(np.roll(x.reshape(grid), shift, axis=tuple(range(len(grid)))).reshape(-1), grid, r)
    assert np.abs(shifted - np.roll(Fx.reshape(grid), shift, axis=tuple(range(len(grid)))).reshape(-1)).max() <= 1e-14
    # against the definition, element by element
    e = tuple(n // 2 for n in grid)
    total = 0.0
    for off in np.ndindex(*([2 * r + 1] * len(grid))):
        total += x.reshape(grid)[tuple((e[d] + off[d] - r) % grid[d] for d in range(len(grid)))]
    assert abs(Fx.reshape(grid)[e] - total / (2 * r + 1) ** len(grid)) <= 1e-14


def test_a_window_as_wide_as_the_cell_counts_every_offset():
    """4 x 4, r = 2: five offsets per axis on four elements, so the element two steps away is met twice (at -2 and at +2)"""
    x = np.zeros((4, 4))
    x[0, 0] = 1.0
    F = ms.periodic_box_filter(x.reshape(-1), (4, 4), 2).reshape(4, 4)
    per_axis = np.array([1.0, 1.0, 2.0, 1.0]) / 5.0
    assert np.abs(F - np.outer(per_axis, per_axis)).max() <= 1e-16


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_matches_a_central_difference_and_is_nowhere_positive(name):
    ne, weights, _ = CASES[name]
    ne, h, D = ms.standard_cell(ne)
    rng = np.random.default_rng(5)
    x = ms.standard_design(ne) * rng.uniform(0.9, 1.1, int(np.prod(ne)))
    d = rng.standard_normal(x.size)
    _, g = ms.filtered_objective(ne, h, D, x, weights)
    up = ms.filtered_objective(ne, h, D, x + FD_STEP * d, weights)[0]
    down = ms.filtered_objective(ne, h, D, x - FD_STEP * d, weights)[0]
    fd, analytic = (up - down) / (2.0 * FD_STEP), float(g @ d)
    print("%s: central difference %.10e, analytic %.10e, relative %.2e" % (name, fd, analytic, abs(fd - analytic) / abs(analytic)))
    assert abs(fd - analytic) <= FD_BOUND * abs(analytic)
    assert np.all(g <= 0.0)
    assert np.all(ms.objective(ne, h, D, ms.periodic_box_filter(x, ne, ms.RADIUS), weights)[1] <= 0.0)


@pytest.mark.parametrize("name", list(CASES))
def test_oc_loop_lowers_the_objective_at_every_step(name):
    ne, _, steps = CASES[name]
    J, x = _trajectory(name)
    print("%s: J = %s" % (name, " ".join("%.10f" % v for v in J)))
    assert len(J) == steps + 1
    assert np.all(np.diff(J) < 0.0)
    assert abs(ms.periodic_box_filter(x, ne, ms.RADIUS).mean() / ms.VOLUME_FRACTION - 1.0) <= ms.CTOL
    assert x.min() >= 0.0 and x.max() <= 1.0
    first, last = RECORDED[name]
    assert abs(J[0] - first) <= 5e-10 and abs(J[-1] - last) <= 5e-10
