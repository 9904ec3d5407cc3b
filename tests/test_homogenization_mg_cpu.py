"""The scipy restatement of the multigrid-preconditioned PCG (tests/homogenization_mg_cpu.py) against itself and the direct solve: the
device tests compare with it, so what it claims is checked here, without a GPU.

Iteration counts at tol = 1e-10, one sweep, spherical / disc void of radius 0.3, isotropic E = 1, nu = 0.3, gamma = 1, E_min = 1e-3
(``python tests/homogenization_mg_cpu.py 16 16 16`` prints them):
    16^3   multigrid 12 .. 15   block Jacobi 62 .. 66
    32^2   13 .. 16 (82 .. 103)     64^2   16 .. 19 (166 .. 204)     128^2   17 .. 20 (333 .. 411)
The test cells (random densities in [0.05, 1], gamma = 3, anisotropic tensors, non-cubic voxels), multigrid PCG against SuperLU,
relative to the largest entry:
    12x8x16   20 .. 21 iterations   w 4.20e-10   Eh 9.76e-13      (block Jacobi 205 .. 210)
    16x12     30 .. 31              w 4.15e-10   Eh 1.75e-11      (194 .. 195)
    8x4x12    17 .. 18              w 2.98e-10   Eh 4.12e-12      (131 .. 133)
V-cycle symmetry u . M v = v . M u: at most 4.9e-14 relative on these cells."""
import functools

import numpy as np
import pytest

import homogenization_cpu as hc
import homogenization_mg_cpu as mg

TOL = 1e-10
# |x_pcg - x| <= tol cond(K) |x| at worst; what the block-Jacobi restatement is held to in the device tests is its own measured
# difference, and the same rule is used here: the measured figures above, times ten
BOUND_W = {"12x8x16": 10 * 4.20e-10, "16x12": 10 * 4.15e-10, "8x4x12": 10 * 2.98e-10}
BOUND_EH = {"12x8x16": 10 * 9.76e-13, "16x12": 10 * 1.75e-11, "8x4x12": 10 * 4.12e-12}


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@functools.lru_cache(maxsize=None)
def _cell(name):
    ref = mg.cell_reference(name)
    return ref, mg.Hierarchy(mg.CELLS[name][0], ref["K0"], ref["E"])


def test_levels():
    assert mg.level_dims((12, 8, 16)) == [[12, 8, 16], [6, 4, 8], [3, 2, 4]]
    assert mg.level_dims((16, 12)) == [[16, 12], [8, 6], [4, 3]]
    assert mg.level_dims((8, 4, 12)) == [[8, 4, 12], [4, 2, 6]]
    assert mg.level_dims((5, 3, 7)) == [[5, 3, 7]]
    assert mg.level_dims((128, 128))[-1] == [2, 2] and len(mg.level_dims((128, 128))) == 7
    assert mg.level_dims((8, 4, 12), levels=0) == [[8, 4, 12]]
    assert mg.level_dims((100, 100, 100)) == [[100] * 3, [50] * 3, [25] * 3]


def test_prolongation_reproduces_constants_and_level_0_is_the_assembled_matrix():
    ref, h = _cell("12x8x16")
    assert _relmax(h.K[0].toarray(), ref["K"].toarray()) < 1e-15
    for l, n in enumerate(h.dims[:-1]):
        P = mg.prolongation(n, 3)
        assert np.abs(P @ np.ones(P.shape[1]) - 1.0).max() < 1e-15          # rows sum to 1 per component
        # a rigid translation is in the kernel of every unpinned level operator
        assert np.abs(h.A[l + 1] @ np.tile([1.0, -2.0, 0.5], P.shape[1] // 3)).max() < 1e-12 * np.abs(h.A[l + 1]).max()


@pytest.mark.parametrize("name", ["12x8x16", "16x12", "8x4x12"])
@pytest.mark.parametrize("smoothing", [1, 2])
def test_vcycle_is_symmetric(name, smoothing):
    ref, h = _cell(name)
    N = len(mg.CELLS[name][0])
    rng = np.random.default_rng(3)
    u, v = rng.standard_normal((2, ref["K"].shape[0]))
    u[:N] = v[:N] = 0.0
    Mu, Mv = h.vcycle(u.copy(), smoothing), h.vcycle(v.copy(), smoothing)
    err = abs(u @ Mv - v @ Mu) / max(abs(u @ Mv), abs(v @ Mu))
    print("symmetry %s, %d sweeps: %.2e" % (name, smoothing, err))
    assert err < 1e-12
    assert u @ Mu > 0.0 and v @ Mv > 0.0


@pytest.mark.parametrize("name", ["12x8x16", "16x12", "8x4x12"])
def test_multigrid_pcg_meets_the_direct_solve(name):
    ref, h = _cell(name)
    ne = mg.CELLS[name][0]
    W, its = mg.pcg_columns(h, ref["b"], TOL)
    Eh = hc.tensor(ne, W, ref["L"], mg.cell_D(name), ref["vol"], ref["E"])
    err_w, err_e = _relmax(W, ref["W"]), _relmax(Eh, ref["Eh"])
    print("%s: iterations %s, w %.2e, Eh %.2e" % (name, its, err_w, err_e))
    assert err_w < BOUND_W[name] and err_e < BOUND_EH[name]


def test_one_level_hierarchy_is_the_exact_inverse():
    ref, h = _cell("5x3x7")
    assert h.dims == [[5, 3, 7]]
    W, its = mg.pcg_columns(h, ref["b"], TOL)
    assert its == [1] * 6
    assert _relmax(W, ref["W"]) < 1e-12


@functools.lru_cache(maxsize=None)
def _void(ne):
    return mg.void_iterations(ne, TOL)[0]


@pytest.mark.parametrize("ne,lo,hi", [((16, 16, 16), 12, 15), ((32, 32), 13, 16), ((64, 64), 16, 19), ((128, 128), 17, 20)])
def test_iteration_counts_of_the_void_cell(ne, lo, hi):
    its = _void(ne)
    print(ne, its)
    assert min(its) == lo and max(its) == hi


def test_grid_independence():
    assert max(_void((128, 128))) <= max(_void((32, 32))) + 5
