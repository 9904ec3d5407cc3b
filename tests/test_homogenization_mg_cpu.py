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


def test_what_the_multi_workgroup_cells_are_for():
    """tests/test_gpu_homogenization_blocks.py chose its cells (homogenization_mg_cpu.block_cell) as the smallest that take the device's
    kernels past one workgroup of 256 threads and its reductions past 256 and 512 partials; that is arithmetic on the sizes, pinned
    here together with the iteration counts that make the laminates a test of the frozen columns, and the singular block of the
    void cell"""
    wg, T = mg.workgroups, mg.THREADS
    nodes = lambda n: int(np.prod(n))
    dims = {name: mg.level_dims(mg.BLOCK_CELLS[name][0]) for name in mg.BLOCK_CELLS}
    assert dims["2d-blocks"] == [[72, 64], [36, 32], [18, 16], [9, 8]]
    assert dims["3d-blocks"] == [[28, 24, 28], [14, 12, 14], [7, 6, 7]]
    assert dims["2d-partials"] == [[320, 256], [160, 128], [80, 64], [40, 32], [20, 16], [10, 8], [5, 4]]
    assert dims["tensor-2d"] == [[520, 260], [260, 130], [130, 65]] and dims["tensor-3d"] == [[52] * 3, [26] * 3, [13] * 3]
    # 2d-blocks: 18 workgroups of nodes; stored levels with a ragged last workgroup; a stored sweep (a quarter of the nodes per colour)
    # in two workgroups; an odd coarsest level
    d = dims["2d-blocks"]
    assert nodes(d[0]) == 18 * T
    assert [nodes(n) for n in d[1:3]] == [1152, 288] and wg(1152) == 5 and wg(288) == 2 and 288 % T != 0
    assert nodes(d[1]) // 4 == 288 and wg(288) == 2
    assert any(n % 2 for n in d[-1])
    # 3d-blocks: level-0 sweep of 2352 threads per colour, a stored level of 2352 nodes, its sweep of 294 threads, the coarsest matrix
    # from the stored blocks of 294 nodes, a gemv with 882 rows
    d = dims["3d-blocks"]
    assert nodes(d[0]) // 8 == 2352 and nodes(d[1]) == 2352 and wg(2352) == 10 and 2352 % T != 0
    assert nodes(d[1]) // 8 == 294 and nodes(d[2]) == 294 and wg(294) == 2 and 3 * nodes(d[2]) == 882
    # 2d-partials: more than 256 partials per reduction needs more than 65 536 nodes; 320 = 256 + 64
    assert nodes(dims["2d-partials"][0]) > 65536 and wg(nodes(dims["2d-partials"][0])) == 320 > T
    # tensor cells: more than 512 workgroups of elements, fewer than 1024: the second pass of the grid-stride loop is ragged
    assert wg(nodes(dims["tensor-2d"][0])) == 529 and wg(nodes(dims["tensor-3d"][0])) == 550
    assert all(512 * T < nodes(dims[name][0]) < 2 * 512 * T for name in ("tensor-2d", "tensor-3d"))
    # every other cell of the two older device test files stays below all of this
    assert max(nodes(c[0]) for c in mg.CELLS.values()) < 65536 and 32 ** 3 < 65536

    # laminates: the restatement's block-Jacobi counts; between the first and the last real column lie at least 9 iterations, so a
    # frozen column is read back at least once (the host reads every 8 iterations)
    counts = {}
    for name in mg.LAMINATES:
        pr = mg.block_problem(name)
        counts[name] = hc.pcg_columns(pr["K"], pr["b"], pr["N"], TOL)[1]
        norms = np.linalg.norm(pr["b"], axis=1)
        noise = [q for q in range(len(norms)) if norms[q] < 1e-12 * norms.max()]
        real = [counts[name][q] for q in range(len(norms)) if q not in noise]
        print(name, counts[name], "noise columns", noise, norms)
        assert noise == ([] if name == "lam-2d" else [3])
        assert max(real) - min(real) >= 9
    assert counts == {"lam-2d": [59, 59, 76], "lam-3d": [57, 57, 57, 87, 86, 86]}
    lam3 = mg.block_problem("lam-3d")
    assert 0.0 < np.linalg.norm(lam3["b"][3]) < 1e-18                # rounding noise, not zero: the device must cope with either

    # uniform cells: no right-hand side beyond rounding
    for name in mg.UNIFORM_CELLS:
        assert np.abs(mg.block_problem(name)["b"]).max() < 1e-15

    # the void cell: nine nodes without stiffness, so the node blocks cannot all be inverted
    pr = mg.block_problem("void-2d")
    diag = pr["K"].diagonal().reshape(-1, 2)
    assert int(np.sum(np.all(diag == 0.0, axis=1))) == 9
    try:
        singular = not np.all(np.isfinite(hc.block_jacobi(pr["K"], 2)))
    except np.linalg.LinAlgError:
        singular = True
    assert singular
