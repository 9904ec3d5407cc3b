"""-m gpu: the five kernels of the block eigensolver (kernels_modal.hip) one at a time at every size its callers reach, and the
solver at the block sizes tests/test_gpu_modal.py does not run.  DESIGN 3.13 lists which instantiation and which launch split each
block size m = numModes + numGuard reaches; in short, a solve forms m x m and 3m x 3m Gram matrices (k_block_gram_partial<1> for
one column, <4> up to four, <8> beyond) and combines m -> m, 2m -> m, 3m -> 2m and 3m -> m columns in launches of 12 output columns.

Bounds.  None comes from the device code.
  Gram and combine: integers stored as doubles (entries -8 .. 8, coefficients -4 .. 4).  Every product and every partial sum is an
    integer below 2^53 (64 x 300 001 < 2^25; 24 x 32 = 768), so every multiply-add is exact whatever the order of the sum: the tests
    assert the bits of the integer product (numpy int64; for the 524 289-row combine a float64 BLAS product, exact for the same
    reason, itself held to the int64 product on the first and last 300 rows).
  Mass apply: TOL_KERNEL of tests/test_gpu_modal.py (1e-12 of the largest entry: an entry is a sum of at most 27 x 8 products).
  Gradient: |got_e - ref_e| <= 2 L 2^-53 S_e against modal_cpu.kernel_gradient (np.longdouble), S_e the sum of the absolute values
    of the products behind g_e and L = modal_cpu.kernel_gradient_chain(N, nmodes) = nmodes (ke^2 + ke + (N ke + ke) + 2 N + 3) + 2
    the roundings one product can pass through (counted there from the kernel): 105 / 311 / 826 for 1 / 3 / 8 modes in 2-D (ke = 8),
    707 / 2 117 / 5 642 in 3-D (ke = 24), so that the bound is 2.3e-14 .. 1.3e-12 of S_e.
  Projection: bits.
  eigenmodes at tol 1e-9: the rule of tests/test_gpu_modal.py.  The restatement's LOBPCG (tests/test_modal_cpu.py prints these:
    test_lobpcg_at_the_other_block_sizes) differs from scipy.linalg.eigh, relative to the largest eigenvalue asked for, by
        modes + guard      16 x 12: iterations, eigenvalues, X^T M X - I      8 x 8 x 6: the same
        1 + 0              7, 5.72e-13, 6.7e-16                               17, 3.23e-13, 1.1e-16
        1 + 2              6, 5.77e-13, 4.4e-16                               8, 3.18e-13, 1.1e-15
        2 + 2              9, 7.10e-14, 2.2e-16                               8, 2.42e-13, 1.4e-15
        8 + 0              22, 1.07e-14, 2.6e-15                              18, 2.20e-14, 1.1e-15
    The device's eigenvalue bound is ten times the figure and not below FLOOR = 1e-12, the iteration cap twice the count; ten times
    every orthonormality figure is below FLOOR, which is that bound.
  bucklingModes, one mode on column2 (m = 3): the restatement (test_buckling_lobpcg_with_one_mode) takes 9 iterations and differs
    from eigh by 9.13e-14 of |nu_1| and 7.9e-14 in phi^T K phi - 1: both bounds are FLOOR, the cap is 18.

Measured on an MI355X:
  Gram: 56 pairs at each of n = 1, 255, 256, 257, 262 145 and (24, 24) at 300 001, six outputs each: every bit that of the int64
    product.  Combine: 35 pairs at each of n = 1, 255, 257, 524 289, twice: the same, and NaN behind the last column.
  mass apply 8.0e-17 .. 5.6e-16 of the largest entry over the thirty cases; a second run and off-line buffers bit-identical.
  gradient: the largest |got - ref| / (2 L 2^-53 S_e) over the 48 cases is 0.0141 (40 x 37, elasticity K0, one mode); second run
    and off-line buffers bit-identical.  Projection: bits as expected in the four cases.
  eigenmodes, iterations (restatement) and eigenvalue difference; orthonormality at most 2.0e-15, every warm start 0 iterations:
        modes + guard      16 x 12, band factor      8 x 8 x 6, band factor      8 x 8 x 6, 2-level V-cycle
        1 + 0              8 (7), 9.0e-13            15 (17), 4.4e-14            21 (17), 4.5e-14
        1 + 2              6 (6), 9.2e-13            7 (8), 4.5e-14              14 (8), 4.5e-14
        2 + 2              9 (9), 1.5e-13            8 (8), 1.3e-13              14 (8), 6.5e-14
        8 + 0              22 (22), 3.7e-14          18 (18), 4.6e-14            23 (18), 4.0e-14
  bucklingModes column2, one mode: 9 iterations, nu 2.0e-13, phi^T K phi - 1 2.2e-16.
  The whole file runs in 7 s (1.5 s of it the 524 289-row combine with its 35 reference products).
  No defect found: every test passed on the library as it was.
  Mutations: MUTATIONS below.
"""
import functools

import numpy as np
import pytest
import torch

import buckling_cpu as bc
import homogenization_cpu as hc
import modal_cpu as mc
import stress_cpu as sc
import test_gpu_buckling as tgb
import test_gpu_modal as tgm
from test_gpu_modal import FLOOR, TOL_KERNEL, TOL_SOLVE, _dev, _dp, _head, _name, _p

pytestmark = pytest.mark.gpu

from ndr_amd import _lib, buckling, modal                      # noqa: E402
from ndr_amd import pyVoxelFEM as pv                           # noqa: E402

NAN = float("nan")

MUTATIONS = """
  Each built as a library of its own, one change that stays inside the arrays, and run on an MI355X against this file and
  tests/test_gpu_modal.py (40 tests, all passing on the shipped library).
  1. k_block_gram_partial<4> stores acc[q][p] for acc[p][q].  This file: 9 fail -- test_gram_of_integer_blocks_is_exact at n = 1,
     255, 256, 257, 262 145 (300 001 runs the widest pair only: <8>), test_gram_of_a_block_with_itself_and_with_its_upper_columns,
     and test_eigenmodes_at_the_other_block_sizes at 1 + 0 on all three paths.  The solves at m = 3 and 4 pass: their <4> matrices
     are the m x m ones, of which the iteration uses the diagonal and the start a matrix it symmetrises; at m = 1 the 3 x 3
     matrix S^T (M S) has its rows and columns in different orders and a transpose is a wrong matrix.  tests/test_gpu_modal.py: 40 pass.
  2. launch_block_combine reads C[r * kout + j] for C[r * kout + j0 + j].  This file: 7 fail -- test_combine_of_integer_blocks_is_exact
     at all four n (kout = 13, 14, 16, 24), test_eigenmodes_at_the_other_block_sizes at 8 + 0 on all three paths (3m -> 2m = 16
     columns).  tests/test_gpu_modal.py: test_combine_matches_numpy[24] fails too (two full launches); 39 pass.
  3. k_modal_gradient takes K0's rows of node mn from node mn ^ 1.  This file: all 16 test_gradient_kernel_matches_the_restatement
     cases fail.  tests/test_gpu_modal.py: the objective's five gradient tests fail (16 x 12 and 8 x 8 x 6, end to end); 35 pass.
  4. k_modal_mass_apply tests mask[node] for mask[node + off].  This file: the 15 masked test_mass_apply_matches_the_assembled_matrix
     cases fail.  tests/test_gpu_modal.py: its eight masked cases and test_public_mass_operator fail too; the solver tests pass (the
     blocks they apply M to are zero at the fixed components already).
  5. k_modal_project starts its component loop at 1.  This file: the four projection cases, every solve (13) and the buckling
     solve fail.  tests/test_gpu_modal.py: 12 fail (every solve and what is built on one).
  So 1 is seen by this file alone; 2 to 5 were already seen by the older file at some size, and are now seen kernel by kernel: the
  second launch of fewer than twelve columns, rows past 64 nodes, the gradient and the projection without a solve around them.
"""


def _bits(a):
    """the bit patterns of a float64 array or device tensor"""
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- Gram and combine on integers: exact ----

GRAM_BLOCKS_ROWS = 1024 * 256                                  # GRAM_BLOCKS workgroups of 256 threads: one row each
COMBINE_ROWS = 2048 * 256                                      # the combine's cap of 2048 workgroups
N_WIDEST = tgm.N_BLOCK                                         # 300 001, for the widest pair only
GRAM_WIDTHS = (1, 2, 3, 4, 5, 8, 9)
GRAM_PAIRS = sorted({(ka, kb) for ka in GRAM_WIDTHS for kb in GRAM_WIDTHS}
                    | {(m, m) for m in range(1, 9)} | {(3 * m, 3 * m) for m in range(1, 9)})           # the solver's: m and 3 m
GRAM_LENGTHS = [1, 255, 256, 257, GRAM_BLOCKS_ROWS + 1]
COMBINE_PAIRS = sorted({p for m in range(1, 9) for p in ((m, m), (2 * m, m), (3 * m, 2 * m), (3 * m, m))}
                       | {(24, 13), (1, 24), (24, 1)})          # (kin, kout); kout = 13, 14, 16: a second launch of 1, 2, 4 columns
COMBINE_LENGTHS = [1, 255, 257, COMBINE_ROWS + 1]


@functools.lru_cache(maxsize=None)
def _integers():
    """A [24, 524 289] and B [24, 300 001] of integers -8 .. 8, drawn once; a test takes leading rows and columns"""
    rng = np.random.default_rng(77)
    return (rng.integers(-8, 9, size=(24, COMBINE_ROWS + 1), dtype=np.int8), rng.integers(-8, 9, size=(24, N_WIDEST), dtype=np.int8))


def _gram_calls(n, ka, A, kb, B):
    """the Gram matrix four times: device output only, host output only, both, and both again"""
    lib = _lib.load()
    out = []
    for to_device, to_host in ((True, False), (False, True), (True, True), (True, True)):
        G = torch.full((ka, kb), NAN, dtype=torch.float64, device="cuda") if to_device else None
        host = np.full((ka, kb), np.nan) if to_host else None
        _lib.check(lib.vfem_block_gram(n, ka, _p(A), kb, _p(B), _p(G), _dp(host) if to_host else None, pv._stream()))
        if to_device:
            out.append(G.cpu().numpy())
        if to_host:
            out.append(host)
    return out


@pytest.mark.parametrize("n", GRAM_LENGTHS + [N_WIDEST])
def test_gram_of_integer_blocks_is_exact(n):
    assert 64 * n < 2 ** 53
    ia, ib = _integers()
    a, b = ia[:, :n].astype(np.int64), ib[:, :n].astype(np.int64)
    want = a @ b.T                                                                     # [24, 24], int64
    A, B = _dev(a.astype(np.float64)), _dev(b.astype(np.float64))
    wrong = []
    for ka, kb in (GRAM_PAIRS if n != N_WIDEST else [(24, 24)]):
        ref = _bits(want[:ka, :kb].astype(np.float64))
        got = _gram_calls(n, ka, A[:ka], kb, B[:kb])
        assert len(got) == 6
        if not all(np.array_equal(_bits(g), ref) for g in got):
            wrong.append((ka, kb, int(sum((_bits(g) != ref).sum() for g in got))))
    print("gram n = %d: %d pairs, wrong (ka, kb, entries over six outputs): %s" % (n, len(GRAM_PAIRS), wrong))
    assert not wrong


def test_gram_of_a_block_with_itself_and_with_its_upper_columns():
    """what the solver passes: the same pointer twice (S^T S is symmetric to the bit), and blocks that start inside a buffer"""
    n = 257
    a = _integers()[0][:, :n].astype(np.int64)
    A = _dev(a.astype(np.float64))
    for m in (1, 3, 4, 8):
        got = _gram_calls(n, m, A[m:2 * m], 3 * m, A[:3 * m])
        ref = _bits((a[m:2 * m] @ a[:3 * m].T).astype(np.float64))
        assert all(np.array_equal(_bits(g), ref) for g in got)
        sym = _gram_calls(n, 3 * m, A[:3 * m], 3 * m, A[:3 * m])[0]
        assert np.array_equal(sym, sym.T) and np.array_equal(sym, (a[:3 * m] @ a[:3 * m].T).astype(np.float64))


@pytest.mark.parametrize("n", COMBINE_LENGTHS)
def test_combine_of_integer_blocks_is_exact(n):
    ia = _integers()[0][:, :n]
    a = ia.astype(np.float64)
    A = _dev(a)
    edge = min(n, 300)
    ends = np.r_[0:edge, n - edge:n]
    ai = ia[:, ends].astype(np.int64)
    lib = _lib.load()
    wrong = []
    for kin, kout in COMBINE_PAIRS:
        ci = np.random.default_rng(1000 * kin + kout).integers(-4, 5, size=(kin, kout))
        C = np.ascontiguousarray(ci.astype(np.float64))
        want = C.T @ a[:kin]                                                           # exact: integers below 2^53 in any order
        assert np.array_equal(want[:, ends], (ci.T @ ai[:kin]).astype(np.float64))
        pad = n + 3
        out = []
        for _ in range(2):
            B = torch.full((kout * n + pad,), NAN, dtype=torch.float64, device="cuda")
            _lib.check(lib.vfem_block_combine(n, kin, kout, _p(A), _dp(C), _p(B), pv._stream()))
            torch.cuda.synchronize()
            assert bool(torch.isnan(B[kout * n:]).all()), (kin, kout, "wrote behind its last column")
            out.append(B[:kout * n].cpu().numpy().reshape(kout, n))
        if not (np.array_equal(_bits(out[0]), _bits(want)) and np.array_equal(_bits(out[1]), _bits(want))):
            wrong.append((kin, kout, sorted(set(np.nonzero(_bits(out[0]) != _bits(want))[0].tolist()))))
    print("combine n = %d: %d pairs, wrong (kin, kout, columns): %s" % (n, len(COMBINE_PAIRS), wrong))
    assert not wrong


# ---- the mass operator: rows past 64 and 128 nodes, one-element grids, up to 24 columns ----

MASS_SHAPES = [(5, 70), (3, 3, 70), (2, 130), (1, 1), (1, 1, 1)]


def _spread(a):
    """true where ``a`` or one of its neighbours (at most one step along every axis) is true"""
    out = a
    for ax in range(a.ndim):
        p = np.pad(out, [(1, 1) if i == ax else (0, 0) for i in range(a.ndim)])
        cut = lambda s: tuple(s if i == ax else slice(None) for i in range(a.ndim))          # noqa: E731
        out = p[cut(slice(0, -2))] | p[cut(slice(1, -1))] | p[cut(slice(2, None))]
    return out


def _fixed_neighbours_across_seams(ne, fixed):
    """per 64-lane seam along the last axis: (nodes below it with a free component and a fixed neighbour above it, the reverse)"""
    nn = [n + 1 for n in ne]
    some_fixed, some_free = fixed.any(1).reshape(nn), (~fixed).any(1).reshape(nn)
    return [(int((some_free[..., s - 1] & _spread(some_fixed[..., s])).sum()), int((some_free[..., s] & _spread(some_fixed[..., s - 1])).sum()))
            for s in range(64, nn[-1], 64)]


@functools.lru_cache(maxsize=None)
def _mass_case(ne):
    N = len(ne)
    rng = np.random.default_rng(700 + int(np.prod(ne)) + N)
    nn = sc.num_nodes(ne)
    m = rng.uniform(0.05, 1.0, size=int(np.prod(ne)))
    X = rng.standard_normal((24, nn * N))
    fixed = rng.uniform(size=(nn, N)) < 0.2
    grid = fixed.reshape([n + 1 for n in ne] + [N])
    for s in range(64, ne[-1] + 1, 64):                        # a fixed component on either side of every seam, its neighbours free
        grid[..., 0, s - 1:s + 1, :] = False
        grid[..., 1, s - 1:s + 1, :] = False
        grid[..., 0, s, 0] = True
        grid[..., 1, s - 1, N - 1] = True
    if nn == 2 ** N:                                           # one element: some components fixed, the last node free
        fixed[0, 0], fixed[1, N - 1], fixed[-1, :] = True, True, False
    bits = np.zeros(nn, dtype=np.uint8)
    for c in range(N):
        bits |= fixed[:, c].astype(np.uint8) << c
    h = tgm.EDGES[N]
    return dict(ne=ne, N=N, h=h, m=m, X=X, fixed=fixed, bits=bits, M=mc.assemble_mass(ne, h, m), MP=mc.assemble_mass(ne, h, m, fixed))


@pytest.mark.parametrize("ne", MASS_SHAPES, ids=_name)
def test_mass_masks_put_fixed_neighbours_across_every_seam(ne):
    """on the CPU, before any launch: the masked cases below do test the neighbour's mask across a block edge"""
    fixed = _mass_case(ne)["fixed"]
    seams = _fixed_neighbours_across_seams(ne, fixed)
    assert len(seams) == ne[-1] // 64 and all(lo > 0 and hi > 0 for lo, hi in seams)
    if not seams:                                              # one element: every node is every other node's neighbour
        assert fixed.any() and (~fixed).any(1).sum() > 1


@pytest.mark.parametrize("masked", [False, True], ids=["free", "masked"])
@pytest.mark.parametrize("ncols", [1, 6, 24])
@pytest.mark.parametrize("ne", MASS_SHAPES, ids=_name)
def test_mass_apply_matches_the_assembled_matrix(ne, ncols, masked):
    c = _mass_case(ne)
    if masked:
        assert all(lo > 0 and hi > 0 for lo, hi in _fixed_neighbours_across_seams(ne, c["fixed"]))
    Y = tgm._run_mass(c, ncols, masked)
    ref = ((c["MP"] if masked else c["M"]) @ c["X"][:ncols].T).T
    err = np.abs(Y.cpu().numpy() - ref).max() / np.abs(ref).max()
    print("mass apply %s, %d columns, %s: %.2e" % (_name(ne), ncols, "masked" if masked else "free", err))
    assert err < TOL_KERNEL
    if masked:
        assert not Y.cpu().numpy()[:, c["fixed"].reshape(-1)].any()
    assert torch.equal(tgm._run_mass(c, ncols, masked), Y)                             # run to run
    assert torch.equal(tgm._run_mass(c, ncols, masked, off=True), Y)                   # 8 bytes off a 16-byte line


# ---- the gradient kernel ----

GRADIENT_SHAPES = [(7, 5), (40, 37), (5, 70), (6, 4, 5), (12, 10, 9), (3, 3, 70), (1, 1), (1, 1, 1)]
GRADIENT_MODES = (1, 3, 8)


@functools.lru_cache(maxsize=None)
def _gradient_case(ne):
    N = len(ne)
    rng = np.random.default_rng(900 + int(np.prod(ne)) + N)
    nel, ke = int(np.prod(ne)), N * 2 ** N
    h = tgm.EDGES[N]
    sign = lambda v: v * np.where(np.arange(v.size) % 2 == 0, 1.0, -1.0)               # noqa: E731  (both signs whatever the draw)
    dE, dm = rng.standard_normal(nel), rng.standard_normal(nel)
    if nel == 1:
        dm = -np.sign(dE) * np.abs(dm)
    return dict(ne=ne, N=N, h=h, Phi=rng.standard_normal((8, sc.num_nodes(ne) * N)), dE=dE, dm=dm,
                cK=sign(rng.uniform(0.2, 2.0, size=8)), cM=-sign(rng.uniform(0.2, 2.0, size=8)),
                K0={"elastic": hc.element_constants(hc.isotropic_D(1.3, 0.3, N), h)[0], "random": rng.standard_normal((ke, ke))})


@functools.lru_cache(maxsize=None)
def _gradient_reference(ne, kind, nmodes):
    c = _gradient_case(ne)
    return mc.kernel_gradient(ne, c["h"], c["K0"][kind], c["dE"], c["dm"], c["Phi"][:nmodes], c["cK"][:nmodes], c["cM"][:nmodes])


def _run_gradient(c, kind, nmodes, off=False):
    args, keep = _head(c["ne"], c["h"])
    Phi, dE, dm = _dev(c["Phi"][:nmodes], off), _dev(c["dE"], off), _dev(c["dm"], off)
    g = _dev(np.full(c["dE"].shape, np.nan), off)
    K0, cK, cM = (np.ascontiguousarray(v, dtype=np.float64) for v in (c["K0"][kind], c["cK"][:nmodes], c["cM"][:nmodes]))
    _lib.check(_lib.load().vfem_modal_gradient(*args, nmodes, _dp(K0), _dp(cK), _dp(cM), _p(dE), _p(dm), _p(Phi), _p(g), pv._stream()))
    torch.cuda.synchronize()
    return g


@pytest.mark.parametrize("kind", ["elastic", "random"])
@pytest.mark.parametrize("ne", GRADIENT_SHAPES, ids=_name)
def test_gradient_kernel_matches_the_restatement(ne, kind):
    """L = nmodes (ke^2 + ke + (N ke + ke) + 2 N + 3) + 2 roundings (modal_cpu.kernel_gradient_chain); the bound is 2 L 2^-53 S_e.
    Largest |got - ref| / (2 L 2^-53 S_e) observed on an MI355X: 0.0141."""
    c = _gradient_case(ne)
    if kind == "random":
        assert not np.allclose(c["K0"][kind], c["K0"][kind].T)
    one = c["dE"].size == 1                                                            # one element: dE and dm of opposite sign
    for v in ((np.r_[c["dE"], c["dm"]],) if one else (c["dE"], c["dm"])) + (c["cK"][:2], c["cM"][:2]):
        assert (v > 0).any() and (v < 0).any()
    for nmodes in GRADIENT_MODES:
        ref, S = _gradient_reference(ne, kind, nmodes)
        bound = 2.0 * mc.kernel_gradient_chain(len(ne), nmodes) * 2.0 ** -53
        g = _run_gradient(c, kind, nmodes)
        ratio = float((np.abs(g.cpu().numpy().astype(np.longdouble) - ref) / (bound * S)).max())
        print("gradient kernel %s, K0 %s, %d modes: %.4f of the bound %.2e S_e" % (_name(ne), kind, nmodes, ratio, bound))
        assert ratio <= 1.0
        assert torch.equal(_run_gradient(c, kind, nmodes), g)                          # run to run
        assert torch.equal(_run_gradient(c, kind, nmodes, off=True), g)                # 8 bytes off a 16-byte line


# ---- the projection kernel ----

SENTINEL = 12345.678


@pytest.mark.parametrize("ncols", [1, 24])
@pytest.mark.parametrize("ne", [(40, 37), (12, 10, 9)], ids=_name)
def test_projection_zeroes_the_fixed_components_and_nothing_else(ne, ncols):
    N, nn = len(ne), sc.num_nodes(ne)
    assert nn > 256 and nn % 256
    rng = np.random.default_rng(1100 + nn + ncols)
    fixed = rng.uniform(size=(nn, N)) < 0.2
    assert all(fixed[:, a].any() and not fixed[:, a].all() for a in range(N))
    bits = np.zeros(nn, dtype=np.uint8)
    for a in range(N):
        bits |= fixed[:, a].astype(np.uint8) << a
    X = rng.standard_normal((ncols, nn, N))
    raw = X.view(np.uint64).reshape(-1)
    odd = rng.choice(raw.size, size=60, replace=False)
    raw[odd[:20]] = np.uint64(0x7FF8000000000000) | rng.integers(1, 2 ** 40, size=20).astype(np.uint64)          # NaN with a payload
    raw[odd[20:40]] = np.uint64(0xFFF8000000000000) | rng.integers(1, 2 ** 40, size=20).astype(np.uint64)
    raw[odd[40:]] = np.uint64(0x8000000000000000)                                                                 # -0.0
    free = ~np.broadcast_to(fixed, X.shape).reshape(-1)
    assert free[odd[:40]].any() and free[odd[40:]].any() and (~free[odd]).any()
    want = X.copy()
    want[:, fixed] = 0.0
    assert (_bits(want)[:, fixed] == 0).all()                                          # +0.0
    buf = torch.from_numpy(np.r_[SENTINEL, X.reshape(-1), SENTINEL]).cuda()
    before = _bits(buf).copy()
    assert np.array_equal(before[1:-1], _bits(X).reshape(-1))                          # the payloads survive the copy
    args, keep = _head(ne, tgm.EDGES[N])
    lib = _lib.load()
    view = buf[1:-1]
    assert lib.vfem_modal_project(*args, None, ncols, _p(view), pv._stream()) == 0     # no mask: nothing to do
    torch.cuda.synchronize()
    assert np.array_equal(_bits(buf), before)
    _lib.check(lib.vfem_modal_project(*args, _p(torch.from_numpy(bits).cuda()), ncols, _p(view), pv._stream()))
    torch.cuda.synchronize()
    after = _bits(buf)
    assert after[0] == before[0] and after[-1] == before[-1]
    assert np.array_equal(after[1:-1], _bits(want).reshape(-1))


# ---- the solver at m = 1, 3, 4 and 8 ----

# (iterations, eigenvalue difference from eigh) of the restatement's LOBPCG: tests/test_modal_cpu.py prints them
RESTATEMENT = {("16x12", 1, 0): (7, 5.72e-13), ("16x12", 1, None): (6, 5.77e-13), ("16x12", 2, None): (9, 7.10e-14), ("16x12", 8, 0): (22, 1.07e-14),
               ("8x8x6", 1, 0): (17, 3.23e-13), ("8x8x6", 1, None): (8, 3.18e-13), ("8x8x6", 2, None): (8, 2.42e-13), ("8x8x6", 8, 0): (18, 2.20e-14)}
SOLVER_BLOCKS = [(1, 0), (1, None), (2, None), (8, 0)]         # (numModes, numGuard): m = 1, 3, 4, 8


@functools.lru_cache(maxsize=None)
def _simulator(name):
    """one simulator per fixture for the whole file (the tests leave it unchanged): its band factor is formed once"""
    return tgm._simulator(name)


@pytest.mark.parametrize("modes,guard", SOLVER_BLOCKS, ids=["1+0", "1+2", "2+2", "8+0"])
@pytest.mark.parametrize("name,preconditioner", [("16x12", "auto"), ("8x8x6", "auto"), ("8x8x6", "multigrid")])
def test_eigenmodes_at_the_other_block_sizes(name, preconditioner, modes, guard):
    its, fig = RESTATEMENT[name, modes, guard]
    want = mc.reference(name)["spectrum"][:modes]
    sim = _simulator(name)
    T = sim.multigridSolver(1) if preconditioner == "multigrid" else "auto"
    kw = dict(tol=TOL_SOLVE, preconditioner=T, numGuard=guard)
    lam, Phi, info = modal.eigenmodes(sim, modes, **kw)
    assert lam.shape == (modes,) and (np.diff(lam) > 0).all() and Phi.shape == (modes, sim.numNodes(), sim.N)
    assert info["blockSize"] == modes + (2 if guard is None else guard) and info["X"].shape[0] == info["blockSize"]
    P = Phi.cpu().numpy().reshape(modes, -1).T
    M = tgm._mass_matrix(name)
    err = np.abs(lam - want).max() / want.max()
    orth = np.abs(P.T @ (M @ P) - np.eye(modes)).max()
    print("eigenmodes %s %s, %d modes, block of %d: %d iterations (restatement %d; P dropped %d times), eigenvalues %.2e (bound %.1e), "
          "orthonormality %.2e, residuals %.2e" % (name, preconditioner, modes, info["blockSize"], info["iterations"], its, info["droppedP"],
                                                   err, max(10 * fig, FLOOR), orth, info["residuals"].max()))
    assert err < max(10 * fig, FLOOR) and orth < FLOOR
    assert info["residuals"].shape == (modes,) and info["residuals"].max() <= TOL_SOLVE
    assert info["iterations"] <= 2 * its
    fixed = mc.case(name)[4].reshape(-1)
    assert not P[fixed].any()
    # the residuals the solver reports are those of what it returns
    KP = np.stack([sim.applyK(Phi[i]).reshape(-1) for i in range(modes)], 1)
    MP = M @ P
    res = np.linalg.norm(np.where(fixed[:, None], 0.0, KP - MP * lam), axis=0) / (lam * np.linalg.norm(MP, axis=0))
    assert res.max() <= 2.0 * TOL_SOLVE
    # a warm start from the converged block, and the same bits from the same start
    lam2, Phi2, info2 = modal.eigenmodes(sim, modes, X0=info["X"], **kw)
    print("  warm start: %d iterations" % info2["iterations"])
    assert info2["iterations"] <= 2 and np.abs(lam2 - lam).max() < FLOOR * lam.max()
    lam3, Phi3, info3 = modal.eigenmodes(sim, modes, **kw)
    assert np.array_equal(lam3, lam) and torch.equal(Phi3, Phi) and info3["iterations"] == info["iterations"]


def test_the_lowest_natural_frequency_with_default_arguments():
    """eigenmodes(sim, 1): a block of three columns, every m x m Gram matrix through k_block_gram_partial<4>"""
    sim = _simulator("16x12")
    lam, Phi, info = modal.eigenmodes(sim, 1)
    want = mc.reference("16x12")["spectrum"][0]
    assert info["blockSize"] == 3 and info["residuals"].max() <= 1e-8
    # some eigenvalue lies within |r|_{M^-1} / |x|_M of a Ritz value, and |r|_{M^-1} / |x|_M <= sqrt(cond M) |r| / |M x|.  The
    # element's mass matrix has eigenvalues 1 : 3 per axis and the multipliers lie in [0.2, 1]: cond M <= 9 x 5, so the default
    # tol = 1e-8 puts lambda within 6.8e-8 of an eigenvalue, and the next one (0.200 against 0.024) is far away
    assert abs(lam[0] - want) < 1e-7 * want


def test_buckling_modes_with_one_mode():
    """the shared driver at m = 3 with the other pair of operators: K_G phi = nu K phi"""
    ref = bc.reference("column2")
    op = ref["op"]
    sim, solved = tgb._solved("column2")
    lam, Phi, info = buckling.bucklingModes(sim, solved._u, 1, tol=TOL_SOLVE)
    p = Phi.cpu().numpy().reshape(-1)[op["free"]]
    err = abs(info["nu"][0] - ref["nu"][0]) / abs(ref["nu"][0])
    orth = abs(p @ (op["K"] @ p) - 1.0)
    print("bucklingModes column2, 1 mode: %d iterations (restatement 9), nu %.2e, phi^T K phi - 1 %.2e, residual %.2e"
          % (info["iterations"], err, orth, info["residuals"].max()))
    assert info["blockSize"] == 3 and lam.shape == (1,) and lam[0] == -1.0 / info["nu"][0]
    assert err < max(10 * 9.13e-14, FLOOR) and orth < max(10 * 7.93e-14, FLOOR)
    assert info["residuals"].max() <= TOL_SOLVE and info["iterations"] <= 2 * 9
    assert not Phi.cpu().numpy().reshape(-1)[op["fixed"]].any()
    lam2, Phi2, info2 = buckling.bucklingModes(sim, solved._u, 1, tol=TOL_SOLVE, X0=info["X"])
    assert info2["iterations"] <= 2 and abs(lam2[0] - lam[0]) < FLOOR * lam[0]
    lam3, Phi3, _ = buckling.bucklingModes(sim, solved._u, 1, tol=TOL_SOLVE)
    assert np.array_equal(lam3, lam) and torch.equal(Phi3, Phi)
