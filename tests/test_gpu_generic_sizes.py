"""The 2-D and generic multigrid kernels of ndr_amd/csrc/generic.hip against the sparse-matrix oracle (oracle.generic_oracle.GenericSim /
GenericMG: assembled K, P^T K P, per-colour sparse rows), one operation at a time, on grids past the toy sizes of
tests/test_gpu_generic.py (24 x 12, 12 x 8 and 8 x 4 x 8, two coarsenings each), where
  - a transfer launch (kg_restrict, kg_prolong: 256 threads per block) has at most two blocks;
  - kg_coarsen_next<N,p> runs once per hierarchy and never on matrices it produced itself;
  - no coarse grid has a single element along an axis, no grid has odd element counts, every mask is a few rollers, no element is void.
Whole solves do not judge these kernels: a PCG solve reaches the right answer with a smoother that skips nodes or a transfer that drops
a weight, it only takes more iterations.

Every case of CASES carries the reason it is there; test_shapes_cover_every_case_claim (no GPU) recomputes the claims from the
launchers' arithmetic, restated here.  Densities are uniform(0.05, 1) with one element in eight void (E_min = 1e-4: the modulus
contrast of a late design), element edges are unequal (0.5 x 0.75 [x 0.625]), and each case runs under two Dirichlet masks: the
clamped face i0 == 0, and that face plus about 5 % of the nodes that lie on an element boundary of every level, each with a random
non-empty subset of its components fixed.  An oracle / HIP pair is built once per (case, mask) by a module-scoped fixture.

Tolerances are those tests/test_gpu_generic.py and tests/test_gpu_degree2_long_rows.py hold the same operations to against the same
oracle, relative to the largest entry of the reference.

Largest achieved error per operation over all pairs, measured on the MI355X (each is in the deltas file under generic_sizes[...]):
  K0 2.3e-16, transfers 2.4e-16, gradient 1.2e-15, the simulator's apply 4.9e-16
  apply and residual of a level 2.4e-14, sweeps 2.7e-14: both on B's level 4 -- the distance between the element-by-element Galerkin
    recursion and the oracle's assembled product grows about threefold per level in 2-D (B: 4e-16, 1.3e-15, 3.8e-15, 1.2e-14)
  cycles 5.3e-10 (B-clamped) and 1.4e-10 (E-clamped): the clamped long cantilevers, whose coarsest levels (17 x 1 and 9 x 1 elements
    held at one end) have condition numbers 1.5e5 and 2.3e5; every other multi-level pair 3.8e-15; the coarsest solve alone (C, F) 7.0e-14
  PCG iterate after 8 iterations 8.1e-10, converged 6.1e-10, residual histories 8.5e-10 and 1.9e-9; plain CG on 45 600 dofs 2.3e-15
Wall time of the whole file there: 14 s (102 tests, 4 s of them the two tests that need no GPU)."""
import re

import numpy as np
import pytest

from helpers import MATERIAL, ROOT, record_deltas, relerr

gpu = pytest.mark.gpu

TOL_K0 = TOL_TRANSFER = 1e-13
TOL_GRADIENT = 1e-12
TOL_APPLY = 1e-11             # apply, residual
TOL_SWEEP = 1e-10
TOL_CYCLE = 1e-9              # cycles, coarsest solve
TOL_PCG = 1e-7                # PCG iterate
TOL_HISTORY = 1e-6            # relative residual after every iteration, relative per entry

EDGE = (0.5, 0.75, 0.625)       # element edges
SEED = 11
PCG_RHS_SEED = 7
E_MIN = 1e-4
WAVES_PER_BLOCK = 4             # kg_apply, kg_gs_color: one wave per node, blk(256)
TRANSFER_BLOCK = 256            # kg_restrict: thread per coarse node; kg_prolong: thread per fine node
DENSE_COARSEST_MAX_DOFS = 40000         # vfem_internal.h

# id: (N, p, fine elements, coarsenings L, what only this case reaches)
CASES = {
    "A": (2, 1, (40, 264), 3, "10 865 fine nodes; levels 20x132, 10x66 and an odd coarsest 5x33; kg_coarsen_next<2,1> on its own output "
                              "twice; transfers of 43 / 11 / 3 blocks with ragged last blocks"),
    "B": (2, 1, (272, 16), 4, "long slow axis, four coarsenings down to 17 x 1: every coarsest node is a boundary node and each colour of "
                              "that axis holds one node"),
    "C": (2, 1, (37, 71), 0, "odd element counts, even node counts; one level: the level-0 sweep and the dense coarsest solve of the whole "
                             "operator (5 472 dofs)"),
    "D": (2, 2, (20, 132), 2, "degree-2 quadrilaterals at 41 x 265 nodes; nine colours with unequal counts; ke = 18: the second half of "
                              "the lane ownership is unused"),
    "E": (2, 2, (72, 8), 3, "degree 2 down to 9 x 1; kg_coarsen_next<2,2> on its own output"),
    "F": (2, 2, (9, 35), 0, "degree 2, odd element counts, one level"),
    "G": (3, 1, (8, 4, 72), 2, "the generic <1,1,1> instantiation (kg_gs_color<3,1>, kg_coarsen_next<3,1>); long fast axis; coarsest "
                               "2 x 1 x 18"),
}
MASKS = ("clamped", "random")
PAIRS = [(cid, mk) for cid in CASES for mk in MASKS]
PAIR_IDS = ["%s-%s" % pm for pm in PAIRS]
TOO_LARGE_COARSENED = (400, 200)        # <1,1>, one coarsening: 201 x 101 x 2 = 40 602 dofs on the coarsest level
TOO_LARGE_ONE_LEVEL = (149, 151)        # <1,1>, uncoarsenable: 150 x 152 x 2 = 45 600 dofs


# ---- the launchers' arithmetic, restated (generic.hip, gs_colors.h) ---------------------------------------------------------------
def level_elems(ne, l):
    assert all(n % 2 ** l == 0 for n in ne), (ne, l)
    return tuple(n // 2 ** l for n in ne)


def level_nodes(p, ne, l):
    return tuple(p * n + 1 for n in level_elems(ne, l))


def colour_counts(p, nn):
    """nodes of every colour of for_each_gs_color: per axis (nn - 1 - la) // inc + 1 with inc = 2p on an element boundary, p inside"""
    out = []
    for la in np.ndindex(*([p + 1] * len(nn))):
        cnt = 1
        for a, l in enumerate(la):
            inc = (2 if l in (0, p) else 1) * p
            cnt *= 0 if l > nn[a] - 1 else (nn[a] - 1 - l) // inc + 1
        out.append(cnt)
    return out


def blocks(n, per_block):
    return -(-n // per_block), n % per_block


def _launcher_literals():
    src = open(ROOT + "/ndr_amd/csrc/generic.hip").read()
    hdr = open(ROOT + "/ndr_amd/csrc/gs_colors.h").read()
    assert "const dim3 grd((unsigned) ((col.total + 3) / 4)), blk(256);" in src                    # kg_gs_color
    assert "const dim3 grd((unsigned) ((d.nnodes + 3) / 4)), blk(256);" in src                     # kg_apply
    assert "kg_restrict<<<dim3((unsigned) ((c.nnodes + 255) / 256)), dim3(256), 0, s>>>" in src
    assert "kg_prolong<<<dim3((unsigned) ((f.nnodes + 255) / 256)), dim3(256), 0, s>>>" in src
    assert "col.cnt[a] = la > nn[a] - 1 ? 0 : (nn[a] - 1 - la) / col.inc[a] + 1;" in hdr
    limit = re.findall(r"constexpr long long DENSE_COARSEST_MAX_DOFS = (\d+);", open(ROOT + "/ndr_amd/csrc/vfem_internal.h").read())
    assert limit == [str(DENSE_COARSEST_MAX_DOFS)], limit


def test_shapes_cover_every_case_claim():
    _launcher_literals()
    nodes = lambda cid, l: level_nodes(CASES[cid][1], CASES[cid][2], l)
    count = lambda cid, l: int(np.prod(nodes(cid, l)))
    # the level extents the table names
    assert count("A", 0) == 10865 and [level_elems(CASES["A"][2], l) for l in (1, 2, 3)] == [(20, 132), (10, 66), (5, 33)]
    assert level_elems(CASES["B"][2], 4) == (17, 1) and level_elems(CASES["E"][2], 3) == (9, 1)
    assert level_elems(CASES["G"][2], 2) == (2, 1, 18) and nodes("D", 0) == (41, 265)
    assert 2 * count("C", 0) == 5472
    # a colour whose node count is no multiple of the four waves of a block, and one whose count is: on level 0 and on coarse levels
    for levels in ((0,), (1, 2, 3, 4)):
        cnts = [c for cid, (N, p, ne, L, _) in CASES.items() for l in levels if l <= L for c in colour_counts(p, nodes(cid, l))]
        assert any(c % WAVES_PER_BLOCK for c in cnts) and any(c and c % WAVES_PER_BLOCK == 0 for c in cnts)
        assert any(c > WAVES_PER_BLOCK for c in cnts)
    assert all(blocks(count(cid, 0), WAVES_PER_BLOCK)[0] > 1 for cid in CASES)
    assert any(blocks(count(cid, 0), WAVES_PER_BLOCK)[1] for cid in CASES)             # kg_apply: a last block with idle waves
    # D: nine colours, their counts not all equal; ke = 18 leaves lanes 18..63 and the whole second half (lane + 64) without a dof
    d = colour_counts(2, nodes("D", 0))
    assert len(d) == 9 and len(set(d)) > 1 and 2 * 9 < 64
    # A: every level pair interpolates in more than one block with a ragged last one (43 / 11 / 3), and restricts so wherever the
    # coarse level exceeds a block (11 / 3; the coarsest, 6 x 34 nodes, is one ragged block)
    assert [blocks(count("A", l), TRANSFER_BLOCK)[0] for l in range(4)] == [43, 11, 3, 1]
    assert all(blocks(count("A", l), TRANSFER_BLOCK)[1] for l in range(4))
    # a coarse level with one element along an axis: both of its nodes there are boundary nodes, one per colour
    for cid in ("B", "E", "G"):
        N, p, ne, L, _ = CASES[cid]
        assert 1 in level_elems(ne, L), cid
        axis = level_elems(ne, L).index(1)
        per_axis = [(p * 1 + 1 - 1 - la) // ((2 if la in (0, p) else 1) * p) + 1 for la in range(p + 1)]
        assert per_axis == [1] * (p + 1) and nodes(cid, L)[axis] == p + 1
    # odd element counts (no coarsening possible: one level).  Degree 1 then has even node counts; degree 2 has 2 ne + 1 nodes, odd
    # on every grid, and what an odd ne changes is that its two boundary colours (local index 0 and 2) hold equally many nodes
    for cid in ("C", "F"):
        N, p, ne, L, _ = CASES[cid]
        assert L == 0 and all(n % 2 for n in ne)
    assert all(n % 2 == 0 for n in nodes("C", 0))
    for n in nodes("F", 0):
        assert (n - 1 - 0) // 4 + 1 == (n - 1 - 2) // 4 + 1
    for n in nodes("D", 0):
        assert (n - 1 - 0) // 4 + 1 == (n - 1 - 2) // 4 + 2
    # kg_coarsen_next builds the levels 2..L: at least twice per hierarchy, from matrices it stored itself from level 3 on
    for cid in ("A", "B", "E"):
        assert CASES[cid][3] - 1 >= 2
    # every coarsest level fits the dense solve; the two refused grids do not
    for cid, (N, p, ne, L, _) in CASES.items():
        assert N * count(cid, L) <= DENSE_COARSEST_MAX_DOFS
    assert 2 * int(np.prod(level_nodes(1, TOO_LARGE_COARSENED, 1))) == 40602 > DENSE_COARSEST_MAX_DOFS
    assert 2 * int(np.prod(level_nodes(1, TOO_LARGE_ONE_LEVEL, 0))) == 45600 > DENSE_COARSEST_MAX_DOFS
    assert any(n % 2 for n in TOO_LARGE_ONE_LEVEL)


# ---- the problems ---------------------------------------------------------------------------------------------------------------------
def domain(ne):
    return ([0.0] * len(ne), [n * e for n, e in zip(ne, EDGE)])


def densities(ne, seed=SEED):
    rng = np.random.default_rng(seed)
    n = int(np.prod(ne))
    rho = rng.uniform(0.05, 1.0, size=n)
    rho[rng.permutation(n)[:n // 8]] = 0.0
    return rho


def dirichlet_mask(N, p, ne, L, kind, seed=SEED):
    """clamped: every component on the face i0 == 0.  random: that face, and about 5 % of the nodes with an index divisible by
    p 2^L (on an element boundary of every level; any node when L = 0), each with a random non-empty subset of its components"""
    nn = tuple(p * n + 1 for n in ne)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in nn], indexing="ij"), -1).reshape(-1, N)
    mask = np.zeros((idx.shape[0], N), dtype=bool)
    mask[idx[:, 0] == 0] = True
    if kind == "random":
        rng = np.random.default_rng(seed + 1)
        cand = np.flatnonzero((idx % (p * 2 ** L) == 0).any(axis=1))
        picked = rng.choice(cand, size=max(1, round(0.05 * cand.size)), replace=False)
        subsets = rng.integers(1, 2 ** N, size=picked.size)
        for c in range(N):
            mask[picked, c] |= ((subsets >> c) & 1).astype(bool)
    return mask


def oracle_sim(N, p, ne, mask, rho):
    from ndr_amd import pyVoxelFEM as pv
    from oracle import generic_oracle as go
    young, poisson = pv._read_isotropic_material(MATERIAL)
    o = go.GenericSim(N, p, domain(ne), ne, young, poisson)
    o.Emin = E_MIN
    o.mask = mask.copy()
    o.rho = rho.copy()
    return o


def hip_sim(N, p, ne, mask, rho):
    from ndr_amd import pyVoxelFEM as pv
    if (N, p) == (3, 1):
        t = type("G111", (pv._GenericSimulator,), {"N": 3, "P": 1})(domain(ne), list(ne))       # generic kernels on the tuned path's case
    else:
        t = pv.TensorProductSimulator([p] * N, domain(ne), list(ne))
    t.readMaterial(MATERIAL)
    t.E_min = E_MIN
    t.dirichletMask = mask
    t.setElementDensities(rho)
    return t


def free_rhs(o, seed):
    f = np.random.default_rng(seed).standard_normal((o.num_nodes, o.N))
    f[o.mask] = 0.0
    return f


def partly_fixed_nodes(mask):
    return int((mask.any(axis=1) & ~mask.all(axis=1)).sum())


def test_masks_coarsen_on_every_level():
    """the oracle coarsens every mask without refusal, every level keeps fixed and free dofs, and under the random mask every level has
    a node with some but not all of its components fixed (the GPU test asserts that the HIP hierarchy holds the same masks)"""
    from oracle import generic_oracle as go
    for cid, mk in PAIRS:
        N, p, ne, L, _ = CASES[cid]
        mask = dirichlet_mask(N, p, ne, L, mk)
        om = go.GenericMG(oracle_sim(N, p, ne, mask, np.ones(int(np.prod(ne)))), L)
        for l in range(L + 1):
            m = om.sims[l].mask
            assert m.any() and not m.all(), (cid, mk, l)
            if mk == "random":
                assert partly_fixed_nodes(m) >= 1, (cid, l)


# ---- one oracle / HIP pair per (case, mask) ------------------------------------------------------------------------------------------
class Pair:
    def __init__(self, cid, mk):
        from oracle import generic_oracle as go
        self.cid, self.mk = cid, mk
        self.N, self.p, self.ne, self.L, _ = CASES[cid]
        self.name = "generic_sizes[%s-%s]" % (cid, mk)
        self.rho = densities(self.ne)
        self.mask = dirichlet_mask(self.N, self.p, self.ne, self.L, mk)
        self.o = oracle_sim(self.N, self.p, self.ne, self.mask, self.rho)
        self.om = go.GenericMG(self.o, self.L)
        self.om.update_element_stiffness()
        self.t = hip_sim(self.N, self.p, self.ne, self.mask, self.rho)
        self.mg = self.t.multigridSolver(self.L)
        self.mg.updateElementStiffnessMatrices()


@pytest.fixture(scope="module", params=PAIRS, ids=PAIR_IDS)
def pair(request):
    p = Pair(*request.param)
    yield p
    p.__dict__.clear()


class Deltas:
    """achieved errors of one test: printed and asserted one by one, written to the deltas file whatever the outcome"""

    def __init__(self, name):
        self.name, self.seen = name, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        record_deltas(self.name, self.seen)
        return False

    def check(self, key, got, ref, tol):
        got = got.cpu().numpy() if hasattr(got, "cpu") else got
        err = relerr(got, ref)
        self.seen[key] = err
        print("%s %s: %.3e (tolerance %.0e)" % (self.name, key, err, tol))
        assert err < tol, (self.name, key, err)


def _level_operators(d, p, l, rng):
    """apply, residual and both sweeps of level l against the oracle's assembled matrix of that level"""
    n = p.om.sims[l].num_nodes
    v, b = rng.standard_normal((n, p.N)), rng.standard_normal((n, p.N))
    what = "level %d" % l
    d.check(what + " apply", p.mg.applyK_device(l, v), p.om.apply_k(l, v), TOL_APPLY)
    d.check(what + " residual", p.mg.computeResidual_device(l, v, b), p.om.residual(l, v, b), TOL_APPLY)
    x0 = p.om.zero_dirichlet(l, v.copy())
    for fwd in (True, False):
        ref = x0.copy()
        p.om.smoothing(l, ref, b, fwd)
        assert relerr(ref, x0) > 1e-3                                  # (the sweep moves the iterate)
        d.check("%s sweep %s" % (what, "forward" if fwd else "backward"), p.mg.smoothing_device(l, x0, b, fwd), ref, TOL_SWEEP)


def _transfers(d, p, l, rng):
    import torch
    N, nf, nc = p.N, p.om.sims[l].num_nodes, p.om.sims[l + 1].num_nodes
    r, c, base = rng.standard_normal((nf, N)), rng.standard_normal((nc, N)), rng.standard_normal((nf, N))
    what = "%d -> %d" % (l, l + 1)
    d.check(what + " restriction", p.mg.restriction_device(l, r), p.om.restriction(l, r), TOL_TRANSFER)
    pc = p.om.interpolation(l, c)
    d.check(what + " interpolation", p.mg.interpolation_device(l, c), pc, TOL_TRANSFER)
    d.check(what + " interpolation accumulated", p.mg.interpolation_device(l, c, out=torch.as_tensor(base, device="cuda").clone()), base + pc,
            TOL_TRANSFER)


@gpu
def test_dirichlet_masks_match_oracle(pair):
    p = pair                    # (the oracle is reached through the pair only: a failed test's traceback then keeps no oracle alive)
    assert np.array_equal(p.t.dirichletMask, p.mask)
    for l in range(p.L + 1):
        got = p.mg.getSimulator(l).dirichletMask
        assert got.shape == (int(np.prod(level_nodes(p.p, p.ne, l))), p.N)
        assert np.array_equal(got, p.om.sims[l].mask), l
        assert got.any(), l
        if p.mk == "random":
            assert partly_fixed_nodes(got) >= 1, l


@gpu
def test_level0_operators_match_oracle(pair):
    """K0, the simulator's apply (kg_apply with E_e K0) and kg_gradient for a random displacement; the hierarchy's apply, residual
    and sweeps of level 0"""
    p = pair
    rng = np.random.default_rng(4)
    u = rng.standard_normal((p.o.num_nodes, p.N))
    with Deltas(p.name + ".level0") as d:
        d.check("K0", p.t.fullDensityElementStiffnessMatrix(), p.o.K0, TOL_K0)
        d.check("applyK", p.t.applyK_device(u), p.o.apply_k(u), TOL_APPLY)
        d.check("gradient", p.t.complianceGradient_device(u), p.o.compliance_gradient(u), TOL_GRADIENT)
        _level_operators(d, p, 0, rng)


@gpu
def test_coarse_levels_match_oracle(pair):
    """every level 1..L against the oracle's P^T K P (the Galerkin matrices of kg_coarsen_first / kg_coarsen_next and the coarsened
    masks are judged here) and the transfers of every level pair against the oracle's P; a one-level hierarchy has no level 1"""
    p = pair
    rng = np.random.default_rng(5)
    if p.L == 0:
        with pytest.raises(IndexError):
            p.mg.applyK_device(1, np.zeros((1, p.N)))
        return
    with Deltas(p.name + ".coarse") as d:
        for l in range(1, p.L + 1):
            _level_operators(d, p, l, rng)
        for l in range(p.L):
            _transfers(d, p, l, rng)


@gpu
def test_cycles_match_oracle(pair):
    """one V-cycle and one full-multigrid cycle from zero, with 1 and 2 sweeps, symmetric and forward-only Gauss-Seidel; on a
    one-level hierarchy the cycle is the coarsest solve alone"""
    p = pair
    f = free_rhs(p.o, 6)
    try:
        with Deltas(p.name + ".cycle") as d:
            for sym in (True, False):
                p.om.symmetric_gs = sym
                p.mg.setSymmetricGaussSeidel(sym)
                for nsm in (1, 2):
                    for fmg in (False, True):
                        xo = p.om.solve(np.zeros_like(f), f, 1, nsm, True, False, fmg).copy()
                        xg = p.mg.solve(np.zeros_like(f), f, 1, nsm, True, False, None, fmg)
                        assert np.abs(xo).max() > 0
                        d.check("%s, %d sweeps, %s" % ("full multigrid" if fmg else "V-cycle", nsm, "symmetric" if sym else "forward only"),
                                xg, xo, TOL_CYCLE)
                        if p.L == 0:
                            assert np.all(xg[p.mask] == 0.0)
    finally:
        p.om.symmetric_gs = True
        p.mg.setSymmetricGaussSeidel(True)


def _pcg_pair(p, f, max_iter, tol):
    """(oracle iterate, HIP iterate, HIP relative residual after every iteration): 1 cycle, 2 sweeps, symmetric"""
    xo = p.om.pcg(np.zeros_like(f), f, max_iter, tol, 1, 2, False)
    hist = []
    xg = p.mg.preconditionedConjugateGradient_device(np.zeros_like(f), f, max_iter, tol, None, 1, 2, False,
                                                     residual_cb=lambda it, rnorm: hist.append(rnorm / np.linalg.norm(f)))
    return xo, xg.cpu().numpy(), np.array(hist)


def _check_history(d, key, got, ref):
    ref = np.array(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float(np.abs(got / ref - 1.0).max())
    d.seen[key] = err
    print("%s %s: %.3e (tolerance %.0e)" % (d.name, key, err, TOL_HISTORY))
    assert err < TOL_HISTORY, (d.name, key, got, ref)


CONVERGED_PAIRS = (("A", "clamped"), ("E", "clamped"))       # ... also solved to CONVERGED_TOL, iteration counts compared
CONVERGED_TOL = 1e-8


@gpu
def test_pcg_matches_oracle(pair):
    """cut off at 8 iterations (tol 1e-12 never stops it): the iterate and the relative residual after every iteration.  On
    CONVERGED_PAIRS also to tol 1e-8 with equal iteration counts -- a fair equality only where rounding cannot move the count, which
    is asserted first, on the oracle's own numbers"""
    p = pair
    f = free_rhs(p.o, PCG_RHS_SEED)
    with Deltas(p.name + ".pcg") as d:
        xo, xg, hist = _pcg_pair(p, f, 8, 1e-12)
        if p.L == 0:
            # the preconditioner is the exact solve: both sides are below the tolerance after one or two iterations, and what their
            # residuals hold then is rounding, which no two summation orders share -- the iterate is compared, the history is not
            print("%s iterations: %d (oracle %d), residual %.3e (oracle %.3e)" % (p.name, p.mg.last_iterations, p.om.last_iters,
                                                                                   p.mg.last_relative_residual, p.om.last_relres))
            assert 1 <= p.om.last_iters <= 2 and 1 <= p.mg.last_iterations <= 2
            assert p.mg.last_relative_residual <= 1e-12 and len(hist) == p.mg.last_iterations
            d.check("iterate, exact preconditioner", xg, xo, TOL_PCG)
            return
        assert p.mg.last_iterations == 8 and p.om.last_iters == 8
        d.check("iterate after 8", xg, xo, TOL_PCG)
        _check_history(d, "residual history of 8", hist, p.om.relres_history)
        if (p.cid, p.mk) in CONVERGED_PAIRS:
            xo, xg, hist = _pcg_pair(p, f, 300, CONVERGED_TOL)
            ref = p.om.relres_history
            print("%s oracle: %d iterations, residual %.3e after, %.3e before" % (p.name, p.om.last_iters, ref[-1], ref[-2]))
            assert p.om.last_iters < 300 and ref[-1] <= 0.97 * CONVERGED_TOL and ref[-2] >= 1.03 * CONVERGED_TOL, ref[-2:]
            assert p.mg.last_iterations == p.om.last_iters
            d.check("iterate converged", xg, xo, TOL_PCG)
            _check_history(d, "residual history converged", hist, ref)


@gpu
def test_design_change_reaches_every_level(pair):
    """after new densities the apply on level L matches an oracle rebuilt with them, and differs from the old one"""
    from oracle import generic_oracle as go
    p = pair
    rho2 = densities(p.ne, SEED + 100)
    v = np.random.default_rng(8).standard_normal((p.om.sims[p.L].num_nodes, p.N))
    old = p.om.apply_k(p.L, v)
    om2 = go.GenericMG(oracle_sim(p.N, p.p, p.ne, p.mask, rho2), p.L)
    om2.update_element_stiffness()
    new = om2.apply_k(p.L, v)
    assert relerr(new, old) > 1e3 * TOL_APPLY
    try:
        with Deltas(p.name + ".design") as d:
            d.check("level %d apply before" % p.L, p.mg.applyK_device(p.L, v), old, TOL_APPLY)
            p.t.setElementDensities(rho2)
            p.mg.updateElementStiffnessMatrices()
            d.check("level %d apply after" % p.L, p.mg.applyK_device(p.L, v), new, TOL_APPLY)
    finally:
        p.t.setElementDensities(p.rho)
        p.mg.updateElementStiffnessMatrices()


def _dev(a, off=False):
    """a device copy; off: a contiguous view that starts 8 bytes off a 16-byte line"""
    import torch
    a = np.ascontiguousarray(a)
    if not off:
        return torch.from_numpy(a).cuda()
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    view = buf[1:].reshape(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    return view


@gpu
def test_repeatable_and_alignment_independent(pair):
    """a second run gives the same bits (fixed lane ownership, fixed reduction tree), and so do inputs that start 8 bytes off a
    16-byte line: apply, residual and both sweeps on the levels 0 and 1, the transfers between them, one cycle (a one-level hierarchy
    has level 0 and the coarsest solve)"""
    from ndr_amd import _lib
    from ndr_amd.pyVoxelFEM import _ptr, _stream
    p = pair
    rng = np.random.default_rng(9)
    levels = (0, 1) if p.L else (0,)
    vec = {l: (rng.standard_normal((p.om.sims[l].num_nodes, p.N)), rng.standard_normal((p.om.sims[l].num_nodes, p.N))) for l in levels}
    f = free_rhs(p.o, 10)

    def sweep(l, u, b, fwd):             # in place on the caller's buffer (smoothing_device relaxes an aligned copy)
        _lib.check(p.mg._mg("smooth")(p.mg._h, l, _ptr(u), _ptr(b), int(fwd), _stream()))
        return u

    def run(off):
        out = {}
        for l in levels:
            u, b = vec[l]
            out["apply %d" % l] = p.mg.applyK_device(l, _dev(u, off))
            out["residual %d" % l] = p.mg.computeResidual_device(l, _dev(u, off), _dev(b, off))
            for fwd in (True, False):
                out["sweep %d %d" % (l, fwd)] = sweep(l, _dev(u, off), _dev(b, off), fwd)
        if p.L:
            out["restriction"] = p.mg.restriction_device(0, _dev(vec[0][0], off))
            out["interpolation"] = p.mg.interpolation_device(0, _dev(vec[1][0], off))
            out["interpolation accumulated"] = p.mg.interpolation_device(0, _dev(vec[1][0], off), out=_dev(vec[0][1], off))
        out["V-cycle"] = p.mg.solve_device(_dev(np.zeros_like(f), off), _dev(f, off), 1, 2, True, False, None, False)
        return {k: v.cpu().numpy() for k, v in out.items()}

    first = run(False)
    assert not np.array_equal(first["sweep 0 1"], vec[0][0]) and np.abs(first["V-cycle"]).max() > 0
    for what, other in (("second run", run(False)), ("8 bytes off", run(True))):
        for k in first:
            assert np.array_equal(first[k], other[k]), (what, k)


# ---- the two branches of gmg_update above the dense limit ----------------------------------------------------------------------------
@gpu
def test_coarsened_hierarchy_with_too_large_coarsest_level_is_refused():
    ne = TOO_LARGE_COARSENED
    t = hip_sim(2, 1, ne, dirichlet_mask(2, 1, ne, 1, "clamped"), densities(ne))
    mg = t.multigridSolver(1)
    with pytest.raises(RuntimeError, match=r"coarsest grid too large.*\(40602 dofs\); use more coarsening levels"):
        mg.updateElementStiffnessMatrices()
    f = np.zeros((t.numNodes(), 2))
    with pytest.raises(RuntimeError, match="coarse operators not built"):
        mg.solve(f, f, 1, 2, True, False, None, False)


@gpu
def test_one_level_hierarchy_above_the_dense_limit_keeps_plain_cg():
    """uncoarsenable and too large for the dense solve: the update succeeds, the unpreconditioned CG (mgSmoothingIterations = 0)
    matches the oracle's iterate after 20 iterations, any cycle throws"""
    from oracle import generic_oracle as go
    ne = TOO_LARGE_ONE_LEVEL
    mask, rho = dirichlet_mask(2, 1, ne, 0, "clamped"), densities(ne)
    o, t = oracle_sim(2, 1, ne, mask, rho), hip_sim(2, 1, ne, mask, rho)
    assert 2 * o.num_nodes == 45600
    om, mg = go.GenericMG(o, 0), t.multigridSolver(0)
    mg.updateElementStiffnessMatrices()
    f = free_rhs(o, 12)
    xo = om.pcg(np.zeros_like(f), f, 20, 1e-12, 1, 0, False)
    xg = mg.preconditionedConjugateGradient(np.zeros_like(f), f, 20, 1e-12, None, 1, 0, False)
    assert mg.last_iterations == 20 and om.last_iters == 20
    with Deltas("generic_sizes[one level, 45600 dofs]") as d:
        d.check("plain CG, 20 iterations", xg, xo, TOL_PCG)
    for updated in (True, False):
        with pytest.raises(RuntimeError, match="coarsest grid too large for the dense coarsest-level solve; use more coarsening levels"):
            mg.solve(np.zeros_like(f), f, 1, 2, updated, False, None, False)
