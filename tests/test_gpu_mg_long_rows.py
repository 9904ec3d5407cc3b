"""-m gpu: the multigrid sweeps that only long z-rows reach, against the element-loop oracle (oracle.vfem_oracle.OracleMG).

The trilinear multigrid picks its Gauss-Seidel kernel from the level's shape.  The grids of tests/test_gpu_parity.py are too short
in z for three of the kernels the production solves run:
  - level 1, k_l1_pair_rows (VFEM_OPT_L1_MERGED = 2): whole 64-node segments of a row, nseg = (cntz - ka) / 64 >= 1, i.e. a fine
    ne_z >= 256; the nodes it leaves over go to k_l1_merged with a `walked` offset (kernels_l1_merged.hip, launch_l1_merged_sweep);
  - level 0, k_gs_rows_mf0_pair with more than one segment per colour (nA >= 2, level-0 NZ >= 129), where its A(s+1)-before-B(s)
    order matters (kernels_mg.hip);
  - stored stencils above WAVE_SWEEP_MAX_NODES (k_gs_color_stencil_split, the one-lane k_gs_color_stencil) and the half stencil
    (VFEM_OPT_L1_STORED = 2).
Every parametrisation recomputes the launchers' segment arithmetic and asserts the case it claims, so that a change of shape cannot
drop the coverage silently (test_shapes_cover_every_branch checks that the claims together reach every branch).  A boundary
condition that masks rows partway along z (write_cut_bc) is used beside the cantilever's whole-plane one."""
import os
import resource
import time

import numpy as np
import pytest
import torch

from helpers import (BC_CANTILEVER, l0_pair_segments, l1_pair_segments, level_nodes, make_hip, make_oracle, record_deltas, relerr,
                     seeded_density, write_cut_bc)

pytestmark = pytest.mark.gpu

TOL_SWEEP, TOL_OP = 1e-10, 1e-11
DOM = ([0, 0, 0], [2, 1, 1])

# option keys of include/vfem.h
GS_PAIR, GS_RESIDENT, STENCIL_SPLIT, GS_MARCH, L1_STORED, L1_MERGED = 10, 13, 18, 19, 21, 22
WAVE_SWEEP_MAX_NODES = 40000           # ndr_amd/csrc/vfem_internal.h


# the launchers' arithmetic, restated: helpers.l0_pair_segments, helpers.l1_pair_segments

# (shape, claims): claims["l0"] = forward / backward (nA, nB) of level 0, claims["l1"] = forward / backward (nseg, A left, B left) of
# level 1; each with two coarsening levels
SHAPES = [
    ((8, 4, 128), {"l0": ((2, 1), (1, 2)), "l1": ((0, 33, 32), (0, 32, 33))}),
    ((4, 8, 132), {"l0": ((2, 2), (2, 2)), "l1": ((0, 34, 33), (0, 33, 34))}),
    ((8, 4, 256), {"l0": ((3, 2), (2, 3)), "l1": ((1, 1, 0), (1, 0, 1))}),
    ((4, 8, 260), {"l0": ((3, 3), (3, 3)), "l1": ((1, 2, 1), (1, 1, 2))}),
    ((4, 4, 512), {"l0": ((5, 4), (4, 5)), "l1": ((2, 1, 0), (2, 0, 1))}),
]
SHAPE_IDS = ["x".join(map(str, s)) for s, _ in SHAPES]


def check_claims(ne, claims):
    NZ0, NZ1 = level_nodes(ne, 0)[2], level_nodes(ne, 1)[2]
    assert tuple(l0_pair_segments(NZ0, f) for f in (True, False)) == claims["l0"], ne
    assert tuple(l1_pair_segments(NZ1, f) for f in (True, False)) == claims["l1"], ne


def test_shapes_cover_every_branch():
    for ne, claims in SHAPES:
        check_claims(ne, claims)
    fwd0 = [c["l0"][0] for _, c in SHAPES]
    for nA in (2, 3):
        assert (nA, nA) in fwd0 and (nA, nA - 1) in fwd0, nA                         # lag-1 order, both tails
    assert any(a[0] >= 3 and b[0] >= 3 for a, b in (c["l0"] for _, c in SHAPES))      # several segments in both directions
    l1 = [s for _, c in SHAPES for s in c["l1"] if s[0] >= 1]
    assert {1, 2} <= {s[0] for s in l1}
    assert {True, False} == {s[1] > 0 for s in l1} == {s[2] > 0 for s in l1}
    for fi in (0, 1):                                                                 # both colour-first parities reach the pair branch
        assert any(c["l1"][fi][0] >= 1 for _, c in SHAPES)


# ---- a boundary condition that cuts z-rows (helpers.write_cut_bc) ------------------------------------------------------------------
@pytest.fixture(scope="module")
def cut_bc(tmp_path_factory):
    return write_cut_bc(tmp_path_factory.mktemp("bc") / "cut_rows.bc")


def _bc(name, cut_bc):
    return cut_bc if name == "cut" else BC_CANTILEVER


def _mg_pair(ne, bc, levels, nthreads=4):
    from oracle import vfem_oracle as vo
    rho = seeded_density(ne, 88)
    o, t = make_oracle(ne, DOM, bc, rho), make_hip(ne, DOM, bc, rho)
    omg = vo.OracleMG(o, levels, nthreads=nthreads)
    omg.update_element_stiffness()
    tmg = t.multigridSolver(levels)
    tmg.updateElementStiffnessMatrices()
    return o, t, omg, tmg


def _opt(t, key, value):
    from ndr_amd import _lib
    _lib.check(t._lib.vfem_sim_set_option(t._h, key, value))


def _partly_masked_row(mask, nn):
    rows = np.asarray(mask).reshape(nn + (3,)).any(axis=-1)
    return bool((rows.any(axis=2) & ~rows.all(axis=2)).any())


def _sweep_chain(omg, tmg, l, u0, b, first_forward, what, nsweeps=3):
    """nsweeps alternating sweeps, compared after each: an ordering fault that stays inside the tolerance after one sweep grows"""
    uo = u0.copy()
    ug = torch.as_tensor(u0, device="cuda")
    bg = torch.as_tensor(b, device="cuda")
    fwd = first_forward
    for step in range(nsweeps):
        omg.smoothing(l, uo, b, fwd)
        ug = tmg.smoothing_device(l, ug, bg, fwd)
        err = relerr(ug.cpu().numpy(), uo)
        assert err < TOL_SWEEP, (what, l, step, fwd, err)
        fwd = not fwd


def _start(omg, l, rng):
    n = omg.sims[l].num_nodes
    u = rng.standard_normal((n, 3))
    omg.enforce_dirichlet(l, u, True)
    return u, rng.standard_normal((n, 3))


@pytest.mark.parametrize("ne,claims", SHAPES, ids=SHAPE_IDS)
def test_cut_bc_masks_match_oracle(ne, claims, cut_bc):
    check_claims(ne, claims)
    o, t, omg, tmg = _mg_pair(ne, cut_bc, 2)
    for l in range(3):
        got = tmg.getSimulator(l).dirichletMask
        assert np.array_equal(got, omg.sims[l].dmask.astype(bool)), l
        if l < 2:
            assert _partly_masked_row(got, level_nodes(ne, l)), l
        else:
            assert np.asarray(got).any()


@pytest.mark.parametrize("bc", ["cut", "cantilever"])
@pytest.mark.parametrize("ne,claims", SHAPES, ids=SHAPE_IDS)
def test_level0_row_sweeps_match_oracle(ne, claims, bc, cut_bc):
    """the row kernels (VFEM_OPT_GS_MARCH = 0): fused z-colour pairs and one launch per colour, with K0 resident and from the table"""
    check_claims(ne, claims)
    o, t, omg, tmg = _mg_pair(ne, _bc(bc, cut_bc), 2)
    rng = np.random.default_rng(17)
    u0, b = _start(omg, 0, rng)
    wild = rng.standard_normal(u0.shape)                # constrained components carry values the sweep must leave alone
    mask = o.dmask != 0
    assert mask.any()
    _opt(t, GS_MARCH, 0)
    for pair in (1, 0):
        for res in (1, 0):
            _opt(t, GS_PAIR, pair)
            _opt(t, GS_RESIDENT, res)
            for first in (True, False):
                _sweep_chain(omg, tmg, 0, u0, b, first, ("pair", pair, "resident", res))
                got = tmg.smoothing_device(0, wild, b, first).cpu().numpy()
                assert np.array_equal(got[mask], wild[mask]), (pair, res, first)
                assert not np.array_equal(got[~mask], wild[~mask])


# level-1 implementations: (VFEM_OPT_L1_STORED, VFEM_OPT_L1_MERGED, VFEM_OPT_STENCIL_SPLIT)
L1_CONFIGS = [
    (0, 0, 1),      # node rows summed per incident element
    (0, 1, 1),      # per mirror class, one launch per colour (k_l1_merged)
    (0, 2, 1),      # per mirror class, z-colour pairs (k_l1_pair_rows + k_l1_merged for the nodes left over)
    (1, 2, 1),      # stored 27-point stencil, no node-major copy: k_gs_color_stencil_split at any size
    (1, 2, 0),      # the same, one lane per node (k_gs_color_stencil)
    (2, 2, 1),      # stored half stencil (k_gs_color_stencil_half)
]


@pytest.mark.parametrize("bc", ["cut", "cantilever"])
@pytest.mark.parametrize("ne,claims", SHAPES, ids=SHAPE_IDS)
def test_level1_sweeps_apply_residual_match_oracle(ne, claims, bc, cut_bc):
    check_claims(ne, claims)
    o, t, omg, tmg = _mg_pair(ne, _bc(bc, cut_bc), 2)
    rng = np.random.default_rng(29)
    u0, b = _start(omg, 1, rng)
    ua = rng.standard_normal(u0.shape)
    ref_apply, ref_res = omg.apply_k(1, ua), omg.residual(1, ua.copy(), b)
    for stored, merged, split in L1_CONFIGS:
        what = ("stored", stored, "merged", merged, "split", split)
        _opt(t, L1_STORED, stored)
        _opt(t, L1_MERGED, merged)
        _opt(t, STENCIL_SPLIT, split)
        tmg.updateElementStiffnessMatrices()
        assert relerr(tmg.applyK(1, ua), ref_apply) < TOL_OP, what
        assert relerr(tmg.computeResidual(1, ua, b), ref_res) < TOL_OP, what
        for first in (True, False):
            _sweep_chain(omg, tmg, 1, u0, b, first, what)


def test_pcg_with_pair_kernels_on_both_levels_matches_oracle(cut_bc):
    """a whole solve through the default level-1 pair kernel and the level-0 row pairs, iterate by iterate"""
    ne = (4, 8, 260)
    o, t, omg, tmg = _mg_pair(ne, cut_bc, 2)
    _opt(t, GS_MARCH, 0)
    _pcg_iterates(o, omg, tmg, 100, 1e-6)


def _pcg_iterates(o, omg, tmg, max_iter, tol):
    f = o.build_load_vector()
    seen_o, seen_g = [], []
    uo = omg.pcg(np.zeros_like(f), f, max_iter, tol, 1, 1, False, callback=lambda i, x, r: seen_o.append((i, x.copy(), r.copy())))
    ug = tmg.preconditionedConjugateGradient(np.zeros_like(f), f, max_iter, tol, lambda i, x, r: seen_g.append((i, x.copy(), r.copy())),
                                             1, 1, False)
    assert tmg.last_iterations == omg.last_iters == len(seen_o) == len(seen_g) > 0
    un, rn = np.abs(uo).max(), np.abs(f).max()
    for (io, xo, ro), (ig, xg, rg) in zip(seen_o, seen_g):
        assert io == ig
        assert np.abs(xg.reshape(xo.shape) - xo).max() < 1e-7 * un, (io, "x")
        assert np.abs(rg.reshape(ro.shape) - ro).max() < 1e-7 * rn, (io, "r")
    co, cg = float(np.sum(f * uo)), float(np.sum(f * ug))
    assert abs(co - cg) < 1e-8 * abs(co)
    return omg.last_iters


def test_level2_above_wave_sweep_threshold_matches_oracle(cut_bc):
    """the production route of a real coarse level: Galerkin element matrices -> stored stencil of a level above
    WAVE_SWEEP_MAX_NODES (no node-major copy, so the split or one-lane stencil sweep), with level 1 on its default pair-row kernel
    and level 0 on the marching sweep (2.27 M nodes)"""
    ne, levels = (32, 64, 1056), 3
    assert level_nodes(ne, 2) == (9, 17, 265)
    assert np.prod(level_nodes(ne, 2)) > WAVE_SWEEP_MAX_NODES
    assert l1_pair_segments(level_nodes(ne, 1)[2], True)[0] == 4
    t0 = time.time()
    o, t, omg, tmg = _mg_pair(ne, cut_bc, levels, nthreads=max(1, min(16, os.cpu_count() or 1)))
    for l in range(levels + 1):
        assert np.array_equal(tmg.getSimulator(l).dirichletMask, omg.sims[l].dmask.astype(bool)), l
    rng = np.random.default_rng(41)
    for l in (0, 1):
        r = rng.standard_normal((omg.sims[l].num_nodes, 3))
        assert relerr(tmg.restriction_device(l, r).cpu().numpy(), omg.restriction(l, r)) < TOL_OP, ("restrict", l)
        c = rng.standard_normal((omg.sims[l + 1].num_nodes, 3))
        assert relerr(tmg.interpolation_device(l, c).cpu().numpy(), omg.interpolation(l, c)) < TOL_OP, ("interpolate", l)
    u0, b = _start(omg, 2, rng)
    ua = rng.standard_normal(u0.shape)
    assert relerr(tmg.applyK(2, ua), omg.apply_k(2, ua)) < TOL_OP
    assert relerr(tmg.computeResidual(2, ua, b), omg.residual(2, ua.copy(), b)) < TOL_OP
    for split in (1, 0):
        _opt(t, STENCIL_SPLIT, split)
        for first in (True, False):
            _sweep_chain(omg, tmg, 2, u0, b, first, ("level 2, split", split))
    _opt(t, STENCIL_SPLIT, 1)
    u1, b1 = _start(omg, 1, rng)
    _sweep_chain(omg, tmg, 1, u1, b1, True, "level 1, default", nsweeps=2)
    iters = _pcg_iterates(o, omg, tmg, 4, 1e-6)
    record_deltas("mg_long_rows_level2", {"seconds": round(time.time() - t0, 1), "pcg_iterations": iters,
                                          "peak_rss_gb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20, 2)})
