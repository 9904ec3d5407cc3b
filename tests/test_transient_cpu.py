"""The restatement of transient heat conduction (tests/transient_cpu.py) against itself, without a GPU: the adjoint gradient against
central differences, the decay of a discrete mode, the energy balance without a sink and the large-dt limit.  Run with -s it prints the
figures that tests/test_gpu_transient.py pins."""
import numpy as np
import pytest

import thermal_cpu as tc
import transient_cpu as tr


def _name(ne):
    return "x".join(map(str, ne))


@pytest.mark.parametrize("ne,theta,lumping", [((6, 5), 1.0, 0.0), ((6, 5), 0.5, 0.0), ((4, 3, 3), 0.7, 1.0)], ids=["6x5-be", "6x5-cn", "4x3x3-lumped"])
def test_adjoint_gradient_matches_central_differences(ne, theta, lumping):
    """step 1e-6, S = 4, random rho in [0.2, 1], random T0, Q and weights; bound: 1e-8 of the largest gradient entry (the rounding of
    the difference quotient is about 1e-10; measured 1.4e-10, 9.1e-11, 1.3e-10)"""
    N = len(ne)
    rng = np.random.default_rng(2100 + tc.num_elements(ne))
    nn, nel = tc.num_nodes(ne), tc.num_elements(ne)
    rho, T0, Q, W = rng.uniform(0.2, 1.0, nel), rng.standard_normal(nn), rng.standard_normal(nn), rng.standard_normal((5, nn))
    fixed = tc.face_mask(ne, 0, 0)
    W[:, fixed] = 0.0
    make = lambda r: tr.Problem(ne, tc.EDGES[N], tc.K_ANISO[N], r, fixed, Q, 4, 0.05, theta, T0, rng_s, lumping=lumping, q=2.0)
    rng_s = rng.uniform(0.5, 1.5, 5)
    J, g = make(rho).weighted(W)
    fd = np.empty(nel)
    for e in range(nel):
        d = np.zeros(nel)
        d[e] = 1e-6
        fd[e] = (make(rho + d).weighted(W)[0] - make(rho - d).weighted(W)[0]) / 2e-6
    err = np.abs(g - fd).max() / np.abs(g).max()
    print("adjoint gradient %s theta %.1f lumping %.0f: %.2e of the largest entry" % (_name(ne), theta, lumping, err))
    assert err <= 1e-8


@pytest.mark.parametrize("theta,lumping", tr.DECAY_CASES)
def test_decay_of_a_discrete_mode(theta, lumping):
    pr, exact = tr.decay_case(theta, lumping)
    err = np.abs(pr.T[3] - exact).max() / np.abs(exact).max()
    print("decay theta %.1f lumping %.0f: factor %.6f, T^3 within %.2e (pinned %.1e)" % (theta, lumping, tr.decay_factor(1.0, 1 / 16, 0.01, theta, lumping), err, tr.DECAY_MEASURED[(theta, lumping)]))
    assert err <= 3.0 * tr.DECAY_MEASURED[(theta, lumping)]


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("ne", tr.ENERGY_SHAPES, ids=_name)
def test_energy_balance_without_a_sink(ne, theta):
    f = tr.energy_case(ne, theta)
    Q = tc.load(ne, f["h"], None, volumetric=f["q"])
    pr = tr.Problem(ne, f["h"], f["k"], f["rho"], f["fixed"], Q, f["steps"], f["dt"], theta, f["T0"])
    err = tr.energy_error(ne, pr.C(), pr.T, Q, f["dt"])
    print("energy balance %s theta %.1f: %.2e of 1^T Q (pinned %.1e)" % (_name(ne), theta, err, tr.ENERGY_MEASURED[ne]))
    assert err <= 3.0 * tr.ENERGY_MEASURED[ne]


@pytest.mark.parametrize("ne", [(16, 6), (6, 4, 3)], ids=_name)
def test_one_large_backward_euler_step_is_the_steady_solve(ne):
    """dt = 1e9.  With E = C / dt and x = |K^-1| |E| <= cond(K) |C| / (dt |K|) < 1 (2-norms, K the steady operator with its identity rows),
    |(K + E)^-1 Q - K^-1 Q| <= x / (1 - x) |K^-1 Q|: the bound of the test"""
    f = tc.direct_fixture(ne)
    J, T, g, Q = tc.compliance(ne, f["h"], f["k"], f["rho"], f["fixed"], f["nodal"], f["volumetric"])
    dt = 1e9
    pr = tr.Problem(ne, f["h"], f["k"], f["rho"], f["fixed"], Q, 1, dt, 1.0)
    K = tc.assemble(ne, pr.Kc0, pr.kap, f["fixed"])
    C = tr.assemble(ne, 0.0 * pr.Kc0, tr.capacity_matrix(pr.m), pr.kap, pr.cp, f["fixed"], 0)
    x = np.linalg.cond(K) * np.linalg.norm(C, 2) / (dt * np.linalg.norm(K, 2))
    err = np.linalg.norm(pr.T[1] - T) / np.linalg.norm(T)
    print("large-dt limit %s: dt %.0e, |T^1 - T| / |T| = %.2e, bound %.2e" % (_name(ne), dt, err, x / (1.0 - x)))
    assert x < 0.1 and err <= x / (1.0 - x)


def test_capacity_matrix_is_the_tensor_product_and_its_row_sums():
    for h in (tc.EDGES[2], tc.EDGES[3]):
        N = len(h)
        one = [np.array([[2.0, 1.0], [1.0, 2.0]]) * hd / 6.0 for hd in h]
        M = one[0]
        for o in one[1:]:
            M = np.kron(M, o)
        assert np.abs(tr.capacity_matrix(tr.capacity_entries(h)) - M).max() < 1e-17
        lumped = tr.capacity_matrix(tr.capacity_entries(h, lumping=1.0))
        assert np.abs(lumped - np.diag(M.sum(axis=1))).max() < 1e-17


@pytest.mark.parametrize("key", sorted(tr.MG_PCG_COUNT), ids=lambda k: "%s-%s" % (_name(k[0]), k[1]))
def test_multigrid_pcg_counts_of_the_two_term_operator_are_pinned(key):
    """the hierarchy of a step's operator: the Galerkin chain keeps the coarse operators symmetric, the PCG takes the pinned count, and
    without any fixed node (where the steady operator is singular) it converges as well"""
    x, info, direct = tr.mg_pcg_solution(*key)
    H = tr.mg_hierarchy(*key)
    for A in H.A[1:]:
        D = A.dense()
        assert np.abs(D - D.T).max() <= 1e-15 * np.abs(D).max()
    sol = np.abs(x - direct).max() / np.abs(direct).max()
    print("multigrid-PCG of the two-term operator %s %s: %d iterations, gap %.1e, solution %.2e of the largest entry" % (_name(key[0]), key[1], info["iterations"], info["gap"], sol))
    assert info["converged"] and info["iterations"] == tr.MG_PCG_COUNT[key]


@pytest.mark.parametrize("ne", tr.MARCH_SHAPES, ids=_name)
def test_multigrid_pcg_march_against_the_direct_march(ne):
    Td, Tp, counts = tr.march_both(ne)
    err = np.abs(Td - Tp).max() / np.abs(Td).max()
    print("multigrid-PCG march %s: counts %s, %.2e of the largest temperature (pinned %.1e)" % (_name(ne), counts, err, tr.MARCH_MEASURED[ne]))
    assert counts == tr.MARCH_COUNTS[ne] and max(counts[1:]) <= counts[0]
    assert err <= 3.0 * tr.MARCH_MEASURED[ne]


def test_jacobi_pcg_march_against_the_direct_march():
    ne = (16, 12)
    (T, counts), Td = tr.march_jacobi(ne), tr.march_both(ne)[0]
    err = np.abs(T - Td).max() / np.abs(Td).max()
    print("Jacobi-PCG march %s: counts %s, %.2e of the largest temperature (pinned %.1e)" % (_name(ne), counts, err, tr.MARCH_JACOBI_MEASURED[ne]))
    assert counts == tr.MARCH_JACOBI_COUNTS[ne] and err <= 3.0 * tr.MARCH_JACOBI_MEASURED[ne]
