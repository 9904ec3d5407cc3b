"""numpy restatement of the design of periodic cells, for the tests, on top of tests/homogenization_cpu.py (imported, not edited):
the periodic box filter by np.roll, the objective J = - sum_qr Cs[q, r] Eh[q, r] with its gradient by the direct solve (or by the
restatement's block-Jacobi / multigrid PCG, to measure what a solver tolerance does to them), and the optimality-criteria step of
OptimalityCriterion.hh with the multiplier bracket persisting from (1, 2).

    filter      (F x)_i = (2r+1)^-d sum over the offsets in [-r, r]^d of x[(i + offset) mod n]; every offset counts once
    objective   J = - Cs : Eh,  dJ/drho_e = - dE_e/drho_e Cs : G_e  (G_e of homogenization_cpu.gradient: positive semidefinite)
    OC step     x <- clip(x sqrt(dJ / (dc lam)), max(x - m, 0), min(x + m, 1)), lam by bisection on the constraint
                1 - mean(F x) / v of the stepped and filtered design until its magnitude is at most ctol

The standard cell of the tests: unit domain, isotropic E = 1, nu = 0.3, gamma = 3, E_min = 1e-3, volume fraction 0.5, filter radius
1, initial design 0.5 everywhere and 0.25 where the element centre is closer than 0.2 to the cell centre, scaled to mean 0.5.
"""
import itertools

import numpy as np

import homogenization_cpu as hc

E0, EMIN, GAMMA, VOLUME_FRACTION, RADIUS, MOVE, CTOL = 1.0, 1e-3, 3.0, 0.5, 1, 0.2, 1e-6
BULK_2D = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
SHEAR_2D = np.diag([0.0, 0.0, 1.0])
BULK_3D = np.zeros((6, 6))
BULK_3D[:3, :3] = 1.0


def periodic_box_filter(x, grid, r):
    """F x on the row-major periodic grid ``grid``; x is flat.  F is symmetric, so this is also its transpose."""
    grid = tuple(int(n) for n in grid)
    y = np.asarray(x, dtype=np.float64).reshape(grid)
    out = np.zeros_like(y)
    offsets = list(itertools.product(range(-int(r), int(r) + 1), repeat=len(grid)))
    for off in offsets:
        out += np.roll(y, [-o for o in off], axis=tuple(range(len(grid))))      # roll by -o: element i receives x[i + o]
    return (out / len(offsets)).reshape(-1)


def standard_design(ne):
    ne = tuple(int(n) for n in ne)
    centres = np.stack(np.meshgrid(*[(np.arange(n) + 0.5) / n for n in ne], indexing="ij"), -1)
    x = np.where(np.linalg.norm(centres - 0.5, axis=-1) < 0.2, 0.25, 0.5).reshape(-1)
    return x * (VOLUME_FRACTION / x.mean())


def standard_cell(ne):
    """(ne, h, D) of the standard cell with ``ne`` elements per axis"""
    ne = tuple(int(n) for n in ne)
    return ne, tuple(1.0 / n for n in ne), hc.isotropic_D(1.0, 0.3, len(ne))


def symmetric_part(C):
    C = np.asarray(C, dtype=np.float64)
    return 0.5 * (C + C.T)


def fields(ne, h, D, rho, solver="direct", tol=None, gamma=GAMMA, Emin=EMIN):
    """dict with K0, L, vol, E, dE, W of the cell problems by ``solver``: "direct", "jacobi" (block-Jacobi PCG to ``tol``) or
    "multigrid" (multigrid PCG to ``tol``, one sweep)"""
    K0, L, vol = hc.element_constants(D, h)
    E, dE = hc.moduli(rho, E0, Emin, gamma)
    K, b = hc.assemble(ne, K0, E), hc.rhs(ne, L, E)
    if solver == "direct":
        W = hc.solve_direct(K, b)
    elif solver == "jacobi":
        W = hc.pcg_columns(K, b, len(ne), tol)[0]
    else:
        import homogenization_mg_cpu as mg
        W = mg.pcg_columns(mg.Hierarchy(ne, K0, E), b, tol, 1)[0]
    return dict(K0=K0, L=L, vol=vol, E=E, dE=dE, W=W)


def tensor_and_gradient(ne, h, D, rho, C, **how):
    """(Eh [S, S], g [numElements]) with g_e = sum_qr C[q, r] dEh[q, r] / drho_e"""
    f = fields(ne, h, D, rho, **how)
    Eh = hc.tensor(ne, f["W"], f["L"], D, f["vol"], f["E"])
    G = hc.gradient(ne, f["W"], f["K0"], f["L"], D, f["vol"])
    return Eh, f["dE"] * np.einsum("qr,eqr->e", np.asarray(C, dtype=np.float64), G)


def objective(ne, h, D, rho, weights, **how):
    """(J, dJ/drho) of J = - Cs : Eh at the physical densities ``rho``"""
    Cs = symmetric_part(weights)
    Eh, g = tensor_and_gradient(ne, h, D, rho, Cs, **how)
    return -float(np.sum(Cs * Eh)), -g


def filtered_objective(ne, h, D, x, weights, r=RADIUS, **how):
    """(J, dJ/dx) of the design variables ``x`` behind the periodic filter of radius ``r``"""
    J, g = objective(ne, h, D, periodic_box_filter(x, ne, r), weights, **how)
    return J, periodic_box_filter(g, ne, r)


class OC:
    """OCOptimizer::step (OptimalityCriterion.hh:30-81) for one volume constraint behind the periodic filter"""

    def __init__(self, ne, h, D, weights, r=RADIUS, v=VOLUME_FRACTION, **how):
        self.ne, self.h, self.D, self.weights, self.r, self.v, self.how = ne, h, D, weights, r, v, how
        self.lmin, self.lmax = 1.0, 2.0

    def constraint(self, x):
        return 1.0 - periodic_box_filter(x, self.ne, self.r).mean() / self.v

    def step(self, x, dJ=None, m=MOVE, ctol=CTOL):
        """the next design; ``dJ``: the filtered gradient at ``x`` when the caller has it"""
        if dJ is None:
            dJ = filtered_objective(self.ne, self.h, self.D, x, self.weights, self.r, **self.how)[1]
        dc = periodic_box_filter(np.full(x.size, -1.0 / (self.v * x.size)), self.ne, self.r)

        def stepped(lam):
            with np.errstate(invalid="ignore"):
                cand = x * np.sqrt(dJ / (dc * lam))
            return np.minimum(np.minimum(np.maximum(np.maximum(cand, x - m), 0.0), x + m), 1.0)

        ceval = lambda lam: self.constraint(stepped(lam))
        while ceval(self.lmin) > 0:
            self.lmax = self.lmin
            self.lmin /= 2
        while ceval(self.lmax) < 0:
            self.lmin = self.lmax
            self.lmax *= 2
        mid = 0.5 * (self.lmin + self.lmax)
        vol = ceval(mid)
        while abs(vol) > ctol:
            if vol < 0:
                self.lmin = mid
            if vol > 0:
                self.lmax = mid
            mid = 0.5 * (self.lmin + self.lmax)
            vol = ceval(mid)
        return stepped(mid)


def trajectory(ne, weights, steps, **how):
    """(J_0 .. J_steps, final design) of ``steps`` OC steps on the standard cell from the standard design"""
    ne, h, D = standard_cell(ne)
    oc = OC(ne, h, D, weights, **how)
    x = standard_design(ne)
    J = []
    for _ in range(steps):
        value, dJ = filtered_objective(ne, h, D, x, weights, **how)
        J.append(value)
        x = oc.step(x, dJ)
    J.append(filtered_objective(ne, h, D, x, weights, **how)[0])
    return np.array(J), x
