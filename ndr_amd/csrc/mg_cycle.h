// The multigrid algorithm itself, written once for the four hierarchies that run it: the trilinear one (mg.hip: TunedOps), the
// generic one (generic.hip: GenericOps), the slab ranks' (mg_slab.hip: DistDriver) and the periodic cells' (hom_mg.hip: HomOps, the
// V-cycle only: its PCG is batched over the strain cases, hom.hip).  Host code only; control flow follows the
// reference's VoxelFEM/MultigridSolver.hh (MG.hh): vcycle / fullMultigrid / solve / applyPreconditionerInv 447-553,
// preconditionedConjugateGradient 696-732.
// An operations type `Ops` says how each step is launched (plain struct, inline members, resolved at compile time):
//   last_level(), last_level_cycle(fmg)      where the recursion ends and what happens there: the coarsest solve, or the slab ranks'
//                                            replicated cycle;  symmetric(): backward post-smoothing sweeps (MG.hh:549)
//   x(l), b(l)                               iterate and right-hand side of level l (the residual r(l) is the type's own business)
//   enforce_dirichlet(l, residual_system, dirichlet_zeroed)     MG.hh:521-523; may skip what dirichlet_zeroed makes a no-op
//   smooth(l, forward, n)                    n sweeps of x(l) in one direction;  residual(l): r(l) = b(l) - K x(l), Dirichlet zeroed
//   restrict_residual(l)                     b(l+1) = R r(l), x(l+1) = 0;  restrict_rhs(l): b(l+1) = R b(l)
//   prolong_correction(l)                    x(l) += P x(l+1)
//   prolong_start(l, residual_system)        x(l) = P x(l+1); true: the Dirichlet components of a residual system came out zeroed
// and for the conjugate gradients, on level-0 vectors:
//   cg()                                     the CgWork below;  dot(a, b, out): a . b over the whole problem
//   s_vector(preconditioned)                 where M^-1 r is read from: x(0) after a cycle, else a vector the copy of r goes to
//   initial_residual(x, b, r)                r = b - K x, Dirichlet components zeroed
//   shift_and_dot_rs(r, s, sc)               rMr_old = rMr; s = zeroDirichlet(s); rMr = r . s
//   apply_dot(d, Ad, out)                    Ad = zeroDirichlet(K d); out = d . Ad
//   step_dot(x, r, d, Ad, sc)                x += alpha d; r -= alpha Ad; sc[3] = ||r||^2
#pragma once
#include "vfem_host.h"

#include <cmath>

namespace vfem {
namespace mg_cycle {

// dofs of level 0, search direction, K d, device scalars ([0] rMr, [1] rMr_old, [2] d.Ad, [3] ||r||^2, [4] ||b||^2), stream
struct CgWork { long long n; double *d, *Ad, *sc; hipStream_t s; };

// MG.hh:516-553.  dirichlet_zeroed: x(l) has zeros at the Dirichlet components already (just zeroed by the restriction of the level
// above, or interpolated with the mask by full_multigrid), which is all the residual system asks for
template <class Ops> void vcycle(Ops &o, int l, int nsmooth, bool residual_system, bool dirichlet_zeroed = false) {
    if (l == o.last_level()) { o.last_level_cycle(false); return; }
    o.enforce_dirichlet(l, residual_system, dirichlet_zeroed);
    o.smooth(l, 1, nsmooth);
    o.residual(l);
    o.restrict_residual(l);
    vcycle(o, l + 1, nsmooth, true, true);
    o.prolong_correction(l);
    o.smooth(l, o.symmetric() ? 0 : 1, nsmooth);
}

// MG.hh:486-508
template <class Ops> void full_multigrid(Ops &o, int l, int nsmooth, bool residual_system) {
    if (l == o.last_level()) { o.last_level_cycle(true); return; }
    o.restrict_rhs(l);
    full_multigrid(o, l + 1, nsmooth, residual_system);
    const bool zeroed = o.prolong_start(l, residual_system);
    vcycle(o, l, nsmooth, residual_system, zeroed);
}

// MG::solve on the work vectors of level l (x(l), b(l) already set), MG.hh:457-471
template <class Ops> void cycles(Ops &o, int l, int n, int nsmooth, bool residual_system, bool fmg) {
    if (fmg) full_multigrid(o, l, nsmooth, residual_system);
    for (int i = fmg ? 1 : 0; i < n; ++i) vcycle(o, l, nsmooth, residual_system);
}

// what an entry point does with the caller's vectors of level l (n dofs): b, and x unless full multigrid overwrites it, into the
// level's work vectors, the cycles, x back out.  Stream-ordered
template <class Ops>
void cycles_on(Ops &o, int l, long long n, double *x, const double *b, int cycles_n, int nsmooth, bool residual_system, bool fmg, hipStream_t s) {
    const size_t bytes = (size_t) n * sizeof(double);
    VFEM_HIP(hipMemcpyAsync(o.b(l), b, bytes, hipMemcpyDeviceToDevice, s));
    if (!fmg) VFEM_HIP(hipMemcpyAsync(o.x(l), x, bytes, hipMemcpyDeviceToDevice, s));
    cycles(o, l, cycles_n, nsmooth, residual_system, fmg);
    VFEM_HIP(hipMemcpyAsync(x, o.x(l), bytes, hipMemcpyDeviceToDevice, s));
}

// MG.hh:696-732 (x has its Dirichlet values, the operators are current).  The residual lives in b(0) and the preconditioned
// residual is read from x(0): no cycle writes b(0), so neither vector is copied in or out (2 x 3.2 GB per iteration at 512^3).
template <class Ops>
void pcg(Ops &o, double *x, const double *b, int max_iter, double tol, int mg_iterations, int mg_smoothing, bool fmg,
         vfem_residual_cb residual_cb, void *cb_user, int *iters_out, double *relres_out) {
    const CgWork w = o.cg();
    hipStream_t s = w.s;
    const size_t bytes = (size_t) w.n * sizeof(double);
    double *r = o.b(0), *d = w.d, *Ad = w.Ad, *sc = w.sc, *sv = o.s_vector(mg_smoothing != 0), host_sc[2];
    o.dot(b, b, sc + 4);                                                // ||b||^2
    o.initial_residual(x, b, r);                                        // MG.hh:696
    o.dot(r, r, sc + 3);
    VFEM_HIP(hipMemcpyAsync(host_sc, sc + 3, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    VFEM_HIP(hipStreamSynchronize(s));
    double rr = host_sc[0], bb = host_sc[1];
    int it = 0;
    while (it < max_iter && rr > tol * tol * bb) {                      // MG.hh:711 (counter started at 0)
        ++it;
        // s = M^{-1} r  (applyPreconditionerInv, MG.hh:476-479)
        if (mg_smoothing == 0) {
            VFEM_HIP(hipMemcpyAsync(sv, r, bytes, hipMemcpyDeviceToDevice, s));
        } else {
            // full multigrid overwrites the iterate of every level (prolongation, MG.hh:500)
            if (!fmg) VFEM_HIP(hipMemsetAsync(o.x(0), 0, bytes, s));
            cycles(o, 0, mg_iterations, mg_smoothing, true, fmg);
        }
        o.shift_and_dot_rs(r, sv, sc);
        launch_pcg_direction(w.n, sv, d, sc, it == 1, s);
        o.apply_dot(d, Ad, sc + 2);
        o.step_dot(x, r, d, Ad, sc);
        VFEM_HIP(hipMemcpyAsync(host_sc, sc + 3, sizeof(double), hipMemcpyDeviceToHost, s));
        VFEM_HIP(hipStreamSynchronize(s));
        rr = host_sc[0];
        if (!(rr == rr)) throw Error("PCG produced NaN residual");
        if (residual_cb) residual_cb(cb_user, it, std::sqrt(rr));
    }
    if (iters_out) *iters_out = it;
    if (relres_out) *relres_out = bb > 0 ? std::sqrt(rr / bb) : 0.0;
}

}  // namespace mg_cycle
}  // namespace vfem
