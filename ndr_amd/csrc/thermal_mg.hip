// The multigrid-preconditioned PCG of the scalar heat operator (include/vfem.h: vfem_thermal_mg_*, vfem_transient_mg_create; DESIGN
// 3.16, 3.18).  A handle holds the hierarchy of one grid, one operator (thermal.h: one-term, or the two-term form of a transient
// step) and one mask: level 0 matrix-free from the caller's kappa and cap, the Galerkin levels stored (thermal_mg.h), the coarsest
// level as a dense inverse (CoarsestSolver).  Nothing below level 0's launchers knows which form the operator has.  The V-cycle is mg_cycle::vcycle, the colour
// order for_each_gs_color, the PCG loop thermal_pcg (thermal.hip) with z = V-cycle(r).  Every argument is checked before the first
// device call.
#include "grid_args.h"
#include "mg_stored.h"
#include "thermal_mg.h"

#include <memory>

using namespace vfem;

struct ThermalMgLevel {
    ModalGrid g;
    DevBuf<uint8_t> fixed;          // 0 / 1 per node
    DevBuf<double> A;               // levels >= 1: [3^N][nodes]
    DevBuf<double> dinv;            // smoothed levels: 1 / diag A_l
    DevBuf<double> x, b, r;         // levels >= 1: iterate and right-hand side; smoothed levels: the residual (level 0 too)
};

struct vfem_thermal_mg {
    ThermalOp fine;                 // level 0's operator: kappa (and cap) are the caller's, read by every level-0 kernel
    const uint8_t *fixed_in;        // the caller's mask (may be null); the levels use their normalised copies
    std::vector<ThermalMgLevel> lv;
    CoarsestSolver coarsest;
    int N() const { return lv[0].g.N; }
    int L() const { return (int) lv.size() - 1; }
    size_t vec(int l) const { return (size_t) lv[l].g.nnode; }
    ThermalLevelOp op(int l) const {
        return l == 0 ? ThermalLevelOp{nullptr, &fine} : ThermalLevelOp{lv[l].A.p, nullptr};
    }
    long long bytes() const {
        size_t d = 0, m = 0;
        for (const ThermalMgLevel &v : lv) {
            d += v.A.n + v.dinv.n + v.x.n + v.b.n + v.r.n;
            m += v.fixed.n;
        }
        return (long long) (d * sizeof(double) + m) + coarsest.bytes();
    }
};

namespace {

// a one-level hierarchy never smooths: its inverted diagonal is made on demand
void need_dinv0(vfem_thermal_mg *h, hipStream_t s) {
    ThermalMgLevel &v = h->lv[0];
    if (v.dinv.p) return;
    v.dinv.alloc((size_t) v.g.nnode);
    launch_thermal_diagonal(v.g, h->fine, v.fixed.p, 1, v.dinv.p, s);
}

// one sweep over the 2^N colours of the level's nodes, ascending (forward) or descending
void sweep(vfem_thermal_mg *h, int l, double *x, const double *b, int forward, hipStream_t s) {
    const ThermalMgLevel &v = h->lv[l];
    const int nn[3] = {v.g.ne[0] + 1, v.g.ne[1] + 1, v.g.N == 3 ? v.g.ne[2] + 1 : 1};
    const ThermalLevelOp src = h->op(l);
    for_each_gs_color(v.g.N, 1, nn, forward, 0, 1 << v.g.N, [&](const GsColor &col) {
        launch_thermal_mg_sweep_colour(v.g, src, v.fixed.p, v.dinv.p, col, x, b, s);
    });
}

void level_apply(vfem_thermal_mg *h, int l, const double *x, const double *b, double *out, hipStream_t s) {
    const ThermalMgLevel &v = h->lv[l];
    if (l == 0) launch_thermal_apply(v.g, h->fine, v.fixed.p, 1, 1, x, b, 1, out, s);
    else launch_thermal_mg_apply(v.g, v.A.p, v.fixed.p, x, b, out, s);
}

// what mg_cycle::vcycle launches on the hierarchy: level 0 works on the caller's X and B, a stored level on its own vectors
struct ThermalOps {
    vfem_thermal_mg *h;
    const double *B;
    double *X;
    hipStream_t s;
    int last_level() const { return h->L(); }
    bool symmetric() const { return true; }
    double *x(int l) const { return l == 0 ? X : h->lv[l].x.p; }
    const double *b(int l) const { return l == 0 ? B : h->lv[l].b.p; }
    double *r(int l) const { return h->lv[l].r.p; }
    void last_level_cycle(bool) {
        const int L = h->L();
        h->coarsest.solve(b(L), x(L), s);
        launch_thermal_mg_copy_fixed(h->lv[L].g.nnode, h->lv[L].fixed.p, b(L), x(L), s);
    }
    void enforce_dirichlet(int, bool, bool) {}  // the identity of the fixed nodes is applied inside the kernels
    void smooth(int l, int forward, int n) { for (int k = 0; k < n; ++k) sweep(h, l, x(l), b(l), forward, s); }
    void residual(int l) { level_apply(h, l, x(l), b(l), r(l), s); }
    void restrict_residual(int l) {
        launch_thermal_mg_restrict(h->lv[l].g, h->lv[l + 1].g, h->lv[l].fixed.p, h->lv[l + 1].fixed.p, r(l), h->lv[l + 1].b.p, s);
        // a smoothed level starts from zero; the coarsest x is overwritten by the dense product
        if (l + 1 < h->L()) VFEM_HIP(hipMemsetAsync(x(l + 1), 0, h->vec(l + 1) * sizeof(double), s));
    }
    void prolong_correction(int l) {
        launch_thermal_mg_prolong_add(h->lv[l].g, h->lv[l + 1].g, h->lv[l].fixed.p, h->lv[l + 1].fixed.p, x(l + 1), x(l), s);
    }
};

// the body of both creates; two_term: level 0 takes mb_host [dim + 1] and cap beside Kc0_host and kappa
void create(const std::string &w, vfem_thermal_mg **out, int dim, const int64_t *nelems_host, const double *Kc0_host, bool two_term,
            const double *mb_host, const double *kappa, const double *cap, const uint8_t *fixed, int max_coarsenings, void *stream) {
    if (!out) throw Error(w + ": null argument");
    *out = nullptr;
    hipStream_t s = S(stream);
    ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    std::unique_ptr<vfem_thermal_mg> h(new vfem_thermal_mg);
    h->fine = thermal_operator_args(w, dim, Kc0_host, two_term, mb_host, kappa, cap);
    h->fixed_in = fixed;
    const int N = g.N;
    // the levels (max_coarsenings < 0: as far as the extents allow); a coarser voxel has twice the edge lengths
    const auto ladder = coarsening_ladder(N, g.ne, max_coarsenings);
    const std::string sizes = ladder_text(N, ladder);
    for (size_t l = 0; l < ladder.size(); ++l) {
        g.nelem = g.nnode = 1;
        for (int d = 0; d < N; ++d) {
            g.ne[d] = ladder[l][d];
            if (l > 0) g.h[d] *= 2.0;
            g.nelem *= g.ne[d];
            g.nnode *= g.ne[d] + 1;
        }
        h->lv.emplace_back();
        h->lv.back().g = g;
    }
    const int L = h->L();
    const long long nc = g.nnode;
    if (nc > DENSE_COARSEST_MAX_DOFS)
        throw Error(w + ": the coarsest level of the hierarchy " + sizes + " has " + std::to_string(nc) + " nodes, above the limit of " +
                    std::to_string(DENSE_COARSEST_MAX_DOFS) +
                    " of the dense coarsest-level solve (a level is coarsened only while every extent is even and at least 4 elements)");
    const int noff = N == 2 ? 9 : 27;
    // the masks, normalised to 0 / 1
    for (int l = 0; l <= L; ++l) {
        ThermalMgLevel &v = h->lv[l];
        v.fixed.alloc((size_t) v.g.nnode);
        if (l > 0) launch_thermal_mg_coarsen_mask(h->lv[l - 1].g, v.g, h->lv[l - 1].fixed.p, v.fixed.p, s);
        else if (fixed) launch_thermal_mg_normalise_mask(v.g.nnode, fixed, v.fixed.p, s);
        else v.fixed.zero(s);
    }
    if (L > 0) {
        need_dinv0(h.get(), s);
        h->lv[0].r.alloc((size_t) h->lv[0].g.nnode);
    }
    for (int l = 1; l <= L; ++l) {
        ThermalMgLevel &v = h->lv[l];
        const size_t nn = (size_t) v.g.nnode;
        v.A.alloc((size_t) noff * nn);
        v.x.alloc(nn);
        v.b.alloc(nn);
        launch_thermal_mg_galerkin(h->lv[l - 1].g, v.g, h->op(l - 1), h->lv[l - 1].fixed.p, v.fixed.p, v.A.p, s);
        if (l < L) {
            v.r.alloc(nn);
            v.dinv.alloc(nn);
            launch_thermal_mg_dinv(v.g, v.A.p, v.fixed.p, v.dinv.p, s);
        }
    }
    // the coarsest level: the dense A_L, inverted
    double *M = h->coarsest.dense_matrix(nc, s);
    launch_thermal_mg_dense(g, h->op(L), h->lv[L].fixed.p, M, s);
    try {
        h->coarsest.factor_dense(1, h->lv[L].fixed.p, s);
    } catch (const Error &e) {                  // a pivot that is not positive: what the PCG would report as its breakdown
        throw Error(w + ": breakdown at the coarsest level of the hierarchy " + sizes + ": " + e.what() +
                    "; the operator is singular: " + thermal_singular_because(h->fine) + ", or non-finite data");
    }
    VFEM_HIP(hipStreamSynchronize(s));          // the factorisation's workspace is not needed again
    h->coarsest.work = DenseWork();
    *out = h.release();
}

}  // namespace

extern "C" {

int vfem_thermal_mg_create(vfem_thermal_mg **out, int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa,
                           const uint8_t *fixed, int max_coarsenings, void *stream) {
    VFEM_TRY
    create("vfem_thermal_mg_create", out, dim, nelems_host, Kc0_host, false, nullptr, kappa, nullptr, fixed, max_coarsenings, stream);
    VFEM_CATCH
}

int vfem_transient_mg_create(vfem_thermal_mg **out, int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host,
                             const double *kappa, const double *cap, const uint8_t *fixed, int max_coarsenings, void *stream) {
    VFEM_TRY
    create("vfem_transient_mg_create", out, dim, nelems_host, Ka_host, true, mb_host, kappa, cap, fixed, max_coarsenings, stream);
    VFEM_CATCH
}

int vfem_thermal_mg_destroy(vfem_thermal_mg *h) {
    VFEM_TRY
    delete h;
    VFEM_CATCH
}

int vfem_thermal_mg_num_levels(vfem_thermal_mg *h) { return h ? (int) h->lv.size() : 0; }

int64_t vfem_thermal_mg_bytes(vfem_thermal_mg *h) { return h ? h->bytes() : 0; }

int vfem_thermal_mg_level_dims(vfem_thermal_mg *h, int l, int64_t *n_out) {
    VFEM_TRY
    check_level(h, l, "vfem_thermal_mg_level_dims", h ? h->L() : 0);
    if (!n_out) throw Error("vfem_thermal_mg_level_dims: null argument");
    for (int d = 0; d < h->N(); ++d) n_out[d] = h->lv[l].g.ne[d];
    VFEM_CATCH
}

int vfem_thermal_mg_level_fixed(vfem_thermal_mg *h, int l, uint8_t *fixed_out, void *stream) {
    VFEM_TRY
    check_level(h, l, "vfem_thermal_mg_level_fixed", h ? h->L() : 0);
    if (!fixed_out) throw Error("vfem_thermal_mg_level_fixed: null argument");
    VFEM_HIP(hipMemcpyAsync(fixed_out, h->lv[l].fixed.p, (size_t) h->lv[l].g.nnode, hipMemcpyDeviceToDevice, S(stream)));
    VFEM_CATCH
}

int vfem_thermal_mg_level_apply(vfem_thermal_mg *h, int l, const double *X, double *Y, void *stream) {
    VFEM_TRY
    if (!X || !Y) throw Error("vfem_thermal_mg_level_apply: null argument");
    check_level(h, l, "vfem_thermal_mg_level_apply", h ? h->L() : 0);
    if (overlaps(Y, h->lv[l].g.nnode, X, h->lv[l].g.nnode)) throw Error("vfem_thermal_mg_level_apply: Y aliases X");
    level_apply(h, l, X, nullptr, Y, S(stream));
    VFEM_CATCH
}

int vfem_thermal_mg_smooth(vfem_thermal_mg *h, int l, double *X, const double *B, int forward, void *stream) {
    VFEM_TRY
    if (!X || !B) throw Error("vfem_thermal_mg_smooth: null argument");
    check_level(h, l, "vfem_thermal_mg_smooth", h ? h->L() : 0);
    if (overlaps(X, h->lv[l].g.nnode, B, h->lv[l].g.nnode)) throw Error("vfem_thermal_mg_smooth: X aliases B");
    if (l == 0) need_dinv0(h, S(stream));
    else if (!h->lv[l].dinv.p) {                // the coarsest level is solved, not smoothed, in a cycle
        h->lv[l].dinv.alloc((size_t) h->lv[l].g.nnode);
        launch_thermal_mg_dinv(h->lv[l].g, h->lv[l].A.p, h->lv[l].fixed.p, h->lv[l].dinv.p, S(stream));
    }
    sweep(h, l, X, B, forward, S(stream));
    VFEM_CATCH
}

int vfem_thermal_mg_restrict(vfem_thermal_mg *h, int l, const double *fine, double *coarse, void *stream) {
    VFEM_TRY
    if (!fine || !coarse) throw Error("vfem_thermal_mg_restrict: null argument");
    check_level(h, l, "vfem_thermal_mg_restrict", h ? h->L() - 1 : 0);
    if (overlaps(coarse, h->lv[l + 1].g.nnode, fine, h->lv[l].g.nnode)) throw Error("vfem_thermal_mg_restrict: coarse aliases fine");
    launch_thermal_mg_restrict(h->lv[l].g, h->lv[l + 1].g, h->lv[l].fixed.p, h->lv[l + 1].fixed.p, fine, coarse, S(stream));
    VFEM_CATCH
}

int vfem_thermal_mg_prolong_add(vfem_thermal_mg *h, int l, const double *coarse, double *fine, void *stream) {
    VFEM_TRY
    if (!fine || !coarse) throw Error("vfem_thermal_mg_prolong_add: null argument");
    check_level(h, l, "vfem_thermal_mg_prolong_add", h ? h->L() - 1 : 0);
    if (overlaps(coarse, h->lv[l + 1].g.nnode, fine, h->lv[l].g.nnode)) throw Error("vfem_thermal_mg_prolong_add: fine aliases coarse");
    launch_thermal_mg_prolong_add(h->lv[l].g, h->lv[l + 1].g, h->lv[l].fixed.p, h->lv[l + 1].fixed.p, coarse, fine, S(stream));
    VFEM_CATCH
}

int vfem_thermal_mg_vcycle(vfem_thermal_mg *h, const double *B, double *X, int smoothing, void *stream) {
    VFEM_TRY
    // what needs no handle first, so that every refusal can be had without one
    if (!B || !X) throw Error("vfem_thermal_mg_vcycle: null argument");
    check_smoothing(smoothing, "vfem_thermal_mg_vcycle");
    if (!h) throw Error("vfem_thermal_mg_vcycle: null handle");
    if (overlaps(X, h->lv[0].g.nnode, B, h->lv[0].g.nnode)) throw Error("vfem_thermal_mg_vcycle: X aliases B");
    cycle_from_zero<ThermalOps>(h, B, X, smoothing, S(stream));
    VFEM_CATCH
}

int vfem_thermal_mg_pcg(vfem_thermal_mg *h, const double *b, double *x, double tol, int max_iter, int smoothing,
                        int *iterations_out_host, double *relres_out_host, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_mg_pcg";
    hipStream_t s = S(stream);
    if (!b || !x || !iterations_out_host || !relres_out_host) throw Error(w + ": null argument");
    if (!(tol > 0.0) || !std::isfinite(tol) || max_iter < 1) throw Error(w + ": tol must be positive and max_iter at least 1");
    check_smoothing(smoothing, w.c_str());
    if (!h) throw Error(w + ": null handle");
    const ModalGrid &g = h->lv[0].g;
    if (overlaps(x, g.nnode, b, g.nnode)) throw Error(w + ": x aliases b");
    // z = V-cycle(r); the host looks after every iteration, so the count is exact: a look costs little beside a cycle
    const ThermalPreconditioner multigrid = [&](const double *r, double *z) { cycle_from_zero<ThermalOps>(h, r, z, smoothing, s); };
    const ThermalApply apply = [&](const double *v, const double *rhs, double *res) { level_apply(h, 0, v, rhs, res, s); };
    thermal_pcg(w, g.nnode, apply, thermal_singular_because(h->fine), b, x, tol, max_iter, 1, multigrid, iterations_out_host,
                relres_out_host, s);
    VFEM_CATCH
}

}  // extern "C"
