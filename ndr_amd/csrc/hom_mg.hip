// The multigrid-preconditioned PCG of the periodic cell problems (include/vfem.h: vfem_hom_mg_*; DESIGN "Periodic homogenisation").
// A handle holds the hierarchy of one cell: level 0 matrix-free, Galerkin levels stored (hom_mg.h), the coarsest level as a dense
// inverse (CoarsestSolver).  It is built once per solve; the moduli it reads at level 0 stay the caller's.
#include "hom_mg.h"
#include "mg_stored.h"

#include <memory>

using namespace vfem;

struct HomMgLevel {
    HomGrid g;
    DevBuf<double> A;               // levels >= 1: [3^N][N][N][nodes], the unpinned Galerkin operator
    DevBuf<double> Dinv;            // levels >= 1: [N N][nodes]
    DevBuf<double> x, b, r;         // levels >= 1: [S][nodes][N] (r: smoothed levels only)
};

struct vfem_hom_mg {
    HomCall call;                   // level 0: the cell, its tables, the caller's moduli
    std::vector<HomMgLevel> lv;
    DevBuf<double> Minv0, r0;       // level 0: launch_hom_jacobi's inverses and the residual (hierarchies of more than one level)
    DevBuf<uint8_t> pin;            // coarsest level: the mask with node 0 fixed
    CoarsestSolver coarsest;
    int N() const { return call.p.N; }
    int L() const { return (int) lv.size() - 1; }
    HomBlocks blocks(int l) const { return l == 0 ? HomBlocks{call.p.stencil, call.p.E} : HomBlocks{lv[l].A.p, nullptr}; }
    HomDinv dinv(int l) const {
        const long long nn = (long long) N() * N();
        return l == 0 ? HomDinv{Minv0.p, nn, 1} : HomDinv{lv[l].Dinv.p, 1, lv[l].g.pn};
    }
    size_t vec(int l) const { return (size_t) lv[l].g.S * lv[l].g.pn * lv[l].g.N; }
    long long bytes() const {
        size_t n = call.tables.n + Minv0.n + r0.n;
        for (const HomMgLevel &v : lv) n += v.A.n + v.Dinv.n + v.x.n + v.b.n + v.r.n;
        return (long long) (n * sizeof(double)) + coarsest.bytes() + (long long) pin.n;
    }
};

namespace {

bool can_colour(const HomGrid &g) {
    for (int d = 0; d < g.N; ++d)
        if (g.n[d] % 2) return false;
    return true;
}

// one sweep over the 2^N colours, ascending (forward) or descending
void sweep(vfem_hom_mg *h, int l, double *x, const double *b, int forward, hipStream_t s) {
    const int nc = 1 << h->N();
    for (int k = 0; k < nc; ++k)
        launch_hom_mg_sweep_colour(h->lv[l].g, h->blocks(l), h->dinv(l), forward ? k : nc - 1 - k, x, b, s);
}

// what mg_cycle::vcycle launches on a cell's hierarchy: level 0 works on the caller's X and B and on r0, a stored level on its own
struct HomOps {
    vfem_hom_mg *h;
    const double *B;
    double *X;
    hipStream_t s;
    int last_level() const { return h->L(); }
    bool symmetric() const { return true; }
    const HomGrid &g(int l) const { return h->lv[l].g; }
    double *x(int l) const { return l == 0 ? X : h->lv[l].x.p; }
    const double *b(int l) const { return l == 0 ? B : h->lv[l].b.p; }
    double *r(int l) const { return l == 0 ? h->r0.p : h->lv[l].r.p; }
    void last_level_cycle(bool) {
        if (h->coarsest.held != CoarsestSolver::DENSE) throw Error("the coarsest level holds no dense inverse");
        launch_hom_mg_gemv(g(h->L()), h->coarsest.Ainv.p, b(h->L()), x(h->L()), s);
    }
    void enforce_dirichlet(int, bool, bool) {}  // the pin is applied inside the kernels
    void smooth(int l, int forward, int n) { for (int k = 0; k < n; ++k) sweep(h, l, x(l), b(l), forward, s); }
    void residual(int l) { launch_hom_mg_residual(g(l), h->blocks(l), x(l), b(l), r(l), s); }
    void restrict_residual(int l) {
        launch_hom_mg_restrict(g(l), g(l + 1), r(l), h->lv[l + 1].b.p, s);
        // a smoothed level starts from zero; the coarsest x is overwritten by the dense product
        if (l + 1 < h->L()) VFEM_HIP(hipMemsetAsync(x(l + 1), 0, h->vec(l + 1) * sizeof(double), s));
    }
    void prolong_correction(int l) { launch_hom_mg_prolong_add(g(l), g(l + 1), x(l + 1), x(l), s); }
};

}  // namespace

extern "C" {

int vfem_hom_mg_create(vfem_hom_mg **out, int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host,
                       const double *D_host, double vol, const double *E, int max_coarsenings, void *stream) {
    VFEM_TRY
    if (!out) throw Error("vfem_hom_mg_create: null argument");
    *out = nullptr;
    hipStream_t s = S(stream);
    std::unique_ptr<vfem_hom_mg> h(new vfem_hom_mg);
    hom_setup(h->call, "vfem_hom_mg_create", dim, nelems_host, K0_host, L_host, D_host, vol, E, s);
    const HomProblem &p = h->call.p;
    const int N = p.N;
    // the levels (max_coarsenings < 0: as far as the extents allow)
    const auto ladder = coarsening_ladder(N, p.n, max_coarsenings);
    const std::string sizes = ladder_text(N, ladder);
    HomGrid g = p;
    for (const std::array<int, 3> &n : ladder) {
        g.pn = 1;
        for (int d = 0; d < N; ++d) { g.n[d] = n[d]; g.pn *= n[d]; }
        h->lv.emplace_back();
        h->lv.back().g = g;
    }
    const int L = h->L();
    const long long nc = (long long) g.pn * N;
    if (nc > DENSE_COARSEST_MAX_DOFS)
        throw Error("vfem_hom_mg_create: the coarsest level of the hierarchy " + sizes + " has " + std::to_string(nc) +
                    " dofs, above the limit of " + std::to_string(DENSE_COARSEST_MAX_DOFS) +
                    " of the dense coarsest-level solve (a level is coarsened only while every extent is even and at least 4)");
    const int noff = N == 2 ? 9 : 27;
    if (L > 0) {
        h->Minv0.alloc((size_t) p.pn * N * N);
        h->r0.alloc(h->vec(0));
        launch_hom_jacobi(p, h->Minv0.p, s);
    }
    for (int l = 1; l <= L; ++l) {
        HomMgLevel &v = h->lv[l];
        v.A.alloc((size_t) noff * N * N * v.g.pn);
        v.Dinv.alloc((size_t) N * N * v.g.pn);
        v.x.alloc(h->vec(l));
        v.b.alloc(h->vec(l));
        if (l < L) v.r.alloc(h->vec(l));
        launch_hom_mg_galerkin(h->lv[l - 1].g, v.g, h->blocks(l - 1), v.A.p, s);
        launch_hom_mg_dinv(v.g, v.A.p, v.Dinv.p, s);
    }
    // the coarsest level: the dense pinned matrix, inverted; the rows and columns of the pin zeroed in the inverse
    std::vector<uint8_t> mask((size_t) g.pn, 0);
    mask[0] = (uint8_t) ((1 << N) - 1);
    h->pin.alloc(mask.size());
    VFEM_HIP(hipMemcpyAsync(h->pin.p, mask.data(), mask.size(), hipMemcpyHostToDevice, s));
    double *M = h->coarsest.dense_matrix(nc, s);
    launch_hom_mg_dense(g, h->blocks(L), M, s);
    h->coarsest.factor_dense(N, h->pin.p, s);
    VFEM_HIP(hipStreamSynchronize(s));          // `mask` goes out of scope; the factorisation's workspace is not needed again
    h->coarsest.work = DenseWork();
    *out = h.release();
    VFEM_CATCH
}

int vfem_hom_mg_destroy(vfem_hom_mg *h) {
    VFEM_TRY
    delete h;
    VFEM_CATCH
}

int vfem_hom_mg_num_levels(vfem_hom_mg *h) { return h ? (int) h->lv.size() : 0; }

int64_t vfem_hom_mg_bytes(vfem_hom_mg *h) { return h ? h->bytes() : 0; }

int vfem_hom_mg_level_dims(vfem_hom_mg *h, int l, int64_t *n_out) {
    VFEM_TRY
    check_level(h, l, "vfem_hom_mg_level_dims", h ? h->L() : 0);
    if (!n_out) throw Error("vfem_hom_mg_level_dims: null argument");
    for (int d = 0; d < h->N(); ++d) n_out[d] = h->lv[l].g.n[d];
    VFEM_CATCH
}

int vfem_hom_mg_level_apply(vfem_hom_mg *h, int l, const double *W_in, double *W_out, void *stream) {
    VFEM_TRY
    check_level(h, l, "vfem_hom_mg_level_apply", h ? h->L() : 0);
    if (!W_in || !W_out || W_in == W_out) throw Error("vfem_hom_mg_level_apply: W_in and W_out must be two arrays");
    if (l == 0) launch_hom_apply(h->call.p, W_in, W_out, nullptr, S(stream));
    else launch_hom_mg_apply(h->lv[l].g, h->lv[l].A.p, W_in, W_out, S(stream));
    VFEM_CATCH
}

int vfem_hom_mg_smooth(vfem_hom_mg *h, int l, double *X, const double *B, int forward, void *stream) {
    VFEM_TRY
    check_level(h, l, "vfem_hom_mg_smooth", h ? h->L() : 0);
    if (!X || !B) throw Error("vfem_hom_mg_smooth: null argument");
    if (!can_colour(h->lv[l].g)) throw Error("vfem_hom_mg_smooth: the colour sweep needs an even extent along every axis (level " + dims_text(h->N(), h->lv[l].g.n) + ")");
    if (l == 0 && !h->Minv0.p) {                // a one-level hierarchy never smooths: the inverses are made on demand
        h->Minv0.alloc((size_t) h->call.p.pn * h->N() * h->N());
        launch_hom_jacobi(h->call.p, h->Minv0.p, S(stream));
    }
    sweep(h, l, X, B, forward, S(stream));
    VFEM_CATCH
}

int vfem_hom_mg_restrict(vfem_hom_mg *h, int l, const double *fine, double *coarse, void *stream) {
    VFEM_TRY
    check_level(h, l, "vfem_hom_mg_restrict", h ? h->L() - 1 : 0);
    if (!fine || !coarse) throw Error("vfem_hom_mg_restrict: null argument");
    launch_hom_mg_restrict(h->lv[l].g, h->lv[l + 1].g, fine, coarse, S(stream));
    VFEM_CATCH
}

int vfem_hom_mg_prolong_add(vfem_hom_mg *h, int l, const double *coarse, double *fine, void *stream) {
    VFEM_TRY
    check_level(h, l, "vfem_hom_mg_prolong_add", h ? h->L() - 1 : 0);
    if (!fine || !coarse) throw Error("vfem_hom_mg_prolong_add: null argument");
    launch_hom_mg_prolong_add(h->lv[l].g, h->lv[l + 1].g, coarse, fine, S(stream));
    VFEM_CATCH
}

int vfem_hom_mg_vcycle(vfem_hom_mg *h, const double *B, double *X, int smoothing, void *stream) {
    VFEM_TRY
    if (!h || !B || !X || B == X) throw Error("vfem_hom_mg_vcycle: B and X must be two arrays");
    check_smoothing(smoothing, "vfem_hom_mg_vcycle");
    cycle_from_zero<HomOps>(h, B, X, smoothing, S(stream));
    VFEM_CATCH
}

int vfem_hom_mg_solve_cells(vfem_hom_mg *h, double *W, double tol, int max_iter, int smoothing, int *iterations_out_host,
                            double *relres_out_host, void *stream) {
    VFEM_TRY
    hipStream_t s = S(stream);
    if (!h || !W || !iterations_out_host || !relres_out_host) throw Error("vfem_hom_mg_solve_cells: null argument");
    if (!(tol > 0.0) || max_iter < 1) throw Error("vfem_hom_mg_solve_cells: tol must be positive and max_iter at least 1");
    check_smoothing(smoothing, "vfem_hom_mg_solve_cells");
    const HomProblem &p = h->call.p;
    // z = V-cycle(r) on all S columns at once; a one-level hierarchy is the exact inverse
    const HomPreconditioner multigrid{[&](bool first, const HomPcgVectors &v) {
        if (!first) launch_hom_mg_update(p, v.pv, v.Ap, v.x, v.r, v.st, s);
        cycle_from_zero<HomOps>(h, v.r, v.z, smoothing, s);
        launch_hom_mg_dots(p, v.r, v.z, v.partial, s);
    }, h->L() == 0};
    hom_pcg(p, "vfem_hom_mg_solve_cells", multigrid, W, tol, max_iter, iterations_out_host, relres_out_host, s);
    VFEM_CATCH
}

}  // extern "C"
