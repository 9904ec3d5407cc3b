// The periodic-homogenisation entry points of include/vfem.h: batched periodic apply, the cell problems by a batched
// block-Jacobi PCG, the homogenised tensor and its density gradient.  Handle-free: every call takes the cell's element constants.
// hom_pcg is the batched PCG itself, which hom_mg.hip runs with its V-cycle in place of block Jacobi.
#include "hom.h"
#include "vfem_host.h"

#include <cmath>

using namespace vfem;

namespace vfem {

void hom_setup(HomCall &c, const char *who, int dim, const int64_t *nelems, const double *K0, const double *L, const double *D,
               double vol, const double *E, hipStream_t s) {
    const std::string w(who);
    if (dim != 2 && dim != 3) throw Error(w + ": dim must be 2 or 3");
    if (!nelems || !K0 || !L || !D || !E) throw Error(w + ": null argument");
    HomProblem &p = c.p;
    p.N = dim;
    p.S = dim == 2 ? 3 : 6;
    p.ke = dim * (1 << dim);
    long long pn = 1;
    p.n[2] = 1;
    for (int d = 0; d < dim; ++d) {
        if (nelems[d] < 2) throw Error(w + ": a periodic cell needs at least 2 elements along every axis");
        if (nelems[d] > (1 << 27)) throw Error(w + ": cell too large");
        p.n[d] = (int) nelems[d];
        pn *= nelems[d];
        if (pn > (1 << 27)) throw Error(w + ": cell too large (more than 2^27 elements)");
    }
    p.pn = (int) pn;
    if (!(vol > 0.0) || !std::isfinite(vol)) throw Error(w + ": the voxel volume must be positive");
    p.vol = vol;
    p.E = E;
    const size_t nk = (size_t) p.ke * p.ke, nl = (size_t) p.ke * p.S, nd = (size_t) p.S * p.S;
    const size_t nst = (size_t) (dim == 2 ? 9 : 27) * (1 << dim) * dim * dim;
    std::vector<double> host(nk + nl + nd + nst);
    std::copy(K0, K0 + nk, host.begin());
    std::copy(L, L + nl, host.begin() + nk);
    std::copy(D, D + nd, host.begin() + nk + nl);
    hom_build_stencil(dim, K0, host.data() + nk + nl + nd);
    for (double v : host)
        if (!std::isfinite(v)) throw Error(w + ": element constants are not finite");
    c.tables.alloc(host.size());
    VFEM_HIP(hipMemcpyAsync(c.tables.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, s));
    VFEM_HIP(hipStreamSynchronize(s));          // `host` goes out of scope
    p.K0 = c.tables.p;
    p.L = c.tables.p + nk;
    p.D = c.tables.p + nk + nl;
    p.stencil = c.tables.p + nk + nl + nd;
}

void hom_pcg(const HomProblem &p, const char *who, const HomPreconditioner &M, double *W, double tol, int max_iter,
             int *iterations_out_host, double *relres_out_host, hipStream_t s) {
    const size_t nv = (size_t) p.S * p.pn * p.N;
    DevBuf<double> r, z, pv, Ap, partial;
    DevBuf<HomState> st;
    r.alloc(nv); z.alloc(nv); pv.alloc(nv); Ap.alloc(nv);
    partial.alloc((size_t) 2 * p.S * hom_node_blocks(p));
    st.alloc(1);
    st.zero(s); pv.zero(s); Ap.zero(s);
    VFEM_HIP(hipMemsetAsync(W, 0, nv * sizeof(double), s));
    const HomPcgVectors v{W, r.p, z.p, pv.p, Ap.p, partial.p, st.p};
    // the second half of an iteration; the first time: x = 0, r = b, z = M^-1 r, p = z
    auto precondition = [&](bool first) {
        M.step(first, v);
        launch_hom_finish_beta(p, partial.p, st.p, tol, first, s);
        launch_hom_direction(p, z.p, pv.p, st.p, s);
    };
    launch_hom_rhs(p, r.p, s);
    precondition(true);
    HomState h;
    auto read_state = [&]() {
        VFEM_HIP(hipMemcpyAsync(&h, st.p, sizeof(HomState), hipMemcpyDeviceToHost, s));
        VFEM_HIP(hipStreamSynchronize(s));
        for (int q = 0; q < p.S; ++q)
            if (h.active[q]) return true;
        return false;
    };
    bool running = read_state();
    for (int it = 1; running && it <= max_iter; ++it) {
        launch_hom_apply(p, pv.p, Ap.p, partial.p, s);
        launch_hom_finish_alpha(p, partial.p, st.p, s);
        precondition(false);
        // the host looks at the residual norms once every 8 iterations (a frozen column no longer moves in between); an exact
        // preconditioner is done after the first
        if (it % 8 == 0 || it == max_iter || (it == 1 && M.exact)) running = read_state();
    }
    // a column is done when its right-hand side is zero or its residual has met the tolerance; a NaN on either side is not done
    int worst = 0, broken = -1;
    for (int q = 0; q < p.S; ++q) {
        iterations_out_host[q] = h.iters[q];
        relres_out_host[q] = h.bb[q] == 0.0 ? 0.0 : std::isfinite(h.bb[q]) ? std::sqrt(h.rr[q] / h.bb[q]) : std::nan("");
        if (relres_out_host[q] > relres_out_host[worst]) worst = q;
        const bool done = h.bb[q] == 0.0 || h.rr[q] <= tol * tol * h.bb[q];
        if (!done && broken < 0) broken = q;
    }
    char msg[512];
    if (running) {
        snprintf(msg, sizeof msg, "%s: no convergence in %d iterations: strain case %d has |r|/|b| = %.3e (tol %.3e)", who, max_iter, worst,
                 relres_out_host[worst], tol);
        throw Error(msg);
    }
    // every column froze, one of them short of the tolerance: its r . z stopped being positive
    if (broken >= 0) {
        snprintf(msg, sizeof msg, "%s: breakdown in strain case %d after %d iterations: r . z = %.3e is not positive (|r|/|b| = %.3e, tol %.3e); "
                 "the cell is singular: a node whose incident elements all have zero modulus, or non-finite moduli", who, broken,
                 h.iters[broken], h.rz[broken], relres_out_host[broken], tol);
        throw Error(msg);
    }
}

}  // namespace vfem

namespace {

double cell_volume_of(const HomProblem &p, double cell_volume, const char *who) {
    if (!(cell_volume > 0.0) || !std::isfinite(cell_volume)) throw Error(std::string(who) + ": the cell volume must be positive");
    return cell_volume;
}

}  // namespace

extern "C" {

int vfem_hom_apply(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host, const double *D_host, double vol,
                   const double *E, const double *W_in, double *W_out, void *stream) {
    VFEM_TRY
    HomCall c;
    hom_setup(c, "vfem_hom_apply", dim, nelems_host, K0_host, L_host, D_host, vol, E, S(stream));
    if (!W_in || !W_out || W_in == W_out) throw Error("vfem_hom_apply: W_in and W_out must be two arrays");
    launch_hom_apply(c.p, W_in, W_out, nullptr, S(stream));
    VFEM_HIP(hipStreamSynchronize(S(stream)));  // the tables are freed on return
    VFEM_CATCH
}

int vfem_hom_solve_cells(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host, const double *D_host,
                         double vol, const double *E, double *W, double tol, int max_iter, int *iterations_out_host,
                         double *relres_out_host, void *stream) {
    VFEM_TRY
    hipStream_t s = S(stream);
    HomCall c;
    hom_setup(c, "vfem_hom_solve_cells", dim, nelems_host, K0_host, L_host, D_host, vol, E, s);
    const HomProblem &p = c.p;
    if (!W || !iterations_out_host || !relres_out_host) throw Error("vfem_hom_solve_cells: null argument");
    if (!(tol > 0.0) || max_iter < 1) throw Error("vfem_hom_solve_cells: tol must be positive and max_iter at least 1");
    // block Jacobi: the fused update kernel; with alpha = 0 (the zeroed state) its first call is the first preconditioning
    DevBuf<double> Minv;
    Minv.alloc((size_t) p.pn * p.N * p.N);
    launch_hom_jacobi(p, Minv.p, s);
    const HomPreconditioner jacobi{[&](bool, const HomPcgVectors &v) {
        launch_hom_update(p, Minv.p, v.pv, v.Ap, v.x, v.r, v.z, v.st, v.partial, s);
    }, false};
    hom_pcg(p, "vfem_hom_solve_cells", jacobi, W, tol, max_iter, iterations_out_host, relres_out_host, s);
    VFEM_CATCH
}

int vfem_hom_tensor(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host, const double *D_host, double vol,
                    const double *E, const double *W, double cell_volume, double *Eh_host, void *stream) {
    VFEM_TRY
    hipStream_t s = S(stream);
    HomCall c;
    hom_setup(c, "vfem_hom_tensor", dim, nelems_host, K0_host, L_host, D_host, vol, E, s);
    const HomProblem &p = c.p;
    if (!W || !Eh_host) throw Error("vfem_hom_tensor: null argument");
    const double cell = cell_volume_of(p, cell_volume, "vfem_hom_tensor");
    const int ss = p.S * p.S;
    DevBuf<double> partial, Eh;
    partial.alloc((size_t) ss * hom_tensor_blocks(p));
    Eh.alloc(ss);
    launch_hom_tensor(p, W, 1.0 / cell, partial.p, Eh.p, s);
    VFEM_HIP(hipMemcpyAsync(Eh_host, Eh.p, ss * sizeof(double), hipMemcpyDeviceToHost, s));
    VFEM_HIP(hipStreamSynchronize(s));
    VFEM_CATCH
}

int vfem_hom_tensor_gradient(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host, const double *D_host,
                             double vol, const double *E, const double *W, double cell_volume, const double *dE, double *G,
                             void *stream) {
    VFEM_TRY
    hipStream_t s = S(stream);
    HomCall c;
    hom_setup(c, "vfem_hom_tensor_gradient", dim, nelems_host, K0_host, L_host, D_host, vol, E, s);
    if (!W || !G) throw Error("vfem_hom_tensor_gradient: null argument");
    const double cell = cell_volume_of(c.p, cell_volume, "vfem_hom_tensor_gradient");
    launch_hom_gradient(c.p, W, dE, 1.0 / cell, G, s);
    VFEM_HIP(hipStreamSynchronize(s));          // the tables are freed on return
    VFEM_CATCH
}

int vfem_hom_tensor_gradient_contract(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host,
                                      const double *D_host, double vol, const double *E, const double *W, double cell_volume,
                                      const double *dE, const double *C_host, double *g, void *stream) {
    VFEM_TRY
    hipStream_t s = S(stream);
    HomCall c;
    hom_setup(c, "vfem_hom_tensor_gradient_contract", dim, nelems_host, K0_host, L_host, D_host, vol, E, s);
    if (!W || !C_host || !g) throw Error("vfem_hom_tensor_gradient_contract: null argument");
    const double cell = cell_volume_of(c.p, cell_volume, "vfem_hom_tensor_gradient_contract");
    // G_e is symmetric, so only (C + C^T) / 2 acts: entry (q, r), q < r, stands for both mirrored entries
    const int n = c.p.S;
    std::vector<double> host((size_t) n * n, 0.0);
    for (int q = 0; q < n; ++q)
        for (int r = q; r < n; ++r) {
            const double a = C_host[q * n + r], b = C_host[r * n + q];
            if (!std::isfinite(a) || !std::isfinite(b)) throw Error("vfem_hom_tensor_gradient_contract: C is not finite");
            host[q * n + r] = q == r ? a : a + b;
        }
    DevBuf<double> wt;
    wt.alloc(host.size());
    VFEM_HIP(hipMemcpyAsync(wt.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, s));
    launch_hom_gradient_contract(c.p, W, dE, 1.0 / cell, wt.p, g, s);
    VFEM_HIP(hipStreamSynchronize(s));          // the tables and `host` are freed on return
    VFEM_CATCH
}

}  // extern "C"
