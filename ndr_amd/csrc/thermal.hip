// The heat-conduction entry points of include/vfem.h that take the operator: the steady ones (vfem_thermal_*)
// and their two-term twins of a transient step (vfem_transient_{apply, diagonal, band_assemble, pcg}), which are wrappers over one
// body each.  Handle-free: every call takes the grid, and the element matrix or the voxel's edge lengths where its kernel needs
// them; the transient calls take the capacity entries and the element capacities too, with the scalars of the time scheme folded in
// by the caller.  Every argument is checked before the first device call.
#include "grid_args.h"
#include "thermal.h"
#include "vfem_host.h"

#include <cstdio>

using namespace vfem;

namespace {

constexpr int THERMAL_PCG_CHECK = 8;        // the host looks at the residual once every so many iterations, as the cell problems do

// an output of `len` doubles against the operator's element fields and the fixed-node bytes (may be null)
void check_operator_output(const std::string &w, const char *name, const ModalGrid &g, const double *out, int64_t len, const ThermalOp &op,
                           const uint8_t *fixed) {
    check_output(w, name, out, len, g, op.kappa, op.cap ? "the element conductivities" : "the element multipliers", fixed, "the fixed-node mask");
    if (op.cap) check_output(w, name, out, len, g, op.cap, "the element capacities", nullptr, "");
}

// The bodies of the paired entry points; two_term: the call takes mb_host [dim + 1] and cap beside K_host and kappa

void apply_entry(const std::string &w, int dim, const int64_t *nelems_host, const double *K_host, bool two_term, const double *mb_host,
                 const double *kappa, const double *cap, const uint8_t *fixed, int identity, int ncols, const double *X, const double *b,
                 double *Y, void *stream) {
    const ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    const ThermalOp op = thermal_operator_args(w, dim, K_host, two_term, mb_host, kappa, cap);
    if (!X || !Y) throw Error(w + ": null argument");
    if (identity != 0 && identity != 1) throw Error(w + ": identity must be 0 or 1");
    check_count(w, "ncols", ncols, THERMAL_MAX_COLS);
    const int64_t len = (int64_t) ncols * g.nnode;
    if (overlaps(Y, len, X, len)) throw Error(w + ": Y aliases X");
    if (b && overlaps(Y, len, b, len)) throw Error(w + ": Y aliases b");
    check_operator_output(w, "Y", g, Y, len, op, fixed);
    launch_thermal_apply(g, op, fixed, identity, ncols, X, b, 0, Y, S(stream));
}

void diagonal_entry(const std::string &w, int dim, const int64_t *nelems_host, const double *K_host, bool two_term, const double *mb_host,
                    const double *kappa, const double *cap, const uint8_t *fixed, double *diag, void *stream) {
    const ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    const ThermalOp op = thermal_operator_args(w, dim, K_host, two_term, mb_host, kappa, cap);
    if (!diag) throw Error(w + ": null argument");
    check_operator_output(w, "diag", g, diag, g.nnode, op, fixed);
    launch_thermal_diagonal(g, op, fixed, 0, diag, S(stream));
}

void band_entry(const std::string &w, int dim, const int64_t *nelems_host, const double *K_host, bool two_term, const double *mb_host,
                const double *kappa, const double *cap, const uint8_t *fixed, double *band, void *stream) {
    const ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    const ThermalOp op = thermal_operator_args(w, dim, K_host, two_term, mb_host, kappa, cap);
    if (!band) throw Error(w + ": null argument");
    long long n, hw;
    thermal_band_geometry(g, n, hw);
    check_operator_output(w, "band", g, band, band_spd_doubles(n, hw), op, fixed);
    launch_thermal_band_assemble(g, op, fixed, band, S(stream));
}

void pcg_entry(const std::string &w, int dim, const int64_t *nelems_host, const double *K_host, bool two_term, const double *mb_host,
               const double *kappa, const double *cap, const uint8_t *fixed, const double *b, double *x, double tol, int max_iter,
               int *iterations_out_host, double *relres_out_host, void *stream) {
    hipStream_t s = S(stream);
    const ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    const ThermalOp op = thermal_operator_args(w, dim, K_host, two_term, mb_host, kappa, cap);
    if (!b || !x || !iterations_out_host || !relres_out_host) throw Error(w + ": null argument");
    if (!(tol > 0.0) || !std::isfinite(tol) || max_iter < 1) throw Error(w + ": tol must be positive and max_iter at least 1");
    const long long n = g.nnode;
    if (overlaps(x, n, b, n)) throw Error(w + ": x aliases b");
    check_operator_output(w, "x", g, x, n, op, fixed);
    DevBuf<double> dinv;
    dinv.alloc((size_t) n);
    launch_thermal_diagonal(g, op, fixed, 1, dinv.p, s);
    const ThermalPreconditioner jacobi = [&](const double *r, double *z) { launch_thermal_scale(n, dinv.p, r, z, s); };
    const ThermalApply apply = [&](const double *v, const double *rhs, double *out) { launch_thermal_apply(g, op, fixed, 1, 1, v, rhs, 1, out, s); };
    thermal_pcg(w, n, apply, thermal_singular_because(op), b, x, tol, max_iter, THERMAL_PCG_CHECK, jacobi, iterations_out_host,
                relres_out_host, s);
}

}  // namespace

namespace vfem {

ThermalMatrix thermal_element_matrix(const std::string &w, int dim, const double *Kc0) {
    if (!Kc0) throw Error(w + ": null argument");
    const int npe = 1 << dim;
    check_finite(w, "the element matrix is", Kc0, npe * npe);
    ThermalMatrix K{};
    for (int i = 0; i < npe * npe; ++i) K.k[i] = Kc0[i];
    return K;
}

ThermalCapacity thermal_capacity_entries(const std::string &w, int dim, const double *m_host) {
    if (!m_host) throw Error(w + ": null argument");
    check_finite(w, "the capacity entries are", m_host, dim + 1);
    ThermalCapacity m{};
    for (int d = 0; d <= dim; ++d) m.m[d] = m_host[d];
    return m;
}

ThermalOp thermal_operator_args(const std::string &w, int dim, const double *K_host, bool two_term, const double *mb_host,
                                const double *kappa, const double *cap) {
    ThermalOp op{};
    op.K = thermal_element_matrix(w, dim, K_host);
    if (two_term) op.mb = thermal_capacity_entries(w, dim, mb_host);
    if (!kappa || (two_term && !cap)) throw Error(w + ": null argument");
    op.kappa = kappa;
    op.cap = two_term ? cap : nullptr;
    return op;
}

void thermal_pcg(const std::string &w, long long n, const ThermalApply &apply, const char *singular_because, const double *b, double *x,
                 double tol, int max_iter, int look_every, const ThermalPreconditioner &precondition, int *iterations_out_host,
                 double *relres_out_host, hipStream_t s) {
    *iterations_out_host = 0;
    *relres_out_host = 0.0;

    DevBuf<double> vec, sc, scratch;
    vec.alloc((size_t) 4 * n);
    sc.alloc(8);
    scratch.alloc(REDUCE_SCRATCH_DOUBLES);
    sc.zero(s);
    double *r = vec.p, *z = r + n, *d = z + n, *Ad = d + n;
    double host[8];
    auto read = [&]() {
        VFEM_HIP(hipMemcpyAsync(host, sc.p, sizeof host, hipMemcpyDeviceToHost, s));
        VFEM_HIP(hipStreamSynchronize(s));
    };
    launch_dot(n, b, b, scratch.p, sc.p + 4, s);
    apply(x, b, r);                                                     // r = b - A x
    launch_dot(n, r, r, scratch.p, sc.p + 3, s);
    read();
    const double bb = host[4];
    double rr = host[3];
    if (bb == 0.0) {                                                    // A is positive definite: the solution is zero
        VFEM_HIP(hipMemsetAsync(x, 0, (size_t) n * sizeof(double), s));
        VFEM_HIP(hipStreamSynchronize(s));
        return;
    }
    int it = 0;
    bool done = rr <= tol * tol * bb;
    char msg[512];
    while (!done && it < max_iter) {
        ++it;
        launch_shift_scalar(sc.p, s);                                   // the last r.z
        precondition(r, z);
        launch_dot(n, r, z, scratch.p, sc.p, s);
        launch_thermal_pcg_guard(sc.p, 0, it, s);
        launch_pcg_direction(n, z, d, sc.p, it == 1, s);
        apply(d, nullptr, Ad);
        launch_dot(n, d, Ad, scratch.p, sc.p + 2, s);
        launch_thermal_pcg_guard(sc.p, 1, it, s);
        launch_pcg_step_dot(n, x, r, d, Ad, sc.p, scratch.p, sc.p + 3, s);
        if (it % look_every == 0 || it == max_iter) {
            read();
            rr = host[3];
            if (host[5] != 0.0) {
                *iterations_out_host = (int) host[5];
                *relres_out_host = std::sqrt(host[7] / bb);
                snprintf(msg, sizeof msg, "%s: breakdown at iteration %d: p . Ap = %.3e is not positive (|r|/|b| = %.3e, tol %.3e); the "
                         "operator is singular: %s, or non-finite data", w.c_str(), (int) host[5], host[6], *relres_out_host, tol,
                         singular_because);
                throw Error(msg);
            }
            done = rr <= tol * tol * bb;
            if (!(rr == rr)) break;
        }
    }
    *iterations_out_host = it;
    *relres_out_host = std::sqrt(rr / bb);
    if (!done) {
        snprintf(msg, sizeof msg, "%s: not converged after %d iterations: |r|/|b| = %.3e (tol %.3e)", w.c_str(), it, *relres_out_host, tol);
        throw Error(msg);
    }
}

}  // namespace vfem

extern "C" {

int vfem_thermal_apply(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                       int ncols, const double *X, double *Y, void *stream) {
    VFEM_TRY
    apply_entry("vfem_thermal_apply", dim, nelems_host, Kc0_host, false, nullptr, kappa, nullptr, fixed, 1, ncols, X, nullptr, Y, stream);
    VFEM_CATCH
}

int vfem_thermal_diagonal(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                          double *diag, void *stream) {
    VFEM_TRY
    diagonal_entry("vfem_thermal_diagonal", dim, nelems_host, Kc0_host, false, nullptr, kappa, nullptr, fixed, diag, stream);
    VFEM_CATCH
}

int vfem_thermal_source(int dim, const int64_t *nelems_host, const double *h_host, const double *q, const uint8_t *fixed,
                        const double *f_in, double *f_out, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_source";
    if (!h_host) throw Error(w + ": null argument");            // (this call refuses missing edge lengths before a bad dim)
    const ModalGrid g = grid_args(w, dim, nelems_host, h_host, true);
    if (!f_out) throw Error(w + ": null argument");
    if (!q && !f_in) throw Error(w + ": null argument: neither a volumetric nor a nodal source");
    if (f_in && f_in != f_out && overlaps(f_out, g.nnode, f_in, g.nnode)) throw Error(w + ": f_out overlaps f_in without being f_in");
    check_output(w, "f_out", f_out, g.nnode, g, q, "the element multipliers", fixed, "the fixed-node mask");
    launch_thermal_source(g, q, fixed, f_in, f_out, S(stream));
    VFEM_CATCH
}

int vfem_thermal_band_assemble(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                               double *band, void *stream) {
    VFEM_TRY
    band_entry("vfem_thermal_band_assemble", dim, nelems_host, Kc0_host, false, nullptr, kappa, nullptr, fixed, band, stream);
    VFEM_CATCH
}

int vfem_thermal_pcg(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                     const double *b, double *x, double tol, int max_iter, int *iterations_out_host, double *relres_out_host,
                     void *stream) {
    VFEM_TRY
    pcg_entry("vfem_thermal_pcg", dim, nelems_host, Kc0_host, false, nullptr, kappa, nullptr, fixed, b, x, tol, max_iter,
              iterations_out_host, relres_out_host, stream);
    VFEM_CATCH
}

int vfem_transient_apply(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                         const double *cap, const uint8_t *fixed, int identity, int ncols, const double *X, const double *b, double *Y,
                         void *stream) {
    VFEM_TRY
    apply_entry("vfem_transient_apply", dim, nelems_host, Ka_host, true, mb_host, kappa, cap, fixed, identity, ncols, X, b, Y, stream);
    VFEM_CATCH
}

int vfem_transient_diagonal(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                            const double *cap, const uint8_t *fixed, double *diag, void *stream) {
    VFEM_TRY
    diagonal_entry("vfem_transient_diagonal", dim, nelems_host, Ka_host, true, mb_host, kappa, cap, fixed, diag, stream);
    VFEM_CATCH
}

int vfem_transient_band_assemble(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                                 const double *cap, const uint8_t *fixed, double *band, void *stream) {
    VFEM_TRY
    band_entry("vfem_transient_band_assemble", dim, nelems_host, Ka_host, true, mb_host, kappa, cap, fixed, band, stream);
    VFEM_CATCH
}

int vfem_transient_pcg(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                       const double *cap, const uint8_t *fixed, const double *b, double *x, double tol, int max_iter,
                       int *iterations_out_host, double *relres_out_host, void *stream) {
    VFEM_TRY
    pcg_entry("vfem_transient_pcg", dim, nelems_host, Ka_host, true, mb_host, kappa, cap, fixed, b, x, tol, max_iter, iterations_out_host,
              relres_out_host, stream);
    VFEM_CATCH
}

int vfem_thermal_gradient(int dim, const int64_t *nelems_host, int ncols, const double *Kc0_host, const double *c_host,
                          const double *dkappa, const double *A, const double *B, double *g, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_gradient";
    const ModalGrid grid = grid_args(w, dim, nelems_host, nullptr, false);
    check_count(w, "ncols", ncols, THERMAL_MAX_COLS);
    const ThermalMatrix K = thermal_element_matrix(w, dim, Kc0_host);
    if (!c_host || !dkappa || !A || !B || !g) throw Error(w + ": null argument");
    check_finite(w, "the coefficients are", c_host, ncols);
    ThermalCoef c{};
    for (int i = 0; i < ncols; ++i) c.c[i] = c_host[i];
    const int64_t len = (int64_t) ncols * grid.nnode;
    if (overlaps(g, grid.nelem, A, len) || overlaps(g, grid.nelem, B, len) || overlaps(g, grid.nelem, dkappa, grid.nelem))
        throw Error(w + ": g aliases an input");
    launch_thermal_gradient(grid, K, ncols, c, dkappa, A, B, g, S(stream));
    VFEM_CATCH
}

int vfem_thermal_flux(int dim, const int64_t *nelems_host, const double *h_host, const double *k_host, const double *kappa,
                      const double *T, double *flux, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_flux";
    if (!h_host) throw Error(w + ": null argument");            // (this call refuses missing edge lengths before a bad dim)
    const ModalGrid g = grid_args(w, dim, nelems_host, h_host, true);
    if (!k_host || !kappa || !T || !flux) throw Error(w + ": null argument");
    check_finite(w, "the conductivity tensor is", k_host, dim * dim);
    ThermalTensor k{};
    for (int i = 0; i < dim * dim; ++i) k.k[i] = k_host[i];
    if (overlaps(flux, g.nelem * dim, T, g.nnode) || overlaps(flux, g.nelem * dim, kappa, g.nelem)) throw Error(w + ": flux aliases an input");
    launch_thermal_flux(g, k, kappa, T, flux, S(stream));
    VFEM_CATCH
}

}  // extern "C"
