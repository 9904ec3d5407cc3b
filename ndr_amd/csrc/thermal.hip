// The heat-conduction entry points of include/vfem.h (vfem_thermal_*).  Handle-free: every call takes the grid, and
// the element matrix or the voxel's edge lengths where its kernel needs them.  Every argument is checked before the first device
// call.
#include "grid_args.h"
#include "thermal.h"
#include "vfem_host.h"

#include <cstdio>

using namespace vfem;

namespace {

constexpr int THERMAL_PCG_CHECK = 8;        // the host looks at the residual once every so many iterations, as the cell problems do

// an output of `len` doubles against the element multipliers and the fixed-node bytes (either may be null)
void check_thermal_output(const std::string &w, const char *name, const ModalGrid &g, const double *out, int64_t len, const double *kappa,
                          const uint8_t *fixed) {
    check_output(w, name, out, len, g, kappa, "the element multipliers", fixed, "the fixed-node mask");
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

void thermal_pcg(const std::string &w, const ModalGrid &g, const ThermalMatrix &K, const double *kappa, const uint8_t *fixed,
                 const double *b, double *x, double tol, int max_iter, int look_every, const ThermalPreconditioner &precondition,
                 int *iterations_out_host, double *relres_out_host, hipStream_t s) {
    const ThermalApply apply = [&](const double *v, const double *rhs, double *out) { launch_thermal_apply(g, K, kappa, fixed, 1, v, rhs, out, s); };
    thermal_pcg(w, g.nnode, apply, "no fixed node, a free node whose incident elements all have zero conductivity", b, x, tol, max_iter,
                look_every, precondition, iterations_out_host, relres_out_host, s);
}

}  // namespace vfem

extern "C" {

int vfem_thermal_apply(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                       int ncols, const double *X, double *Y, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_apply";
    const ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    const ThermalMatrix K = thermal_element_matrix(w, dim, Kc0_host);
    if (!kappa || !X || !Y) throw Error(w + ": null argument");
    check_count(w, "ncols", ncols, THERMAL_MAX_COLS);
    const int64_t len = (int64_t) ncols * g.nnode;
    if (overlaps(Y, len, X, len)) throw Error(w + ": Y aliases X");
    check_thermal_output(w, "Y", g, Y, len, kappa, fixed);
    launch_thermal_apply(g, K, kappa, fixed, ncols, X, nullptr, Y, S(stream));
    VFEM_CATCH
}

int vfem_thermal_diagonal(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                          double *diag, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_diagonal";
    const ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    const ThermalMatrix K = thermal_element_matrix(w, dim, Kc0_host);
    if (!kappa || !diag) throw Error(w + ": null argument");
    check_thermal_output(w, "diag", g, diag, g.nnode, kappa, fixed);
    launch_thermal_diagonal(g, K, kappa, fixed, 0, diag, S(stream));
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
    check_thermal_output(w, "f_out", g, f_out, g.nnode, q, fixed);
    launch_thermal_source(g, q, fixed, f_in, f_out, S(stream));
    VFEM_CATCH
}

int vfem_thermal_band_assemble(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                               double *band, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_band_assemble";
    const ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    const ThermalMatrix K = thermal_element_matrix(w, dim, Kc0_host);
    if (!kappa || !band) throw Error(w + ": null argument");
    long long n, hw;
    thermal_band_geometry(g, n, hw);
    check_thermal_output(w, "band", g, band, band_spd_doubles(n, hw), kappa, fixed);
    launch_thermal_band_assemble(g, K, kappa, fixed, band, S(stream));
    VFEM_CATCH
}

int vfem_thermal_pcg(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                     const double *b, double *x, double tol, int max_iter, int *iterations_out_host, double *relres_out_host,
                     void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_pcg";
    hipStream_t s = S(stream);
    const ModalGrid g = grid_args(w, dim, nelems_host, nullptr, false);
    const ThermalMatrix K = thermal_element_matrix(w, dim, Kc0_host);
    if (!kappa || !b || !x || !iterations_out_host || !relres_out_host) throw Error(w + ": null argument");
    if (!(tol > 0.0) || !std::isfinite(tol) || max_iter < 1) throw Error(w + ": tol must be positive and max_iter at least 1");
    const long long n = g.nnode;
    if (overlaps(x, n, b, n)) throw Error(w + ": x aliases b");
    check_thermal_output(w, "x", g, x, n, kappa, fixed);
    DevBuf<double> dinv;
    dinv.alloc((size_t) n);
    launch_thermal_diagonal(g, K, kappa, fixed, 1, dinv.p, s);
    const ThermalPreconditioner jacobi = [&](const double *r, double *z) { launch_thermal_scale(n, dinv.p, r, z, s); };
    thermal_pcg(w, g, K, kappa, fixed, b, x, tol, max_iter, THERMAL_PCG_CHECK, jacobi, iterations_out_host, relres_out_host, s);
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
