// The heat-conduction entry points of include/vfem.h (vfem_thermal_*).  Handle-free: every call takes the grid, and
// the element matrix or the voxel's edge lengths where its kernel needs them.  Every argument is checked before the first device
// call.
#include "thermal.h"
#include "vfem_host.h"

#include <cmath>
#include <cstdio>

using namespace vfem;

namespace {

constexpr int THERMAL_PCG_CHECK = 8;        // the host looks at the residual once every so many iterations, as the cell problems do

ModalGrid thermal_setup(const std::string &w, int dim, const int64_t *nelems, const double *h) {
    if (dim != 2 && dim != 3) throw Error(w + ": dim must be 2 or 3");
    if (!nelems) throw Error(w + ": null argument");
    ModalGrid g;
    g.N = dim;
    g.ne[2] = 1;
    g.h[0] = g.h[1] = g.h[2] = 1.0;
    g.nelem = g.nnode = 1;
    for (int d = 0; d < dim; ++d) {
        if (nelems[d] < 1) throw Error(w + ": every extent must be at least 1 element");
        if (nelems[d] > (1 << 27)) throw Error(w + ": grid too large");
        if (h) {
            if (!(h[d] > 0.0) || !std::isfinite(h[d])) throw Error(w + ": the voxel's edge lengths must be positive");
            g.h[d] = h[d];
        }
        g.ne[d] = (int) nelems[d];
        g.nelem *= nelems[d];
        g.nnode *= nelems[d] + 1;
        if (g.nnode > (1LL << 31)) throw Error(w + ": grid too large (more than 2^31 nodes)");
    }
    return g;
}

ThermalMatrix thermal_matrix(const std::string &w, int dim, const double *Kc0) {
    if (!Kc0) throw Error(w + ": null argument");
    ThermalMatrix K{};
    const int npe = 1 << dim;
    for (int i = 0; i < npe * npe; ++i) {
        if (!std::isfinite(Kc0[i])) throw Error(w + ": the element matrix is not finite");
        K.k[i] = Kc0[i];
    }
    return K;
}

void check_columns(const std::string &w, int k) {
    if (k < 1 || k > THERMAL_MAX_COLS)
        throw Error(w + ": ncols must be 1 to " + std::to_string(THERMAL_MAX_COLS) + " (got " + std::to_string(k) + ")");
}

bool overlaps_bytes(const void *a, int64_t na, const void *b, int64_t nb) {
    const char *pa = (const char *) a, *pb = (const char *) b;
    return pa < pb + nb && pb < pa + na;
}

bool overlaps(const double *a, int64_t na, const double *b, int64_t nb) {
    return overlaps_bytes(a, na * (int64_t) sizeof(double), b, nb * (int64_t) sizeof(double));
}

// an output of `len` doubles against the element multipliers and the fixed-node bytes
void check_output(const std::string &w, const char *name, const ModalGrid &g, const double *out, int64_t len, const double *kappa,
                  const uint8_t *fixed) {
    if (kappa && overlaps(out, len, kappa, g.nelem)) throw Error(w + ": " + name + " aliases the element multipliers");
    if (fixed && overlaps_bytes(out, len * (int64_t) sizeof(double), fixed, g.nnode)) throw Error(w + ": " + name + " aliases the fixed-node mask");
}

}  // namespace

namespace vfem {

ModalGrid thermal_grid(const std::string &w, int dim, const int64_t *nelems) { return thermal_setup(w, dim, nelems, nullptr); }
ThermalMatrix thermal_element_matrix(const std::string &w, int dim, const double *Kc0) { return thermal_matrix(w, dim, Kc0); }

void thermal_pcg(const std::string &w, const ModalGrid &g, const ThermalMatrix &K, const double *kappa, const uint8_t *fixed,
                 const double *b, double *x, double tol, int max_iter, int look_every, const ThermalPreconditioner &precondition,
                 int *iterations_out_host, double *relres_out_host, hipStream_t s) {
    const long long n = g.nnode;
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
    launch_thermal_apply(g, K, kappa, fixed, 1, x, b, r, s);            // r = b - A x
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
        launch_thermal_apply(g, K, kappa, fixed, 1, d, nullptr, Ad, s);
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
                         "operator is singular: no fixed node, a free node whose incident elements all have zero conductivity, or "
                         "non-finite data", w.c_str(), (int) host[5], host[6], *relres_out_host, tol);
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
    const std::string w = "vfem_thermal_apply";
    const ModalGrid g = thermal_setup(w, dim, nelems_host, nullptr);
    const ThermalMatrix K = thermal_matrix(w, dim, Kc0_host);
    if (!kappa || !X || !Y) throw Error(w + ": null argument");
    check_columns(w, ncols);
    const int64_t len = (int64_t) ncols * g.nnode;
    if (overlaps(Y, len, X, len)) throw Error(w + ": Y aliases X");
    check_output(w, "Y", g, Y, len, kappa, fixed);
    launch_thermal_apply(g, K, kappa, fixed, ncols, X, nullptr, Y, S(stream));
    VFEM_CATCH
}

int vfem_thermal_diagonal(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                          double *diag, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_diagonal";
    const ModalGrid g = thermal_setup(w, dim, nelems_host, nullptr);
    const ThermalMatrix K = thermal_matrix(w, dim, Kc0_host);
    if (!kappa || !diag) throw Error(w + ": null argument");
    check_output(w, "diag", g, diag, g.nnode, kappa, fixed);
    launch_thermal_diagonal(g, K, kappa, fixed, 0, diag, S(stream));
    VFEM_CATCH
}

int vfem_thermal_source(int dim, const int64_t *nelems_host, const double *h_host, const double *q, const uint8_t *fixed,
                        const double *f_in, double *f_out, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_source";
    if (!h_host) throw Error(w + ": null argument");
    const ModalGrid g = thermal_setup(w, dim, nelems_host, h_host);
    if (!f_out) throw Error(w + ": null argument");
    if (!q && !f_in) throw Error(w + ": null argument: neither a volumetric nor a nodal source");
    if (f_in && f_in != f_out && overlaps(f_out, g.nnode, f_in, g.nnode)) throw Error(w + ": f_out overlaps f_in without being f_in");
    check_output(w, "f_out", g, f_out, g.nnode, q, fixed);
    launch_thermal_source(g, q, fixed, f_in, f_out, S(stream));
    VFEM_CATCH
}

int vfem_thermal_band_assemble(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                               double *band, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_band_assemble";
    const ModalGrid g = thermal_setup(w, dim, nelems_host, nullptr);
    const ThermalMatrix K = thermal_matrix(w, dim, Kc0_host);
    if (!kappa || !band) throw Error(w + ": null argument");
    long long n, hw;
    thermal_band_geometry(g, n, hw);
    check_output(w, "band", g, band, band_spd_doubles(n, hw), kappa, fixed);
    launch_thermal_band_assemble(g, K, kappa, fixed, band, S(stream));
    VFEM_CATCH
}

int vfem_thermal_pcg(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                     const double *b, double *x, double tol, int max_iter, int *iterations_out_host, double *relres_out_host,
                     void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermal_pcg";
    hipStream_t s = S(stream);
    const ModalGrid g = thermal_setup(w, dim, nelems_host, nullptr);
    const ThermalMatrix K = thermal_matrix(w, dim, Kc0_host);
    if (!kappa || !b || !x || !iterations_out_host || !relres_out_host) throw Error(w + ": null argument");
    if (!(tol > 0.0) || !std::isfinite(tol) || max_iter < 1) throw Error(w + ": tol must be positive and max_iter at least 1");
    const long long n = g.nnode;
    if (overlaps(x, n, b, n)) throw Error(w + ": x aliases b");
    check_output(w, "x", g, x, n, kappa, fixed);
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
    const ModalGrid grid = thermal_setup(w, dim, nelems_host, nullptr);
    check_columns(w, ncols);
    const ThermalMatrix K = thermal_matrix(w, dim, Kc0_host);
    if (!c_host || !dkappa || !A || !B || !g) throw Error(w + ": null argument");
    ThermalCoef c{};
    for (int i = 0; i < ncols; ++i) {
        if (!std::isfinite(c_host[i])) throw Error(w + ": the coefficients are not finite");
        c.c[i] = c_host[i];
    }
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
    if (!h_host) throw Error(w + ": null argument");
    const ModalGrid g = thermal_setup(w, dim, nelems_host, h_host);
    if (!k_host || !kappa || !T || !flux) throw Error(w + ": null argument");
    ThermalTensor k{};
    for (int i = 0; i < dim * dim; ++i) {
        if (!std::isfinite(k_host[i])) throw Error(w + ": the conductivity tensor is not finite");
        k.k[i] = k_host[i];
    }
    if (overlaps(flux, g.nelem * dim, T, g.nnode) || overlaps(flux, g.nelem * dim, kappa, g.nelem)) throw Error(w + ": flux aliases an input");
    launch_thermal_flux(g, k, kappa, T, flux, S(stream));
    VFEM_CATCH
}

}  // extern "C"
