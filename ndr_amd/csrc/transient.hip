// The transient heat-conduction entry points of include/vfem.h (vfem_transient_*).  Handle-free, as the steady ones
// (thermal.hip): every call takes the grid, the element matrix and the capacity entries with the scalars of the time scheme folded
// in by the caller.  Every argument is checked before the first device call.
#include "grid_args.h"
#include "transient.h"
#include "vfem_host.h"

using namespace vfem;

namespace {

constexpr int TRANSIENT_PCG_CHECK = 8;      // the host looks at the residual once every so many iterations, as vfem_thermal_pcg does

ThermalCapacity capacity_entries(const std::string &w, int dim, const double *m_host) {
    if (!m_host) throw Error(w + ": null argument");
    check_finite(w, "the capacity entries are", m_host, dim + 1);
    ThermalCapacity m{};
    for (int d = 0; d <= dim; ++d) m.m[d] = m_host[d];
    return m;
}

// what every operator call takes after the grid: the element matrix, the capacity entries and the two element fields
struct Operator {
    ModalGrid g;
    ThermalMatrix K;
    ThermalCapacity m;
};

Operator operator_args(const std::string &w, int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host,
                       const double *kappa, const double *cap) {
    Operator op;
    op.g = grid_args(w, dim, nelems_host, nullptr, false);
    op.K = thermal_element_matrix(w, dim, Ka_host);
    op.m = capacity_entries(w, dim, mb_host);
    if (!kappa || !cap) throw Error(w + ": null argument");
    return op;
}

// an output of `len` doubles against both element fields and the fixed-node bytes
void check_transient_output(const std::string &w, const char *name, const ModalGrid &g, const double *out, int64_t len, const double *kappa,
                            const double *cap, const uint8_t *fixed) {
    check_output(w, name, out, len, g, kappa, "the element conductivities", fixed, "the fixed-node mask");
    check_output(w, name, out, len, g, cap, "the element capacities", nullptr, "");
}

}  // namespace

extern "C" {

int vfem_transient_apply(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                         const double *cap, const uint8_t *fixed, int identity, int ncols, const double *X, const double *b, double *Y,
                         void *stream) {
    VFEM_TRY
    const std::string w = "vfem_transient_apply";
    const Operator op = operator_args(w, dim, nelems_host, Ka_host, mb_host, kappa, cap);
    if (!X || !Y) throw Error(w + ": null argument");
    if (identity != 0 && identity != 1) throw Error(w + ": identity must be 0 or 1");
    check_count(w, "ncols", ncols, THERMAL_MAX_COLS);
    const int64_t len = (int64_t) ncols * op.g.nnode;
    if (overlaps(Y, len, X, len)) throw Error(w + ": Y aliases X");
    if (b && overlaps(Y, len, b, len)) throw Error(w + ": Y aliases b");
    check_transient_output(w, "Y", op.g, Y, len, kappa, cap, fixed);
    launch_transient_apply(op.g, op.K, op.m, kappa, cap, fixed, identity, ncols, X, b, 0, Y, S(stream));
    VFEM_CATCH
}

int vfem_transient_diagonal(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                            const double *cap, const uint8_t *fixed, double *diag, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_transient_diagonal";
    const Operator op = operator_args(w, dim, nelems_host, Ka_host, mb_host, kappa, cap);
    if (!diag) throw Error(w + ": null argument");
    check_transient_output(w, "diag", op.g, diag, op.g.nnode, kappa, cap, fixed);
    launch_transient_diagonal(op.g, op.K, op.m, kappa, cap, fixed, 0, diag, S(stream));
    VFEM_CATCH
}

int vfem_transient_band_assemble(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                                 const double *cap, const uint8_t *fixed, double *band, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_transient_band_assemble";
    const Operator op = operator_args(w, dim, nelems_host, Ka_host, mb_host, kappa, cap);
    if (!band) throw Error(w + ": null argument");
    long long n, hw;
    thermal_band_geometry(op.g, n, hw);
    check_transient_output(w, "band", op.g, band, band_spd_doubles(n, hw), kappa, cap, fixed);
    launch_transient_band_assemble(op.g, op.K, op.m, kappa, cap, fixed, band, S(stream));
    VFEM_CATCH
}

int vfem_transient_pcg(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                       const double *cap, const uint8_t *fixed, const double *b, double *x, double tol, int max_iter,
                       int *iterations_out_host, double *relres_out_host, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_transient_pcg";
    hipStream_t s = S(stream);
    const Operator op = operator_args(w, dim, nelems_host, Ka_host, mb_host, kappa, cap);
    if (!b || !x || !iterations_out_host || !relres_out_host) throw Error(w + ": null argument");
    if (!(tol > 0.0) || !std::isfinite(tol) || max_iter < 1) throw Error(w + ": tol must be positive and max_iter at least 1");
    const long long n = op.g.nnode;
    if (overlaps(x, n, b, n)) throw Error(w + ": x aliases b");
    check_transient_output(w, "x", op.g, x, n, kappa, cap, fixed);
    DevBuf<double> dinv;
    dinv.alloc((size_t) n);
    launch_transient_diagonal(op.g, op.K, op.m, kappa, cap, fixed, 1, dinv.p, s);
    const ThermalPreconditioner jacobi = [&](const double *r, double *z) { launch_thermal_scale(n, dinv.p, r, z, s); };
    const ThermalApply apply = [&](const double *v, const double *rhs, double *out) {
        launch_transient_apply(op.g, op.K, op.m, kappa, cap, fixed, 1, 1, v, rhs, 1, out, s);
    };
    thermal_pcg(w, n, apply, "a free node whose incident elements all have zero conductivity and zero capacity", b, x, tol, max_iter,
                TRANSIENT_PCG_CHECK, jacobi, iterations_out_host, relres_out_host, s);
    VFEM_CATCH
}

int vfem_transient_gradient(int dim, const int64_t *nelems_host, int64_t steps, const double *Kc0_host, const double *m_host, double dt,
                            double theta, const double *dkappa, const double *dcap, const double *T, const double *Lam, double *g,
                            void *stream) {
    VFEM_TRY
    const std::string w = "vfem_transient_gradient";
    const ModalGrid grid = grid_args(w, dim, nelems_host, nullptr, false);
    if (steps < 1) throw Error(w + ": steps must be at least 1 (got " + std::to_string(steps) + ")");
    if (!(dt > 0.0) || !std::isfinite(dt)) throw Error(w + ": dt must be positive and finite");
    if (!(theta >= 0.5 && theta <= 1.0)) throw Error(w + ": theta must be in [0.5, 1]");
    const ThermalMatrix K = thermal_element_matrix(w, dim, Kc0_host);
    const ThermalCapacity m = capacity_entries(w, dim, m_host);
    if (!dkappa || !dcap || !T || !Lam || !g) throw Error(w + ": null argument");
    if (steps > (int64_t) ((1LL << 60) / grid.nnode)) throw Error(w + ": steps too large");
    const int64_t len = (steps + 1) * grid.nnode;
    if (overlaps(g, grid.nelem, T, len) || overlaps(g, grid.nelem, Lam, len) || overlaps(g, grid.nelem, dkappa, grid.nelem) ||
        overlaps(g, grid.nelem, dcap, grid.nelem))
        throw Error(w + ": g aliases an input");
    launch_transient_gradient(grid, K, m, steps, dt, theta, dkappa, dcap, T, Lam, g, S(stream));
    VFEM_CATCH
}

}  // extern "C"
