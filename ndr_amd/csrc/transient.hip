// The transient heat-conduction entry point of include/vfem.h that is the transient problem's alone: the density
// gradient summed over a march.  The operator calls of a step (vfem_transient_{apply, diagonal, band_assemble, pcg}) are the two-term
// forms of the steady ones and live beside them in thermal.hip, vfem_transient_mg_create beside its twin in thermal_mg.hip.
// Handle-free; every argument is checked before the first device call.
#include "grid_args.h"
#include "transient.h"
#include "vfem_host.h"

using namespace vfem;

extern "C" {

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
    const ThermalCapacity m = thermal_capacity_entries(w, dim, m_host);
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
