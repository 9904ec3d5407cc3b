// CoarsestSolver (vfem_internal.h): what the trilinear hierarchy (mg.hip) and the generic ones (generic.hip) do with their coarsest
// operator once it is assembled.  Host code only: the factorisations are dense_spd.hip and plane_spd.hip, the finish and the GEMV
// kernels_mg.hip.
#include "vfem_host.h"

namespace vfem {

bool CoarsestSolver::set_mode(int m) {
    if (m != VFEM_COARSEST_AUTO && m != VFEM_COARSEST_DENSE && m != VFEM_COARSEST_PLANES)
        throw Error("unknown coarsest-level solver mode " + std::to_string(m));
    const bool changed = m != mode;
    mode = m;
    return changed;
}

void CoarsestSolver::refuse_if_too_large(long long dofs, const Dims *plane_grid) const {
    if (plane_grid ? plane_spd_bytes_needed(*plane_grid) > PLANE_SPD_MAX_BYTES : dofs > DENSE_COARSEST_MAX_DOFS)
        throw Error("coarsest grid too large for the " + std::string(plane_grid ? "plane-block" : "dense") + " coarsest-level solve (" +
                    std::to_string(dofs) + " dofs); use more coarsening levels");
}

double *CoarsestSolver::dense_matrix(long long dofs, hipStream_t s) {
    planes.release();
    held = NONE;
    n = dofs;
    Ainv.alloc((size_t) n * n);
    Ainv.zero(s);
    return Ainv.p;
}

void CoarsestSolver::factor_dense(int N, const uint8_t *mask, hipStream_t s) {
    dense_spd_inverse(n, Ainv.p, work, s);      // own kernels, fixed summation order (dense_spd.hip)
    // three further n x n work matrices: kept between operator updates while they are small (2 187 dofs: 115 MB), released when the
    // coarsest level is large -- they would otherwise be held for the hierarchy's lifetime at three times the inverse's size
    if ((size_t) n * (size_t) n * sizeof(double) > ((size_t) 256 << 20)) {
        VFEM_HIP(hipStreamSynchronize(s));
        work.L.release(); work.X.release(); work.Tm.release();
    }
    launch_dense_finish_inverse(n, N, mask, Ainv.p, s);
    held = DENSE;
}

void CoarsestSolver::factor_planes(const Dims &d, const double *S, const uint8_t *mask, hipStream_t s) {
    Ainv.release();
    held = NONE;
    plane_spd_factor(planes, d, S, mask, work, s);
    held = PLANES;
    n = 3 * d.nn;
}

void CoarsestSolver::solve(const double *b, double *x, hipStream_t s) {
    if (held == PLANES) plane_spd_solve(planes, b, x, s);
    else if (held == DENSE) launch_gemv_sym(n, Ainv.p, b, x, s);
    else throw Error("coarsest grid too large for the dense coarsest-level solve; use more coarsening levels");
}

}  // namespace vfem
