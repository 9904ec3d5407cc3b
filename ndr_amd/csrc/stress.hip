// The element-stress entry points of include/vfem.h (vfem_stress_*).  Handle-free: every call takes the grid, the voxel's
// edge lengths and the flattened tensor.  Every argument is checked before the first device call.
#include "grid_args.h"
#include "stress.h"
#include "vfem_host.h"

using namespace vfem;

namespace {

StressProblem stress_setup(const char *who, int dim, const int64_t *nelems, const double *h, const double *D) {
    const ModalGrid g = grid_and_tensor_args(who, dim, nelems, h, D);
    StressProblem p;
    p.N = dim;
    p.S = dim == 2 ? 3 : 6;
    for (int d = 0; d < 3; ++d) {
        p.ne[d] = g.ne[d];
        p.gs[d] = d < dim ? 1.0 / (g.h[d] * (double) (1 << (dim - 1))) : 0.0;
    }
    p.nelem = g.nelem;
    p.nnode = g.nnode;
    for (int q = 0; q < p.S; ++q)
        for (int r = 0; r < p.S; ++r) p.Dm[q * p.S + r] = D[q * p.S + r] * (r < dim ? 1.0 : 2.0);
    for (int i = p.S * p.S; i < 36; ++i) p.Dm[i] = 0.0;
    return p;
}

void check_exponent(const char *who, double P) {
    if (!std::isfinite(P) || P < 1.0) throw Error(std::string(who) + ": the exponent P must be finite and at least 1");
}

void check_measure(const char *who, double J) {
    if (!(J >= 0.0) || !std::isfinite(J)) throw Error(std::string(who) + ": the measure J must be finite and not negative");
}

}  // namespace

extern "C" {

int vfem_stress_fields(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *m,
                       const double *u, double *strain, double *stress, double *vm, void *stream) {
    VFEM_TRY
    const StressProblem p = stress_setup("vfem_stress_fields", dim, nelems_host, h_host, D_host);
    if (!u) throw Error("vfem_stress_fields: null argument");
    if (!strain && !stress && !vm) throw Error("vfem_stress_fields: no output requested");
    if ((stress || vm) && !m) throw Error("vfem_stress_fields: stresses need the element multipliers");
    launch_stress_fields(p, m, u, strain, stress, vm, S(stream));
    VFEM_CATCH
}

int vfem_stress_pnorm(int64_t n, const double *vm, double P, double *J_host, double *vmax_host, void *stream) {
    VFEM_TRY
    hipStream_t s = S(stream);
    if (n < 1) throw Error("vfem_stress_pnorm: n must be at least 1");
    if (!vm || !J_host) throw Error("vfem_stress_pnorm: null argument");
    check_exponent("vfem_stress_pnorm", P);
    DevBuf<double> work;
    work.alloc(STRESS_REDUCE_BLOCKS + 2);
    launch_stress_pnorm(n, vm, P, work.p + 2, work.p, s);
    double out[2];
    VFEM_HIP(hipMemcpyAsync(out, work.p, sizeof out, hipMemcpyDeviceToHost, s));
    VFEM_HIP(hipStreamSynchronize(s));
    *J_host = out[0];
    if (vmax_host) *vmax_host = out[1];
    VFEM_CATCH
}

int vfem_stress_adjoint_load(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *m,
                             const double *u, double J, double P, const uint8_t *mask, double *work, double *a, void *stream) {
    VFEM_TRY
    const StressProblem p = stress_setup("vfem_stress_adjoint_load", dim, nelems_host, h_host, D_host);
    if (!m || !u || !work || !a) throw Error("vfem_stress_adjoint_load: null argument");
    check_exponent("vfem_stress_adjoint_load", P);
    check_measure("vfem_stress_adjoint_load", J);
    if (J == 0.0) VFEM_HIP(hipMemsetAsync(a, 0, (size_t) p.nnode * p.N * sizeof(double), S(stream)));     // no stress anywhere: dv = 0
    else launch_stress_adjoint_load(p, m, u, J, P, mask, work, a, S(stream));
    VFEM_CATCH
}

int vfem_stress_pnorm_gradient(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *K0_host,
                               const double *m, const double *dm, const double *dE, const double *u, const double *lambda, double J,
                               double P, double *g, void *stream) {
    VFEM_TRY
    hipStream_t s = S(stream);
    const StressProblem p = stress_setup("vfem_stress_pnorm_gradient", dim, nelems_host, h_host, D_host);
    if (!K0_host || !m || !dm || !dE || !u || !lambda || !g) throw Error("vfem_stress_pnorm_gradient: null argument");
    check_exponent("vfem_stress_pnorm_gradient", P);
    check_measure("vfem_stress_pnorm_gradient", J);
    const int ke = p.N * (1 << p.N);
    check_finite("vfem_stress_pnorm_gradient", "the element matrix is", K0_host, ke * ke);
    if (J == 0.0) {
        VFEM_HIP(hipMemsetAsync(g, 0, (size_t) p.nelem * sizeof(double), s));
    } else {
        DevBuf<double> K0;
        K0.alloc((size_t) ke * ke);
        VFEM_HIP(hipMemcpyAsync(K0.p, K0_host, (size_t) ke * ke * sizeof(double), hipMemcpyHostToDevice, s));
        launch_stress_gradient(p, K0.p, m, dm, dE, u, lambda, J, P, g, s);
        VFEM_HIP(hipStreamSynchronize(s));          // the table is freed on return
    }
    VFEM_CATCH
}

}  // extern "C"
