// The thermo-elastic entry points of include/vfem.h (vfem_thermoelastic_*).  Handle-free: every call takes the grid and
// the voxel's edge lengths.  Every argument is checked before the first device call.
#include "grid_args.h"
#include "thermoelastic.h"
#include "vfem_host.h"

#include <vector>

using namespace vfem;

namespace {

// the coupling matrices of ncases cases on the device, uploaded on the stream
void upload_matrices(DevBuf<double> &table, const double *G_host, size_t n, hipStream_t s) {
    table.alloc(n);
    VFEM_HIP(hipMemcpyAsync(table.p, G_host, n * sizeof(double), hipMemcpyHostToDevice, s));
}

}  // namespace

extern "C" {

int vfem_thermoelastic_load(int dim, const int64_t *nelems_host, const double *h_host, const double *G_host, double T_ref,
                            const double *E, const double *T, const uint8_t *mask, const double *f_in, double *f_out, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermoelastic_load";
    const ModalGrid g = grid_args(w, dim, nelems_host, h_host, true);
    if (!G_host || !E || !T || !f_out) throw Error(w + ": null argument");
    const int npe = 1 << g.N, ke = g.N * npe;
    check_finite(w, "the coupling matrix is", G_host, ke * npe);
    check_finite(w, "the reference temperature is", &T_ref, 1);
    const int64_t one = g.nnode * g.N;
    if (f_in && f_in != f_out && overlaps(f_out, one, f_in, one)) throw Error(w + ": f_out overlaps f_in without being f_in");
    if (overlaps(f_out, one, T, g.nnode)) throw Error(w + ": f_out aliases the temperatures");
    check_output(w, "f_out", f_out, one, g, E, "the multipliers", mask, "the mask");
    TeMatrix M{};
    for (int k = 0; k < ke * npe; ++k) M.G[k] = G_host[k];
    launch_te_load(g, M, T_ref, E, T, mask, f_in, f_out, S(stream));
    VFEM_CATCH
}

int vfem_thermoelastic_adjoint_source(int dim, const int64_t *nelems_host, const double *h_host, int ncases, const double *a_host,
                                      const double *G_host, const double *E, const double *U, const uint8_t *fixed, double *q,
                                      void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermoelastic_adjoint_source";
    hipStream_t s = S(stream);
    const ModalGrid g = grid_args(w, dim, nelems_host, h_host, true);
    check_count(w, "ncases", ncases, TE_MAX_CASES);
    if (!a_host || !G_host || !E || !U || !q) throw Error(w + ": null argument");
    const int npe = 1 << g.N, ke = g.N * npe;
    check_finite(w, "the coefficients are", a_host, ncases);
    check_finite(w, "the coupling matrices are", G_host, ncases * ke * npe);
    if (overlaps(q, g.nnode, U, ncases * g.nnode * g.N)) throw Error(w + ": q aliases the displacements");
    check_output(w, "q", q, g.nnode, g, E, "the multipliers", fixed, "the mask");
    TeCoef c{};
    for (int i = 0; i < ncases; ++i) c.a[i] = a_host[i];
    DevBuf<double> table;
    upload_matrices(table, G_host, (size_t) ncases * ke * npe, s);
    launch_te_adjoint_source(g, ncases, table.p, c, E, U, fixed, q, s);
    VFEM_HIP(hipStreamSynchronize(s));          // the table is freed on return
    VFEM_CATCH
}

int vfem_thermoelastic_gradient(int dim, const int64_t *nelems_host, const double *h_host, int ncases, const double *a_host,
                                const double *G_host, const double *Tref_host, const double *dE, const double *T, const double *U,
                                const double *g_in, double *g_out, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_thermoelastic_gradient";
    hipStream_t s = S(stream);
    const ModalGrid g = grid_args(w, dim, nelems_host, h_host, true);
    check_count(w, "ncases", ncases, TE_MAX_CASES);
    if (!a_host || !G_host || !Tref_host || !dE || !T || !U || !g_out) throw Error(w + ": null argument");
    const int npe = 1 << g.N, ke = g.N * npe;
    check_finite(w, "the coefficients are", a_host, ncases);
    check_finite(w, "the coupling matrices are", G_host, ncases * ke * npe);
    check_finite(w, "the reference temperatures are", Tref_host, ncases);
    if (g_in && g_in != g_out && overlaps(g_out, g.nelem, g_in, g.nelem)) throw Error(w + ": g_out overlaps g_in without being g_in");
    if (overlaps(g_out, g.nelem, U, ncases * g.nnode * g.N) || overlaps(g_out, g.nelem, T, g.nnode) ||
        overlaps(g_out, g.nelem, dE, g.nelem))
        throw Error(w + ": g_out aliases an input");
    TeCoef c{};
    for (int i = 0; i < ncases; ++i) {
        c.a[i] = a_host[i];
        c.tref[i] = Tref_host[i];
    }
    DevBuf<double> table;
    upload_matrices(table, G_host, (size_t) ncases * ke * npe, s);
    launch_te_gradient(g, ncases, table.p, c, dE, T, U, g_in, g_out, s);
    VFEM_HIP(hipStreamSynchronize(s));          // the table is freed on return
    VFEM_CATCH
}

}  // extern "C"
