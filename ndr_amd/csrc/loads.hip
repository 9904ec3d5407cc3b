// The load-case entry points of include/vfem.h (vfem_loads_*).  Handle-free: every call takes the grid and the voxel's
// edge lengths.  Every argument is checked before the first device call.
#include "grid_args.h"
#include "loads.h"
#include "vfem_host.h"

#include <vector>

using namespace vfem;

extern "C" {

int vfem_loads_assemble(int dim, const int64_t *nelems_host, const double *h_host, const double *Lb_host, const double *Lt_host,
                        const double *m, const double *E, const uint8_t *mask, const double *f_in, double *f_out, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_loads_assemble";
    const ModalGrid g = grid_args(w, dim, nelems_host, h_host, true);
    if (!f_out) throw Error(w + ": null argument");
    if (!Lb_host && !Lt_host) throw Error(w + ": null argument: neither a body-force nor an eigenstrain pattern");
    if ((Lb_host == nullptr) != (m == nullptr)) throw Error(w + ": the body-force pattern and its multipliers m go together");
    if ((Lt_host == nullptr) != (E == nullptr)) throw Error(w + ": the eigenstrain pattern and its multipliers E go together");
    const int ke = g.N * (1 << g.N);
    LoadPatterns p{};
    if (Lb_host) {
        check_finite(w, "the body-force pattern is", Lb_host, ke);
        for (int k = 0; k < ke; ++k) p.Lb[k] = Lb_host[k];
    }
    if (Lt_host) {
        check_finite(w, "the eigenstrain pattern is", Lt_host, ke);
        for (int k = 0; k < ke; ++k) p.Lt[k] = Lt_host[k];
    }
    const int64_t one = g.nnode * g.N;
    if (f_in && f_in != f_out && overlaps(f_out, one, f_in, one)) throw Error(w + ": f_out overlaps f_in without being f_in");
    if ((m && overlaps(f_out, one, m, g.nelem)) || (E && overlaps(f_out, one, E, g.nelem)))
        throw Error(w + ": f_out aliases the multipliers");
    if (mask && overlaps_bytes(f_out, one * (int64_t) sizeof(double), mask, g.nnode)) throw Error(w + ": f_out aliases the mask");
    launch_loads_assemble(g, p, m, E, mask, f_in, f_out, S(stream));
    VFEM_CATCH
}

int vfem_loads_gradient(int dim, const int64_t *nelems_host, const double *h_host, int ncases, const double *K0_host,
                        const double *cK_host, const double *cB_host, const double *cT_host, const double *Lb_host,
                        const double *Lt_host, const double *dE, const double *dm, const double *U, double *g, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_loads_gradient";
    hipStream_t s = S(stream);
    const ModalGrid grid = grid_args(w, dim, nelems_host, h_host, true);
    check_count(w, "ncases", ncases, LOADS_MAX_CASES);
    if (!K0_host || !cK_host || !dE || !U || !g) throw Error(w + ": null argument");
    if ((Lb_host == nullptr) != (cB_host == nullptr) || (Lb_host == nullptr) != (dm == nullptr))
        throw Error(w + ": the body-force patterns, their coefficients and dm go together");
    if ((Lt_host == nullptr) != (cT_host == nullptr)) throw Error(w + ": the eigenstrain patterns and their coefficients go together");
    const int ke = grid.N * (1 << grid.N);
    check_finite(w, "the element matrix is", K0_host, ke * ke);
    check_finite(w, "the coefficients are", cK_host, ncases);
    if (Lb_host) {
        check_finite(w, "the coefficients are", cB_host, ncases);
        check_finite(w, "the body-force patterns are", Lb_host, ncases * ke);
    }
    if (Lt_host) {
        check_finite(w, "the coefficients are", cT_host, ncases);
        check_finite(w, "the eigenstrain patterns are", Lt_host, ncases * ke);
    }
    LoadCoef c{};
    for (int i = 0; i < ncases; ++i) {
        c.cK[i] = cK_host[i];
        c.cB[i] = cB_host ? cB_host[i] : 0.0;
        c.cT[i] = cT_host ? cT_host[i] : 0.0;
    }
    const int64_t one = grid.nnode * grid.N;
    if (overlaps(g, grid.nelem, U, ncases * one) || overlaps(g, grid.nelem, dE, grid.nelem) ||
        (dm && overlaps(g, grid.nelem, dm, grid.nelem)))
        throw Error(w + ": g aliases an input");
    // one table: K0, then the patterns
    const size_t nK = (size_t) ke * ke, nP = (size_t) ncases * ke;
    std::vector<double> table(nK + 2 * nP, 0.0);
    for (size_t i = 0; i < nK; ++i) table[i] = K0_host[i];
    for (size_t i = 0; i < nP; ++i) {
        if (Lb_host) table[nK + i] = Lb_host[i];
        if (Lt_host) table[nK + nP + i] = Lt_host[i];
    }
    DevBuf<double> T;
    T.alloc(table.size());
    VFEM_HIP(hipMemcpyAsync(T.p, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, s));
    launch_loads_gradient(grid, ncases, T.p, Lb_host ? T.p + nK : nullptr, Lt_host ? T.p + nK + nP : nullptr, c, dE, dm, U, g, s);
    VFEM_HIP(hipStreamSynchronize(s));          // the table is freed on return
    VFEM_CATCH
}

}  // extern "C"
