// The linearised-buckling entry points of include/vfem.h (vfem_buckling_*).  Handle-free: every call takes the grid, the
// voxel's edge lengths and the flattened tensor.  Every argument is checked before the first device call.
#include "buckling.h"
#include "grid_args.h"
#include "vfem_host.h"

#include <cmath>
#include <list>
#include <mutex>
#include <vector>

using namespace vfem;

namespace {

// T[j][n][m] = int_e grad N_n^T (C : B_j(x)) grad N_m dV by 2 Gauss points per axis (exact: degree <= 3 per axis); D is the
// flattened tensor of ndr_amd.materials (xx yy xy / xx yy zz yz xz xy, TENSOR components: the shear strains count twice).
// Entry (m, n) is a copy of (n, m): the kernels read either.
std::vector<double> geometric_table(int N, const double *h, const double *D) {
    static const int pairs2[3][2] = {{0, 0}, {1, 1}, {0, 1}};
    static const int pairs3[6][2] = {{0, 0}, {1, 1}, {2, 2}, {1, 2}, {0, 2}, {0, 1}};
    const int (*pairs)[2] = N == 2 ? pairs2 : pairs3;
    const int S = N == 2 ? 3 : 6, npe = 1 << N, ke = N * npe;
    const double gauss[2] = {0.5 - 0.5 / std::sqrt(3.0), 0.5 + 0.5 / std::sqrt(3.0)};
    double wgt = 1.0;
    for (int d = 0; d < N; ++d) wgt *= 0.5 * h[d];
    std::vector<double> T((size_t) ke * npe * npe, 0.0);
    for (int q = 0; q < npe; ++q) {
        double x[3], grad[8][3];
        for (int d = 0; d < N; ++d) x[d] = gauss[(q >> (N - 1 - d)) & 1];
        for (int n = 0; n < npe; ++n)
            for (int d = 0; d < N; ++d) {
                double v = 1.0;
                for (int e = 0; e < N; ++e) {
                    const int bit = (n >> (N - 1 - e)) & 1;
                    v *= e == d ? (bit ? 1.0 : -1.0) / h[e] : (bit ? x[e] : 1.0 - x[e]);
                }
                grad[n][d] = v;
            }
        for (int j = 0; j < ke; ++j) {
            const int jn = j / N, a = j % N;
            double eps[6], sig[3][3];
            for (int r = 0; r < S; ++r) {
                const int p = pairs[r][0], t = pairs[r][1];
                eps[r] = p == t ? (p == a ? grad[jn][p] : 0.0) : 0.5 * ((p == a ? grad[jn][t] : 0.0) + (t == a ? grad[jn][p] : 0.0));
            }
            for (int r = 0; r < S; ++r) {
                double s = 0.0;
                for (int c = 0; c < S; ++c) s += D[r * S + c] * (pairs[c][0] == pairs[c][1] ? 1.0 : 2.0) * eps[c];
                sig[pairs[r][0]][pairs[r][1]] = sig[pairs[r][1]][pairs[r][0]] = s;
            }
            for (int n = 0; n < npe; ++n)
                for (int m = n; m < npe; ++m) {
                    double s = 0.0;
                    for (int p = 0; p < N; ++p)
                        for (int t = 0; t < N; ++t) s += grad[n][p] * sig[p][t] * grad[m][t];
                    T[((size_t) j * npe + n) * npe + m] += wgt * s;
                }
        }
    }
    for (int j = 0; j < ke; ++j)
        for (int n = 0; n < npe; ++n)
            for (int m = 0; m < n; ++m) T[((size_t) j * npe + n) * npe + m] = T[((size_t) j * npe + m) * npe + n];
    return T;
}

// The table on the device.  It depends on (device, dim, h, D) only, so it is formed and uploaded once per such key and kept for the
// life of the process: an eigensolve applies K_G a few times per iteration with the same key, and a table that outlives the launch
// needs no synchronisation after it.  A design loop holds one or two keys; past TABLE_CACHE_MAX the oldest is dropped (after a
// device synchronisation: a launch in flight may still read it).
constexpr size_t TABLE_CACHE_MAX = 8;

struct TableEntry {
    int device, N;
    double h[3], D[36];
    DevBuf<double> d;
};

const double *device_table(const ModalGrid &g, const double *D) {
    static std::mutex lock;
    static std::list<TableEntry> &cache = *new std::list<TableEntry>;        // never destroyed: no hipFree after the runtime has gone
    const int S = g.N == 2 ? 3 : 6;
    int device = 0;
    VFEM_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> hold(lock);
    for (const TableEntry &e : cache) {
        if (e.device != device || e.N != g.N) continue;
        bool same = true;
        for (int d = 0; d < g.N; ++d) same = same && e.h[d] == g.h[d];
        for (int i = 0; i < S * S; ++i) same = same && e.D[i] == D[i];
        if (same) return e.d.p;
    }
    if (cache.size() >= TABLE_CACHE_MAX) {
        VFEM_HIP(hipDeviceSynchronize());
        cache.pop_front();
    }
    const std::vector<double> T = geometric_table(g.N, g.h, D);
    cache.emplace_back();
    TableEntry &e = cache.back();
    e.device = device;
    e.N = g.N;
    for (int d = 0; d < 3; ++d) e.h[d] = d < g.N ? g.h[d] : 0.0;
    for (int i = 0; i < 36; ++i) e.D[i] = i < S * S ? D[i] : 0.0;
    try {
        e.d.alloc(T.size());
        VFEM_HIP(hipMemcpy(e.d.p, T.data(), T.size() * sizeof(double), hipMemcpyHostToDevice));      // blocking: T leaves scope here
    } catch (...) {
        cache.pop_back();
        throw;
    }
    return e.d.p;
}

}  // namespace

extern "C" {

int vfem_buckling_geom_apply(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *mG,
                             const double *u, const uint8_t *mask, int ncols, const double *X, double *Y, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_buckling_geom_apply";
    hipStream_t s = S(stream);
    const ModalGrid g = grid_and_tensor_args(w, dim, nelems_host, h_host, D_host);
    if (!mG || !u || !X || !Y) throw Error(w + ": null argument");
    check_count(w, "ncols", ncols, BLOCK_MAX_COLS);
    const int64_t one = g.nnode * g.N, len = (int64_t) ncols * one;
    if (overlaps(Y, len, X, len)) throw Error(w + ": Y aliases X");
    if (overlaps(Y, len, u, one)) throw Error(w + ": Y aliases u");
    check_output(w, "Y", Y, len, g, mG, "the multipliers", mask, "the mask");
    launch_buckling_geom_apply(g, device_table(g, D_host), mG, u, mask, ncols, X, Y, s);
    VFEM_CATCH
}

int vfem_buckling_adjoint_load(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *mG,
                               const uint8_t *mask, int nmodes, const double *c_host, const double *Phi, double *a, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_buckling_adjoint_load";
    hipStream_t s = S(stream);
    const ModalGrid g = grid_and_tensor_args(w, dim, nelems_host, h_host, D_host);
    if (!mG || !c_host || !Phi || !a) throw Error(w + ": null argument");
    check_count(w, "nmodes", nmodes, BUCKLING_MAX_MODES);
    check_finite(w, "the coefficients are", c_host, nmodes);
    BucklingCoef c{};
    for (int i = 0; i < nmodes; ++i) c.c[i] = c_host[i];
    const int64_t one = g.nnode * g.N;
    if (overlaps(a, one, Phi, nmodes * one)) throw Error(w + ": a aliases Phi");
    check_output(w, "a", a, one, g, mG, "the multipliers", mask, "the mask");
    launch_buckling_adjoint_load(g, device_table(g, D_host), mG, mask, nmodes, c, Phi, a, s);
    VFEM_CATCH
}

int vfem_buckling_gradient(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, int nmodes,
                           const double *K0_host, const double *cG_host, const double *cK_host, const double *dmG, const double *dE,
                           const double *u, const double *v, const double *Phi, double *g, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_buckling_gradient";
    hipStream_t s = S(stream);
    const ModalGrid grid = grid_and_tensor_args(w, dim, nelems_host, h_host, D_host);
    check_count(w, "nmodes", nmodes, BUCKLING_MAX_MODES);
    if (!K0_host || !cG_host || !cK_host || !dmG || !dE || !u || !v || !Phi || !g) throw Error(w + ": null argument");
    const int ke = grid.N * (1 << grid.N);
    check_finite(w, "the element matrix is", K0_host, ke * ke);
    check_finite(w, "the coefficients are", cG_host, nmodes);
    check_finite(w, "the coefficients are", cK_host, nmodes);
    BucklingCoef c{};
    for (int i = 0; i < nmodes; ++i) {
        c.c[i] = cG_host[i];
        c.cK[i] = cK_host[i];
    }
    const int64_t one = grid.nnode * grid.N;
    if (overlaps(g, grid.nelem, u, one) || overlaps(g, grid.nelem, v, one) || overlaps(g, grid.nelem, Phi, nmodes * one) ||
        overlaps(g, grid.nelem, dmG, grid.nelem) || overlaps(g, grid.nelem, dE, grid.nelem))
        throw Error(w + ": g aliases an input");
    DevBuf<double> K0;
    K0.alloc((size_t) ke * ke);
    VFEM_HIP(hipMemcpyAsync(K0.p, K0_host, (size_t) ke * ke * sizeof(double), hipMemcpyHostToDevice, s));
    launch_buckling_gradient(grid, device_table(grid, D_host), K0.p, nmodes, c, dmG, dE, u, v, Phi, g, s);
    VFEM_HIP(hipStreamSynchronize(s));          // K0 is freed on return
    VFEM_CATCH
}

}  // extern "C"
