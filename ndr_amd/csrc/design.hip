// The design-update entry points of include/vfem.h: box filters, projection, optimality-criteria candidate, LangelaarFilter, mean.
#include "vfem_host.h"

#include <algorithm>

using namespace vfem;

static void check_langelaar(const int64_t n[3], double eps, double p, double q) {
    for (int d = 0; d < 3; ++d)
        if (n[d] < 1 || n[d] > (1 << 30)) throw Error("invalid grid dimensions");
    if (n[0] * n[1] > (int64_t) 1 << 31) throw Error("grid too large");
    if (!(eps > 0) || !(p > 1) || !(q > 0)) throw Error("LangelaarFilter needs eps > 0, p > 1, q > 0");
}

extern "C" {

int vfem_box_filter(const int64_t n[3], int radius, const double *in, double *out, int transpose, void *stream) {
    VFEM_TRY
    if (radius < 0) throw Error("negative filter radius");
    launch_box_filter((int) n[0], (int) n[1], (int) n[2], radius, in, out, transpose, S(stream));
    VFEM_CATCH
}
int vfem_box_filter_slab(const int64_t n_local[3], int64_t x_first, int64_t nx_global, int64_t out_first, int64_t out_layers,
                         int radius, const double *in, double *out, int transpose, void *stream) {
    VFEM_TRY
    if (radius < 0) throw Error("negative filter radius");
    for (int d = 0; d < 3; ++d)
        if (n_local[d] < 1 || n_local[d] > (1 << 30)) throw Error("vfem_box_filter_slab: invalid slab dimensions");
    if (nx_global > (1 << 30) || x_first < 0 || x_first + n_local[0] > nx_global)
        throw Error("vfem_box_filter_slab: the local layers do not lie in the global grid");
    if (out_first < 0 || out_layers < 0 || out_first + out_layers > n_local[0])
        throw Error("vfem_box_filter_slab: the output layers do not lie in the local layers");
    if (radius > (1 << 30)) throw Error("vfem_box_filter_slab: radius too large");
    auto width = [&](int64_t n) { return std::min<int64_t>(2 * (int64_t) radius + 1, n); };
    if (width(nx_global) * width(n_local[1]) * width(n_local[2]) > INT32_MAX)
        throw Error("vfem_box_filter_slab: neighbourhood too large");
    if (out_layers == 0) return 0;
    // every neighbour layer of a written layer that lies in the global grid must lie in the local layers
    const int64_t g0 = x_first + out_first, g1 = g0 + out_layers - 1;
    if (std::max<int64_t>(g0 - radius, 0) < x_first || std::min<int64_t>(g1 + radius, nx_global - 1) > x_first + n_local[0] - 1)
        throw Error("vfem_box_filter_slab: the neighbourhood of a written layer leaves the local layers (too few ghost layers)");
    launch_box_filter_slab((int) n_local[0], (int) n_local[1], (int) n_local[2], (int) x_first, (int) nx_global, (int) out_first,
                           (int) out_layers, radius, in, out, transpose, S(stream));
    VFEM_CATCH
}
int vfem_box_filter_periodic(const int64_t n[3], int radius, const double *in, double *out, void *stream) {
    VFEM_TRY
    if (radius < 0) throw Error("negative filter radius");
    if (!n || !in || !out || in == out) throw Error("vfem_box_filter_periodic: in and out must be two arrays");
    for (int d = 0; d < 3; ++d)
        if (n[d] < 1 || n[d] > (1 << 30)) throw Error("vfem_box_filter_periodic: invalid grid dimensions");
    if (radius > (1 << 30)) throw Error("vfem_box_filter_periodic: radius too large");
    // every offset counts, also past the grid's extent: the window is not clipped to it
    int64_t offsets = 1;
    for (int d = 0; d < 3; ++d) {
        if (n[d] > 1) offsets *= 2 * (int64_t) radius + 1;
        if (offsets > INT32_MAX) throw Error("vfem_box_filter_periodic: neighbourhood too large");
    }
    launch_box_filter_periodic((int) n[0], (int) n[1], (int) n[2], radius, in, out, S(stream));
    VFEM_CATCH
}
int vfem_projection(int64_t n, double beta, const double *x, double *out, void *stream) {
    VFEM_TRY
    if (!(beta > 0)) throw Error("Beta parameter has to be positive (received beta = " + std::to_string(beta) + ")");
    launch_projection(n, beta, x, nullptr, out, 0, S(stream));
    VFEM_CATCH
}
int vfem_projection_backprop(int64_t n, double beta, const double *g, const double *vars, double *out, void *stream) {
    VFEM_TRY launch_projection(n, beta, vars, g, out, 1, S(stream)); VFEM_CATCH
}
int vfem_oc_candidate(int64_t n, const double *x0, const double *dJ, const double *dc, double lambda, double move, double *out,
                      void *stream) {
    VFEM_TRY launch_oc_candidate(n, x0, dJ, dc, lambda, move, out, S(stream)); VFEM_CATCH
}
int vfem_langelaar_apply(const int64_t n[3], double eps, double p, double q, const double *in, double *out, double *smax,
                         void *stream) {
    VFEM_TRY
    check_langelaar(n, eps, p, q);
    launch_langelaar_apply((int) n[0], (int) n[1], (int) n[2], eps, p, q, in, out, smax, S(stream));
    VFEM_CATCH
}
int vfem_langelaar_backprop(const int64_t n[3], double eps, double p, double q, const double *g, const double *vars,
                            const double *out, const double *smax, double *work, double *grad, void *stream) {
    VFEM_TRY
    check_langelaar(n, eps, p, q);
    launch_langelaar_backprop((int) n[0], (int) n[1], (int) n[2], eps, p, q, g, vars, out, smax, work, grad, S(stream));
    VFEM_CATCH
}
int vfem_mean(int64_t n, const double *x, double *mean_host, void *stream) {
    VFEM_TRY
    // the mean of nothing is undefined (the reference's Eigen mean() gives 0/0 = NaN, which would end the OC bisection on a
    // meaningless multiplier without a word): refuse it
    if (n < 1) throw Error("vfem_mean: empty vector");
    DevBuf<double> tmp; tmp.alloc(2048 + 8);
    launch_sum(n, x, tmp.p + 8, tmp.p, S(stream));
    double v = 0.0;
    VFEM_HIP(hipMemcpyAsync(&v, tmp.p, sizeof(double), hipMemcpyDeviceToHost, S(stream)));
    VFEM_HIP(hipStreamSynchronize(S(stream)));
    *mean_host = v / (double) n;
    VFEM_CATCH
}

}  // extern "C"
