// The part of the extern "C" boundary (include/vfem.h) that belongs to no subsystem: last error, version, section timers, device /
// memory / stream plumbing and the stand-alone dense and band factorisations.  The subsystems have a file each: sim.hip (trilinear
// simulator), mg.hip (its multigrid hierarchy), mg_slab.hip (the slab-decomposed solve), design.hip (design-update entry points),
// mlp.hip (neural density field), generic.hip (simulators and hierarchies of any dimension and degree).
#include "vfem_host.h"

#include <cstring>
#include <map>
#include <mutex>

namespace vfem {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }

struct TimerEntry { double seconds = 0.0; long long calls = 0; };
static std::map<std::string, TimerEntry> g_timers;
static std::mutex g_timer_mu;
void timer_add(const char *name, double seconds) {
    std::lock_guard<std::mutex> lk(g_timer_mu);
    auto &e = g_timers[name];
    e.seconds += seconds; e.calls += 1;
}
}  // namespace vfem

using namespace vfem;

extern "C" {

const char *vfem_last_error(void) { return vfem::g_err.c_str(); }
int vfem_version(void) { return 101; }
#ifdef VFEM_ABLATION
// timing ablations with WRONG results (tools/ only): exists in `make ablation` builds of the library, never in the shipped one
int vfem_debug_set(int key, int value) {
    if (key == 1) vfem::g_ablate_apply = value;
    else if (key == 3) vfem::g_ablate_store = value;
    else if (key == 8) vfem::g_ablate_mlp = value;
    else return 1;
    return 0;
}
#endif

int vfem_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
int vfem_set_device(int device) { VFEM_TRY VFEM_HIP(hipSetDevice(device)); VFEM_CATCH }

int vfem_malloc(void **ptr, size_t bytes) { VFEM_TRY VFEM_HIP(hipMalloc(ptr, bytes)); VFEM_CATCH }
int vfem_free(void *ptr) { VFEM_TRY VFEM_HIP(hipFree(ptr)); VFEM_CATCH }
int vfem_copy_h2d(void *dst, const void *src, size_t bytes, void *stream) {
    VFEM_TRY
    VFEM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream)));
    VFEM_HIP(hipStreamSynchronize(S(stream)));
    VFEM_CATCH
}
int vfem_copy_d2h(void *dst, const void *src, size_t bytes, void *stream) {
    VFEM_TRY
    VFEM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream)));
    VFEM_HIP(hipStreamSynchronize(S(stream)));
    VFEM_CATCH
}
int vfem_copy_d2d(void *dst, const void *src, size_t bytes, void *stream) {
    VFEM_TRY VFEM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, S(stream))); VFEM_CATCH
}
int vfem_memset(void *dst, int value, size_t bytes, void *stream) {
    VFEM_TRY VFEM_HIP(hipMemsetAsync(dst, value, bytes, S(stream))); VFEM_CATCH
}
int vfem_stream_sync(void *stream) { VFEM_TRY VFEM_HIP(hipStreamSynchronize(S(stream))); VFEM_CATCH }

int vfem_dense_spd_inverse(int64_t n, double *A, void *stream) {
    VFEM_TRY
    if (n < 1 || n > DENSE_COARSEST_MAX_DOFS) throw Error("dense inverse: n must be in [1, " + std::to_string(DENSE_COARSEST_MAX_DOFS) + "]");
    DenseWork w;
    dense_spd_inverse(n, A, w, S(stream));
    VFEM_HIP(hipStreamSynchronize(S(stream)));      // the workspace is released on return
    VFEM_CATCH
}
int vfem_band_spd_factor(int64_t n, int64_t w, double *band, void *stream) {
    VFEM_TRY
    if (n < 1 || w < 0 || w >= n) throw Error("band factorisation: n >= 1 and 0 <= w < n required");
    DevBuf<int> info;
    info.alloc(1);
    launch_band_clean(n, w, band, S(stream));
    band_spd_factor(n, w, band, info.p, S(stream), "band matrix");
    VFEM_CATCH
}
int vfem_band_spd_solve(int64_t n, int64_t w, const double *factor, double *x, int64_t nrhs, void *stream) {
    VFEM_TRY
    if (n < 1 || w < 0 || w >= n || nrhs < 0) throw Error("band solve: n >= 1, 0 <= w < n and nrhs >= 0 required");
    band_spd_solve(n, w, factor, x, nrhs, S(stream));
    VFEM_CATCH
}

int vfem_timers_reset(void) {
    std::lock_guard<std::mutex> lk(vfem::g_timer_mu);
    vfem::g_timers.clear();
    return 0;
}
int vfem_timers_report(char *buf, size_t len) {
    std::lock_guard<std::mutex> lk(vfem::g_timer_mu);
    std::string out;
    for (auto &kv : vfem::g_timers) {
        char line[256];
        std::snprintf(line, sizeof(line), "%s\t%.6f\t%lld\n", kv.first.c_str(), kv.second.seconds, kv.second.calls);
        out += line;
    }
    if (len == 0) return 0;
    std::strncpy(buf, out.c_str(), len - 1);
    buf[len - 1] = 0;
    return 0;
}

}  // extern "C"
