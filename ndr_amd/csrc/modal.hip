// The natural-frequency entry points of include/vfem.h (vfem_modal_*, vfem_block_*).  Handle-free: every grid call
// takes the grid and the voxel's edge lengths, the block calls a length.  Every argument is checked before the first device call.
#include "grid_args.h"
#include "vfem_host.h"

using namespace vfem;

namespace {

// stream-ordered scratch, as the MMA dual's is (mma.hip): taking and returning it does not synchronise the device
struct Scratch {
    double *p = nullptr;
    hipStream_t s;
    Scratch(size_t doubles, hipStream_t s_) : s(s_) { VFEM_HIP(hipMallocAsync((void **) &p, doubles * sizeof(double), s)); }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { if (p) (void) hipFreeAsync(p, s); }
};

}  // namespace

extern "C" {

int vfem_modal_mass_apply(int dim, const int64_t *nelems_host, const double *h_host, const double *m, const uint8_t *mask, int ncols,
                          const double *X, double *Y, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_modal_mass_apply";
    const ModalGrid g = grid_args(w, dim, nelems_host, h_host, true);
    if (!m || !X || !Y) throw Error(w + ": null argument");
    check_count(w, "ncols", ncols, BLOCK_MAX_COLS);
    const int64_t len = (int64_t) ncols * g.nnode * g.N;
    if (overlaps(Y, len, X, len)) throw Error(w + ": Y aliases X");
    launch_modal_mass_apply(g, m, mask, ncols, X, Y, S(stream));
    VFEM_CATCH
}

int vfem_modal_project(int dim, const int64_t *nelems_host, const double *h_host, const uint8_t *mask, int ncols, double *X,
                       void *stream) {
    VFEM_TRY
    const std::string w = "vfem_modal_project";
    const ModalGrid g = grid_args(w, dim, nelems_host, h_host, true);
    if (!X) throw Error(w + ": null argument");
    check_count(w, "ncols", ncols, BLOCK_MAX_COLS);
    launch_modal_project(g.nnode, g.N, mask, ncols, X, S(stream));
    VFEM_CATCH
}

int vfem_block_gram(int64_t n, int ka, const double *A, int kb, const double *B, double *G, double *G_host, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_block_gram";
    hipStream_t s = S(stream);
    if (n < 1) throw Error(w + ": n must be at least 1");
    check_count(w, "ka", ka, BLOCK_MAX_COLS);
    check_count(w, "kb", kb, BLOCK_MAX_COLS);
    if (!A || !B) throw Error(w + ": null argument");
    if (!G && !G_host) throw Error(w + ": no output requested");
    const size_t entries = (size_t) ka * kb;
    Scratch work((GRAM_BLOCKS + 1) * entries, s);
    double *out = G ? G : work.p + GRAM_BLOCKS * entries;
    launch_block_gram(n, ka, A, kb, B, work.p, out, s);
    if (G_host) {
        VFEM_HIP(hipMemcpyAsync(G_host, out, entries * sizeof(double), hipMemcpyDeviceToHost, s));
        VFEM_HIP(hipStreamSynchronize(s));
    }
    VFEM_CATCH
}

int vfem_block_combine(int64_t n, int kin, int kout, const double *A, const double *C_host, double *B, void *stream) {
    VFEM_TRY
    const std::string w = "vfem_block_combine";
    if (n < 1) throw Error(w + ": n must be at least 1");
    check_count(w, "kin", kin, BLOCK_MAX_COLS);
    check_count(w, "kout", kout, BLOCK_MAX_COLS);
    if (!A || !C_host || !B) throw Error(w + ": null argument");
    check_finite(w, "the coefficients are", C_host, kin * kout);
    if (overlaps(B, n * kout, A, n * kin)) throw Error(w + ": B aliases A");
    launch_block_combine(n, kin, kout, A, C_host, B, S(stream));
    VFEM_CATCH
}

int vfem_modal_gradient(int dim, const int64_t *nelems_host, const double *h_host, int nmodes, const double *K0_host,
                        const double *cK_host, const double *cM_host, const double *dE, const double *dm, const double *Phi, double *g,
                        void *stream) {
    VFEM_TRY
    const std::string w = "vfem_modal_gradient";
    hipStream_t s = S(stream);
    const ModalGrid grid = grid_args(w, dim, nelems_host, h_host, true);
    check_count(w, "nmodes", nmodes, MODAL_MAX_MODES);
    if (!K0_host || !cK_host || !cM_host || !dE || !dm || !Phi || !g) throw Error(w + ": null argument");
    const int ke = grid.N * (1 << grid.N);
    check_finite(w, "the element matrix is", K0_host, ke * ke);
    check_finite(w, "the coefficients are", cK_host, nmodes);
    check_finite(w, "the coefficients are", cM_host, nmodes);
    ModalCoef c{};
    for (int i = 0; i < nmodes; ++i) {
        c.cK[i] = cK_host[i];
        c.cM[i] = cM_host[i];
    }
    DevBuf<double> K0;
    K0.alloc((size_t) ke * ke);
    VFEM_HIP(hipMemcpyAsync(K0.p, K0_host, (size_t) ke * ke * sizeof(double), hipMemcpyHostToDevice, s));
    launch_modal_gradient(grid, nmodes, K0.p, c, dE, dm, Phi, g, s);
    VFEM_HIP(hipStreamSynchronize(s));          // the table is freed on return
    VFEM_CATCH
}

}  // extern "C"
