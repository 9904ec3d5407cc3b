// Host side of the neural density field (networks.MLP of the reference): weights and their split fp16 operands, forward passes,
// the training backward pass and Adam; the vfem_mlp_* entry points of include/vfem.h.  Kernels: kernels_mlp*.hip.
#include "vfem_host.h"
#include "mlp_args.h"

#include <algorithm>
#include <memory>

using namespace vfem;

// a hidden activation left fp16's range in an earlier reference-precision launch: its high half was inf, the results of that launch
// are not the network's.  Reported by the next entry point (the check costs one 4-byte read-back; launches stay asynchronous)
static void mlp_check_range(vfem_mlp *m, hipStream_t s) {
    if (!m->range_flag.p) return;
    int bad = 0;
    VFEM_HIP(hipMemcpyAsync(&bad, m->range_flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    VFEM_HIP(hipStreamSynchronize(s));
    if (bad) {
        m->range_flag.zero(s);
        throw Error("MLP activation outside fp16's range (>= 65000 or not finite) in the previous reference-precision evaluation: "
                    "its results are invalid; rescale the network or use torch for it");
    }
}
static vfem::MlpArgs mlp_base_args(const vfem_mlp *m) {
    vfem::MlpArgs a{};
    a.range_flag = m->range_flag.p;
    a.ablate = ablate_mlp();
    a.es = m->es; a.nn = m->nn; a.n_hidden = m->n_layers - 2; a.sigmoid = m->sigmoid;
    a.B = m->B.p; a.W1 = m->W1.p; a.Wh = m->Wh.p; a.bias = m->bias.p; a.wout = m->wout.p; a.bout = m->bout;
    return a;
}
static void mlp_grid_args(MlpArgs &a, const int64_t n[3], const double lo[3], const double hi[3]) {
    a.coords = nullptr;
    a.nvox = 1;
    for (int dd = 0; dd < 3; ++dd) {
        a.gn[dd] = (int) n[dd];
        a.glo[dd] = (float) lo[dd];
        a.gstep[dd] = n[dd] > 1 ? (float) ((hi[dd] - lo[dd]) / (double) (n[dd] - 1)) : 0.f;
        a.nvox *= n[dd];
    }
}
// the voxels [first, first + count) of the grid in `a`; false: none (an error unless allow_empty)
static bool mlp_voxel_range(MlpArgs &a, int64_t first, int64_t count, bool allow_empty) {
    if (first < 0 || count < (allow_empty ? 0 : 1) || first + count > a.nvox) throw Error("voxel range outside the grid");
    a.v_offset = first; a.nvox = count;
    return count > 0;
}
// Reference-precision forward (the reference evaluates networks.MLP in fp32 end to end, networks.py:178-185): the fused kernel with
// split fp16 operands (kernels_mlp_x3.hip) -- three MFMA products per product, fp32 accumulation, accurate fp32 sin / cos of the
// argument formed as the reference forms it.  Nothing wider than the output scalar per voxel reaches HBM.
static void mlp_forward_f32_impl(vfem_mlp *m, vfem::MlpArgs base, float *o32, double *o64, hipStream_t s,
                                 const int64_t *grid_n = nullptr, const double *grid_lo = nullptr, const double *grid_hi = nullptr) {
    if (!m->loaded) throw Error("vfem_mlp_load_weights has not been called");
    mlp_check_range(m, s);
    base.out32 = o32; base.out64 = o64;
    m->h0_valid = false;
    bool keep = m->keep_first && grid_n && base.nvox > 0 && m->n_layers > 2 && (size_t) base.nvox * m->nn * 4 <= ((size_t) 96 << 30);
    if (keep) {
        // room for the padded rows of the backward pass's last chunk (they must exist and be finite: they meet dz = 0)
        const size_t rows = (size_t) base.nvox + 4096;
        try {
            m->h0_hi.reserve(rows * m->nn);
            m->h0_lo.reserve(rows * m->nn);
        } catch (const Error &) { (void) hipGetLastError(); m->h0_hi.release(); m->h0_lo.release(); keep = false; }
    }
    if (keep) {
        VFEM_HIP(hipMemsetAsync(m->h0_hi.p + (size_t) base.nvox * m->nn, 0, (size_t) 4096 * m->nn * 2, s));
        VFEM_HIP(hipMemsetAsync(m->h0_lo.p + (size_t) base.nvox * m->nn, 0, (size_t) 4096 * m->nn * 2, s));
        base.save_act = m->h0_hi.p; base.save_act_lo = m->h0_lo.p; base.act_rows = 0; base.save_first_only = 1;
    }
    launch_mlp_forward_x3(base, m->W1h.p, m->W1l.p, m->Whh.p, m->Whl.p, s, m->kc);
    if (keep) {
        for (int dd = 0; dd < 3; ++dd) { m->h0_n[dd] = grid_n[dd]; m->h0_lo_c[dd] = grid_lo[dd]; m->h0_hi_c[dd] = grid_hi[dd]; }
        m->h0_first = base.v_offset; m->h0_count = base.nvox;
        m->h0_valid = true;
    }
}
// Gradients of a scalar loss wrt the MLP parameters given dL/d(out) per voxel (what torch.autograd computes for
// networks.MLP in the reference, train_xdg.py:282-329), at the reference's precision and with no library GEMM
// (kernels_mlp_bwd.hip).  Voxels are processed in chunks: reference-precision forward with saved split activations, fused backward
// data pass, the weight gradients as voxel-reduction GEMMs of our own (first layer: Fourier features regenerated in the kernel),
// column sums for the biases and the output layer.
static void mlp_backward_impl(vfem_mlp *m, vfem::MlpArgs base, const float *coords, const float *g_out, float scale,
                              float *dW1, float *dWh, float *dbias, float *dwout, float *dbout, hipStream_t s,
                              const int64_t *grid_n = nullptr, const double *grid_lo = nullptr, const double *grid_hi = nullptr) {
    if (!m->loaded) throw Error("vfem_mlp_load_weights has not been called");
    if (!(scale > 0.f)) throw Error("loss scale must be positive");
    mlp_check_range(m, s);
    const long long V = base.nvox;
    const int nn = m->nn, K1 = 2 * m->es, nh = m->n_layers - 2, nact = nh + 1;
    if (V <= 0) throw Error("empty voxel set");
    // a chunk: at most 2^20 voxels; its voxel slices (one block of the weight-gradient kernel per slice and output tile): enough
    // blocks to fill the chip -- the first layer has 16 output tiles at the run.md sizes, a hidden layer 4 -- of at least 128 voxels each
    auto plan = [](long long n_c, int &s1, int &sh, long long &rows) {
        s1 = 8; sh = 8;
        while (s1 < 32 && n_c >= (long long) 2 * s1 * 128) s1 *= 2;
        while (sh < 128 && n_c >= (long long) 2 * sh * 128) sh *= 2;
        const long long q = 32LL * std::max(s1, sh);
        rows = (n_c + q - 1) / q * q;
    };
    const long long Vc = std::min<long long>(V, 1LL << 20);
    int s1, sh; long long rows_max;
    plan(Vc, s1, sh, rows_max);
    m->acts.alloc((size_t) nact * rows_max * nn);
    m->acts_lo.alloc((size_t) nact * rows_max * nn);
    m->dz.alloc((size_t) nact * rows_max * nn);
    m->dz_lo.alloc((size_t) nact * rows_max * nn);
    m->gs.alloc((size_t) rows_max);
    m->out_chunk.alloc((size_t) rows_max);
    const size_t colblocks = (size_t) ((rows_max + 511) / 512);
    m->partial.alloc(std::max(std::max((size_t) s1 * nn * K1, (size_t) sh * nn * nn), colblocks * (size_t) nn));
    m->partial_b.alloc((size_t) 128 * nn);
    const float inv = 1.f / scale;
    // the first layer's activations as the forward pass of this step left them (VFEM_MLP_OPT_KEEP_FIRST), if they belong to this grid and range
    bool kept = m->h0_valid && grid_n && !coords && nh >= 1 && m->h0_first == base.v_offset && m->h0_count == V;
    if (kept)
        for (int dd = 0; dd < 3; ++dd) kept = kept && m->h0_n[dd] == grid_n[dd] && m->h0_lo_c[dd] == grid_lo[dd] && m->h0_hi_c[dd] == grid_hi[dd];
    for (long long c0 = 0; c0 < V; c0 += Vc) {
        const long long n_c = std::min(Vc, V - c0);
        long long rows;
        plan(n_c, s1, sh, rows);
        const float beta = c0 == 0 ? 0.f : 1.f;
        if (rows != n_c) { m->acts.zero(s); m->acts_lo.zero(s); }      // padded rows must be finite (they meet dz = 0)
        vfem::MlpArgs a = base;
        a.nvox = n_c; a.v_offset = base.v_offset + c0; a.coords = coords ? coords + 3 * c0 : nullptr;
        a.out32 = m->out_chunk.p; a.out64 = nullptr; a.save_act = m->acts.p; a.save_act_lo = m->acts_lo.p; a.act_rows = rows;
        const uint16_t *k_hi = kept ? m->h0_hi.p + (size_t) c0 * nn : nullptr, *k_lo = kept ? m->h0_lo.p + (size_t) c0 * nn : nullptr;
        a.h0_hi = k_hi; a.h0_lo = k_lo;
        launch_mlp_forward_x3(a, m->W1h.p, m->W1l.p, m->Whh.p, m->Whl.p, s, m->kc);
        a.h0_hi = nullptr; a.h0_lo = nullptr;
        vfem::MlpBwdArgs b{};
        b.nn = nn; b.n_hidden = nh; b.sigmoid = m->sigmoid; b.WhTh = m->WhTh.p; b.WhTl = m->WhTl.p; b.wout = m->wout.p; b.g = g_out + c0;
        b.out32 = m->out_chunk.p; b.scale = scale; b.act_hi = m->acts.p; b.act_lo = m->acts_lo.p; b.dz_hi = m->dz.p; b.dz_lo = m->dz_lo.p;
        b.gs = m->gs.p; b.act_rows = rows; b.nvox = n_c; b.act0_hi = k_hi; b.act0_lo = k_lo;
        launch_mlp_backward_x3(b, rows, s);
        a.save_act = nullptr; a.save_act_lo = nullptr;
        vfem::MlpDwArgs w{};
        w.nn = nn; w.rows = rows; w.terms = m->bwd_terms; w.partial = m->partial.p; w.grid = a;
        // first layer: against the Fourier features of the chunk's voxels, regenerated in the kernel
        w.K = K1; w.dz_hi = m->dz.p; w.dz_lo = m->dz_lo.p; w.h_hi = nullptr; w.h_lo = nullptr; w.slices = s1;
        w.colsum_partial = m->partial_b.p;                              // the layer's bias gradient: column sums of its dz, formed by the same kernel
        launch_mlp_dw(w, s);
        launch_reduce_partials(s1, (long long) nn * K1, m->partial.p, inv, beta, dW1, s);
        launch_reduce_partials(s1, nn, m->partial_b.p, inv, beta, dbias, s);
        for (int l = 0; l < nh; ++l) {
            w.K = nn; w.slices = sh;
            w.dz_hi = m->dz.p + (size_t) (l + 1) * rows * nn; w.dz_lo = m->dz_lo.p + (size_t) (l + 1) * rows * nn;
            w.h_hi = (l == 0 && kept) ? k_hi : m->acts.p + (size_t) l * rows * nn;
            w.h_lo = (l == 0 && kept) ? k_lo : m->acts_lo.p + (size_t) l * rows * nn;
            w.h_lo_scaled = (l == 0 && kept) ? 1 : 0;
            launch_mlp_dw(w, s);
            launch_reduce_partials(sh, (long long) nn * nn, m->partial.p, inv, beta, dWh + (size_t) l * nn * nn, s);
            launch_reduce_partials(sh, nn, m->partial_b.p, inv, beta, dbias + (size_t) (l + 1) * nn, s);
        }
        const int cb = (int) ((rows + 511) / 512);
        launch_colsum_split(rows, nn, m->acts.p + (size_t) nh * rows * nn, m->acts_lo.p + (size_t) nh * rows * nn, m->gs.p, m->partial.p, s);
        launch_reduce_partials(cb, nn, m->partial.p, inv, beta, dwout, s);
        launch_sum_f32(rows, m->gs.p, inv, beta, dbout, m->partial.p, s);
    }
    mlp_check_range(m, s);                               // (the pass's own forward)
}

extern "C" {

int vfem_mlp_create(vfem_mlp **out, int es, int nn, int n_layers, int sigmoid) {
    VFEM_TRY
    if (es <= 0 || es % 32 != 0) throw Error("embedding_size must be a positive multiple of 32");
    if (nn <= 0 || nn % 32 != 0 || nn > 512) throw Error("n_neurons must be a multiple of 32, at most 512");
    if (n_layers < 2) throw Error("n_layers must be at least 2");
    std::unique_ptr<vfem_mlp> m(new vfem_mlp);
    m->es = es; m->nn = nn; m->n_layers = n_layers; m->sigmoid = sigmoid;
    *out = m.release();
    VFEM_CATCH
}
int vfem_mlp_destroy(vfem_mlp *mlp) {
    VFEM_TRY
    delete mlp;
    VFEM_CATCH
}
int vfem_mlp_set_option(vfem_mlp *m, int key, int value) {
    VFEM_TRY
    if (key == VFEM_MLP_OPT_BWD_TERMS) {
        if (value != 1 && value != 3) throw Error("VFEM_MLP_OPT_BWD_TERMS: 3 (hi hi + hi lo + lo hi, reference precision) or 1 (hi hi)");
        m->bwd_terms = value;
    } else if (key == VFEM_MLP_OPT_KEEP_FIRST) {
        m->keep_first = value != 0;
        if (!m->keep_first) { m->h0_valid = false; m->h0_hi.release(); m->h0_lo.release(); }
    } else throw Error("unknown MLP option");
    VFEM_CATCH
}
int vfem_mlp_load_weights(vfem_mlp *m, const float *B, const float *W1, const float *Wh, const float *biases,
                          const float *wout, float bout) {
    VFEM_TRY
    const int nh = m->n_layers - 2;
    auto up = [](DevBuf<float> &d, const float *h, size_t n) {
        d.alloc(n);
        if (n) VFEM_HIP(hipMemcpy(d.p, h, n * sizeof(float), hipMemcpyDefault));
    };
    // fp32 copies first (the reference-precision forward uses them); the fp16 operands and the transposed hidden weights are
    // converted from those on the device: no temporary allocations, no device-wide synchronisation per training step
    up(m->B, B, (size_t) m->es * 3);
    up(m->W1f, W1, (size_t) m->nn * 2 * m->es);
    up(m->Whf, Wh, (size_t) nh * m->nn * m->nn);
    m->W1.alloc((size_t) m->nn * 2 * m->es);
    launch_f32_to_f16_frag(m->nn, 2 * m->es, 0, m->W1f.p, m->W1.p, nullptr);
    m->W1h.alloc((size_t) m->nn * 2 * m->es);
    m->W1l.alloc((size_t) m->nn * 2 * m->es);
    m->kc = m->es % 64 == 0 ? 128 : 64;
    launch_split_f32_frag(m->nn, 2 * m->es, m->W1f.p, m->W1h.p, m->W1l.p, nullptr, m->es, 0, m->kc);
    m->Whh.alloc((size_t) nh * m->nn * m->nn);
    m->Whl.alloc((size_t) nh * m->nn * m->nn);
    for (int l = 0; l < nh; ++l)
        launch_split_f32_frag(m->nn, m->nn, m->Whf.p + (size_t) l * m->nn * m->nn, m->Whh.p + (size_t) l * m->nn * m->nn, m->Whl.p + (size_t) l * m->nn * m->nn, nullptr, 0);
    m->Wh.alloc((size_t) nh * m->nn * m->nn);
    m->WhTh.alloc((size_t) nh * m->nn * m->nn);
    m->WhTl.alloc((size_t) nh * m->nn * m->nn);
    if (nh) {
        for (int l = 0; l < nh; ++l) {
            const size_t o = (size_t) l * m->nn * m->nn;
            launch_f32_to_f16_frag(m->nn, m->nn, 0, m->Whf.p + o, m->Wh.p + o, nullptr);
            launch_split_f32_frag(m->nn, m->nn, m->Whf.p + o, m->WhTh.p + o, m->WhTl.p + o, nullptr, 0, 1);
        }
    }
    up(m->bias, biases, (size_t) (nh + 1) * m->nn);
    up(m->wout, wout, (size_t) m->nn);
    // the split operands carry fp16(w) as their high half: a weight of 65 504 or more would become inf (the fp32 reference has no
    // such limit; networks of this kind have |w| < 10)
    m->range_flag.alloc(1);
    m->range_flag.zero(nullptr);
    launch_range_check_f32((long long) m->nn * 2 * m->es, m->W1f.p, 65504.f, m->range_flag.p, nullptr);
    if (nh) launch_range_check_f32((long long) nh * m->nn * m->nn, m->Whf.p, 65504.f, m->range_flag.p, nullptr);
    {
        int bad = 0;
        VFEM_HIP(hipMemcpy(&bad, m->range_flag.p, sizeof(int), hipMemcpyDeviceToHost));
        if (bad) { m->loaded = false; throw Error("MLP weight of magnitude >= 65504 (or not finite): outside the range of the split fp16 operands"); }
    }
    VFEM_HIP(hipStreamSynchronize(nullptr));      // the conversions ran on the null stream; consumers may launch on any stream
    m->bout = bout;
    m->h0_valid = false;
    m->loaded = true;
    VFEM_CATCH
}
int vfem_mlp_forward(vfem_mlp *m, const float *coords, int64_t nvox, float *o32, double *o64, void *stream) {
    VFEM_TRY
    if (!m->loaded) throw Error("vfem_mlp_load_weights has not been called");
    MlpArgs a = mlp_base_args(m);
    a.coords = coords; a.nvox = nvox; a.out32 = o32; a.out64 = o64;
    launch_mlp_forward(a, S(stream));
    VFEM_CATCH
}
int vfem_mlp_forward_grid(vfem_mlp *m, const int64_t n[3], const double lo[3], const double hi[3], float *o32, double *o64,
                          void *stream) {
    VFEM_TRY
    if (!m->loaded) throw Error("vfem_mlp_load_weights has not been called");
    MlpArgs a = mlp_base_args(m);
    mlp_grid_args(a, n, lo, hi);
    a.out32 = o32; a.out64 = o64;
    launch_mlp_forward(a, S(stream));
    VFEM_CATCH
}
int vfem_mlp_forward_grid_range(vfem_mlp *m, const int64_t n[3], const double lo[3], const double hi[3], int64_t first_voxel,
                                int64_t num_voxels, float *o32, double *o64, void *stream) {
    VFEM_TRY
    if (!m->loaded) throw Error("vfem_mlp_load_weights has not been called");
    MlpArgs a = mlp_base_args(m);
    mlp_grid_args(a, n, lo, hi);
    if (!mlp_voxel_range(a, first_voxel, num_voxels, true)) return 0;
    a.out32 = o32; a.out64 = o64;                      // outputs are indexed from the start of the range
    launch_mlp_forward(a, S(stream));
    VFEM_CATCH
}
int vfem_mlp_forward_f32(vfem_mlp *m, const float *coords, int64_t nvox, float *o32, double *o64, void *stream) {
    VFEM_TRY
    MlpArgs a = mlp_base_args(m);
    a.coords = coords; a.nvox = nvox;
    mlp_forward_f32_impl(m, a, o32, o64, S(stream));
    VFEM_CATCH
}
int vfem_mlp_forward_grid_range_f32(vfem_mlp *m, const int64_t n[3], const double lo[3], const double hi[3], int64_t first_voxel,
                                    int64_t num_voxels, float *o32, double *o64, void *stream) {
    VFEM_TRY
    MlpArgs a = mlp_base_args(m);
    mlp_grid_args(a, n, lo, hi);
    if (!mlp_voxel_range(a, first_voxel, num_voxels, true)) return 0;
    mlp_forward_f32_impl(m, a, o32, o64, S(stream), n, lo, hi);
    VFEM_CATCH
}
int vfem_mlp_backward(vfem_mlp *m, const float *coords, int64_t nvox, const float *g_out, float loss_scale, float *dW1,
                      float *dWh, float *dbias, float *dwout, float *dbout, void *stream) {
    VFEM_TRY
    MlpArgs a = mlp_base_args(m);
    a.nvox = nvox;
    mlp_backward_impl(m, a, coords, g_out, loss_scale, dW1, dWh, dbias, dwout, dbout, S(stream));
    VFEM_CATCH
}
int vfem_mlp_backward_grid(vfem_mlp *m, const int64_t n[3], const double lo[3], const double hi[3], const float *g_out,
                           float loss_scale, float *dW1, float *dWh, float *dbias, float *dwout, float *dbout, void *stream) {
    VFEM_TRY
    MlpArgs a = mlp_base_args(m);
    mlp_grid_args(a, n, lo, hi);
    mlp_backward_impl(m, a, nullptr, g_out, loss_scale, dW1, dWh, dbias, dwout, dbout, S(stream), n, lo, hi);
    VFEM_CATCH
}
int vfem_mlp_backward_grid_range(vfem_mlp *m, const int64_t n[3], const double lo[3], const double hi[3], int64_t first_voxel,
                                 int64_t num_voxels, const float *g_out, float loss_scale, float *dW1, float *dWh, float *dbias,
                                 float *dwout, float *dbout, void *stream) {
    VFEM_TRY
    MlpArgs a = mlp_base_args(m);
    mlp_grid_args(a, n, lo, hi);
    mlp_voxel_range(a, first_voxel, num_voxels, false);
    mlp_backward_impl(m, a, nullptr, g_out, loss_scale, dW1, dWh, dbias, dwout, dbout, S(stream), n, lo, hi);
    VFEM_CATCH
}
int vfem_adam_step(int64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float lr, float beta1,
                   float beta2, float eps, int step, void *stream) {
    VFEM_TRY
    if (step < 1) throw Error("Adam step count starts at 1");
    launch_adam(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, S(stream));
    VFEM_CATCH
}

}  // extern "C"
