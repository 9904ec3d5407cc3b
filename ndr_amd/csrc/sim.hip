// The trilinear simulator (TensorProductSimulator<1,1,1>): reference element, densities and moduli, K u, compliance and its
// gradient, the direct solve; the vfem_sim_* entry points of include/vfem.h.
#include "vfem_host.h"
#include "gs_coef.h"

#include <cmath>
#include <cstring>
#include <memory>

using namespace vfem;

// ------------------------------------------------------------------------------------------
// reference element: closed-form Q1 stiffness for an axis-aligned box voxel, isotropic C or any flattened tensor D.
// Same quantity as Element_T::Stiffness (TPS.hh:127-140), which integrates it by 2-point Gauss
// quadrature (exact for these integrands); derived here from the 1-D integrals
//   Mm[a][b] = int N_a N_b,  Dd[a][b] = int N_a' N_b',  Gg[a][b] = int N_a' N_b   on [0,1].
// ------------------------------------------------------------------------------------------
void vfem_sim::update_k0() {
    static const double Mm[2][2] = {{1.0 / 3, 1.0 / 6}, {1.0 / 6, 1.0 / 3}};
    static const double Dd[2][2] = {{1.0, -1.0}, {-1.0, 1.0}};
    static const double Gg[2][2] = {{-0.5, -0.5}, {0.5, 0.5}};
    const double vol = h[0] * h[1] * h[2];
    auto I = [&](int n, int m, int p, int q) {   // int d_p N_n d_q N_m over the reference cube, physical gradients
        double v = 1.0 / (h[p] * h[q]);
        for (int dd = 0; dd < 3; ++dd) {
            const int a = (n >> (2 - dd)) & 1, b = (m >> (2 - dd)) & 1;
            if (dd == p && dd == q) v *= Dd[a][b];
            else if (dd == p)       v *= Gg[a][b];
            else if (dd == q)       v *= Gg[b][a];
            else                    v *= Mm[a][b];
        }
        return v;
    };
    // a general tensor: K0[(n,a),(m,b)] = vol sum_pq C_apbq int d_p N_n d_q N_m with C_apbq = D[flat(a,p)][flat(b,q)].  The isotropic
    // case keeps its own three-term form (the same sum with the zero terms left out: results of existing inputs stay bit-identical)
    static const int flat[3][3] = {{0, 5, 4}, {5, 1, 3}, {4, 3, 2}};              // Flattening.hh: xx yy zz yz xz xy
    for (int n = 0; n < 8; ++n)
        for (int a = 0; a < 3; ++a)
            for (int m = 0; m < 8; ++m)
                for (int b = 0; b < 3; ++b) {
                    double v = 0.0;
                    if (general_tensor) {
                        // (one of each transposed pair is summed, the other copies it: K0 is symmetric bit for bit whatever the order of the terms)
                        const bool tr = a > b || (a == b && n > m);
                        const int n_ = tr ? m : n, a_ = tr ? b : a, m_ = tr ? n : m, b_ = tr ? a : b;
                        for (int p = 0; p < 3; ++p)
                            for (int q = 0; q < 3; ++q) v += D[flat[a_][p] * 6 + flat[b_][q]] * I(n_, m_, p, q);
                    } else {
                        v = lambda * I(n, m, a, b) + mu * I(n, m, b, a);
                        if (a == b) v += mu * (I(n, m, 0, 0) + I(n, m, 1, 1) + I(n, m, 2, 2));
                    }
                    K0[(3 * n + a) * 24 + 3 * m + b] = vol * v;
                }
    ++material_version;
    // mode-space form: Dmode = T K0 T^T / 64 with T = H (x) H (x) H, H = [[1,1],[-1,1]] per axis.
    // For a box voxel with an orthotropic/isotropic tensor only 45 entries survive:
    // 21 diagonal ones (the three rigid translations are null) and 12 symmetric couplings.
    double T[8][8];
    for (int p = 0; p < 8; ++p)
        for (int n = 0; n < 8; ++n) {
            double v = 1.0;
            for (int dd = 0; dd < 3; ++dd) {
                const int pb = (p >> (2 - dd)) & 1, nb = (n >> (2 - dd)) & 1;
                if (pb && !nb) v = -v;
            }
            T[p][n] = v;
        }
    std::vector<double> TK(576), Dfull(576);
    for (int p = 0; p < 8; ++p)
        for (int a = 0; a < 3; ++a)
            for (int col = 0; col < 24; ++col) {
                double v = 0.0;
                for (int n = 0; n < 8; ++n) v += T[p][n] * K0[(3 * n + a) * 24 + col];
                TK[(3 * p + a) * 24 + col] = v;
            }
    double maxabs = 0.0;
    for (int row = 0; row < 24; ++row)
        for (int q = 0; q < 8; ++q)
            for (int b = 0; b < 3; ++b) {
                double v = 0.0;
                for (int m = 0; m < 8; ++m) v += TK[row * 24 + 3 * m + b] * T[q][m];
                Dfull[row * 24 + 3 * q + b] = v / 64.0;
                maxabs = std::max(maxabs, std::fabs(v / 64.0));
            }
    // pack: Dm[0..23] diagonal (3p+a); Dm[24..35] couplings (order fixed in kernels_apply.hip)
    for (int q = 0; q < 64; ++q) Dm[q] = 0.0;
    std::vector<char> used(576, 0);
    for (int r = 0; r < 24; ++r) { Dm[r] = Dfull[r * 24 + r]; used[r * 24 + r] = 1; }
    // coupling list: for each component pair (a<b), third axis t, parity pt of the third axis:
    //   lambda-type: u_a mode (bit a [+ pt*bit t]) <-> u_b mode (bit b [+ pt*bit t])
    //   mu-type:     u_a mode (bit b [+ pt*bit t]) <-> u_b mode (bit a [+ pt*bit t])
    int idx = 24;
    auto bit = [](int axis) { return 1 << (2 - axis); };
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b) {
            const int t = 3 - a - b;
            for (int pt = 0; pt < 2; ++pt)
                for (int type = 0; type < 2; ++type) {
                    const int pa = (type == 0 ? bit(a) : bit(b)) | (pt ? bit(t) : 0);
                    const int pb = (type == 0 ? bit(b) : bit(a)) | (pt ? bit(t) : 0);
                    const int r = 3 * pa + a, c = 3 * pb + b;
                    Dm[idx++] = Dfull[r * 24 + c];
                    used[r * 24 + c] = 1; used[c * 24 + r] = 1;
                }
        }
    fast_ok = true;
    for (int q = 0; q < 576; ++q)
        if (!used[q] && std::fabs(Dfull[q]) > 1e-13 * maxabs) fast_ok = false;
    dK0.alloc(576);
    VFEM_HIP(hipMemcpy(dK0.p, K0, sizeof(K0), hipMemcpyHostToDevice));
    double tab[GS_TABLE_DOUBLES + 36 + 48 + 96];
    vfem::build_gs_table(K0, tab);
    gs_resident_ok = vfem::build_gs_coef(K0, tab + GS_TABLE_DOUBLES);
    vfem::build_gs_coef_parts(tab + GS_TABLE_DOUBLES, tab + GS_TABLE_DOUBLES + 36, tab + GS_TABLE_DOUBLES + 60);
    tune.gs_resident = gs_resident_ok ? 1 : 0;
    {   // K0 by neighbour kind for the node-per-lane marching sweep (class 0 of l1m::build_table applied to K0 itself); it relies on
        // K0[(n^f,a),(m^f,b)] = s_a(f) s_b(f) K0[(n,a),(m,b)] (box voxel, isotropic / orthotropic tensor), checked here
        double full[L1M_TABLE_DOUBLES];
        vfem::build_l1_merged_table(K0, full);
        std::memcpy(tab + GS_TABLE_DOUBLES + 84, full, 96 * sizeof(double));
        double scale = 0.0, err = 0.0;
        for (int q = 0; q < 576; ++q) scale = std::max(scale, std::fabs(K0[q]));
        for (int f = 1; f < 8; ++f)
            for (int n = 0; n < 8; ++n)
                for (int a = 0; a < 3; ++a)
                    for (int m = 0; m < 8; ++m)
                        for (int b = 0; b < 3; ++b) {
                            const double sg = (((f >> (2 - a)) ^ (f >> (2 - b))) & 1) ? -1.0 : 1.0;
                            err = std::max(err, std::fabs(K0[(3 * n + a) * 24 + 3 * m + b] - sg * K0[(3 * (n ^ f) + a) * 24 + 3 * (m ^ f) + b]));
                        }
        k0_mirror_ok = err <= 1e-13 * scale;
    }
    dGsTab.alloc(GS_TABLE_DOUBLES + 36 + 48 + 96);
    VFEM_HIP(hipMemcpy(dGsTab.p, tab, sizeof(tab), hipMemcpyHostToDevice));
}

void vfem::check_flattened_tensor(const double *D, int n) {
    double maxabs = 0.0;
    for (int q = 0; q < n * n; ++q) {
        if (!std::isfinite(D[q])) throw Error("elasticity tensor has a non-finite entry");
        maxabs = std::max(maxabs, std::fabs(D[q]));
    }
    for (int i = 0; i < n; ++i) {
        if (!(D[i * n + i] > 0.0)) throw Error("elasticity tensor is not positive definite");
        for (int j = 0; j < i; ++j)
            if (std::fabs(D[i * n + j] - D[j * n + i]) > 1e-10 * maxabs) throw Error("elasticity tensor is not symmetric");
    }
}

double vfem::compliance(long long n,const double *f, const double *u, hipStream_t s) {
    double *tmp = nullptr;                           // the partial sums, then the result
    VFEM_HIP(hipMallocAsync((void **) &tmp, (REDUCE_SCRATCH_DOUBLES + 1) * sizeof(double), s));
    launch_dot(n, f, u, tmp, tmp + REDUCE_SCRATCH_DOUBLES, s);
    double v = 0.0;
    VFEM_HIP(hipMemcpyAsync(&v, tmp + REDUCE_SCRATCH_DOUBLES, sizeof(double), hipMemcpyDeviceToHost, s));
    VFEM_HIP(hipFreeAsync(tmp, s));
    VFEM_HIP(hipStreamSynchronize(s));
    return 0.5 * v;
}

extern "C" {

int vfem_sim_create_padded(vfem_sim **out, const double bbmin[3], const double bbmax[3], const int64_t ne[3], int64_t extra_lo,
                           int64_t extra_hi) {
    VFEM_TRY
    for (int dd = 0; dd < 3; ++dd)
        if (ne[dd] < 1 || ne[dd] > 4096) throw Error("elements per dimension must be in [1, 4096]");
    if (extra_lo < 0 || extra_hi < 0) throw Error("negative padding");
    std::unique_ptr<vfem_sim> sim(new vfem_sim);
    sim->d = Dims(ne[0], ne[1], ne[2]);
    for (int dd = 0; dd < 3; ++dd) {
        sim->h[dd] = (bbmax[dd] - bbmin[dd]) / (double) ne[dd];          // TPS.hh:287
        if (!(sim->h[dd] > 0)) throw Error("empty domain bounding box");
    }
    sim->update_k0();
    sim->ex_lo = extra_lo; sim->ex_hi = extra_hi;
    sim->rho.alloc((size_t) sim->n_store());   sim->rho.zero(nullptr);
    sim->E.alloc((size_t) sim->n_store());
    launch_simp(sim->n_store(), sim->rho.p, sim->E0, sim->Emin, sim->gamma, sim->E.p, nullptr);
    sim->dmask.alloc((size_t) sim->d.nn); sim->dmask.zero(nullptr);
    sim->dvals.alloc((size_t) sim->d.nn * 3); sim->dvals.zero(nullptr);
    sim->loads.alloc((size_t) sim->d.nn * 3); sim->loads.zero(nullptr);
    sim->hmask.assign((size_t) sim->d.nn, 0);
    sim->hvals.assign((size_t) sim->d.nn * 3, 0.0);
    VFEM_HIP(hipDeviceSynchronize());
    *out = sim.release();
    VFEM_CATCH
}
int vfem_sim_create(vfem_sim **out, const double bbmin[3], const double bbmax[3], const int64_t ne[3]) {
    return vfem_sim_create_padded(out, bbmin, bbmax, ne, 0, 0);
}
int vfem_sim_destroy(vfem_sim *sim) { VFEM_TRY delete sim; VFEM_CATCH }
int64_t vfem_sim_num_nodes(const vfem_sim *sim) { return sim->d.nn; }
int64_t vfem_sim_num_elements(const vfem_sim *sim) { return sim->d.ne; }
int64_t vfem_sim_num_stored_elements(const vfem_sim *sim) { return sim->n_store(); }

int vfem_sim_set_isotropic(vfem_sim *sim, double young, double poisson) {
    VFEM_TRY
    sim->lambda = poisson * young / ((1.0 + poisson) * (1.0 - 2.0 * poisson));   // ElasticityTensor.hh:105-106
    sim->mu = young / (2.0 + 2.0 * poisson);
    sim->general_tensor = false;
    sim->update_k0();
    ++sim->operator_version;
    VFEM_CATCH
}
int vfem_sim_set_elasticity_tensor(vfem_sim *sim, const double D[36]) {
    VFEM_TRY
    check_flattened_tensor(D, 6);
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) sim->D[i * 6 + j] = 0.5 * (D[i * 6 + j] + D[j * 6 + i]);
    sim->general_tensor = true;
    sim->update_k0();
    ++sim->operator_version;
    VFEM_CATCH
}
int vfem_sim_tensor_paths(const vfem_sim *sim) {
    return (sim->fast_ok ? VFEM_PATH_MODE_SPACE : 0) | (sim->gs_resident_ok ? VFEM_PATH_GS_RESIDENT : 0) |
           (sim->k0_mirror_ok ? VFEM_PATH_K0_MIRROR : 0);
}
int vfem_sim_set_simp(vfem_sim *sim, double E0, double Emin, double gamma) {
    VFEM_TRY
    sim->E0 = E0; sim->Emin = Emin; sim->gamma = gamma;
    ++sim->operator_version;
    launch_simp(sim->n_store(), sim->rho.p, E0, Emin, gamma, sim->E.p, nullptr);
    VFEM_HIP(hipDeviceSynchronize());
    VFEM_CATCH
}
int vfem_sim_set_option(vfem_sim *sim, int key, int value) {
    VFEM_TRY
    Tuning &t = sim->tune;
    switch (key) {
        case VFEM_OPT_APPLY_PLANES:  if (value < 2 || value > 4) throw Error("planes in flight must be 2..4"); t.apply_pd = value; break;
        case VFEM_OPT_GS_VARIANT:    t.gs_variant = value != 0; break;
        case VFEM_OPT_APPLY_IMPL:    t.apply_impl = value != 0; break;
        case VFEM_OPT_DMA_CHUNKS:    if (value < 0) throw Error("negative chunk count"); t.dma_chunks = value; break;
        case VFEM_OPT_DMA_STRIP:     if (value < 0 || value > 2) throw Error("strip mode must be 0..2"); t.dma_strip = value; break;
        case VFEM_OPT_DMA_LX:        if (value < 0 || value > 2) throw Error("line-exclusive tiling mode must be 0..2"); t.dma_lx = value; break;
        case VFEM_OPT_GS_PAIR:       t.gs_pair = value != 0; break;
        case VFEM_OPT_GS_RESIDENT:   t.gs_resident = (value != 0 && sim->gs_resident_ok) ? 1 : 0; break;
        case VFEM_OPT_L1_SPLIT:      if (value != 1 && value != 2 && value != 4 && value != 8) throw Error("level-1 slot split 1, 2, 4 or 8"); t.l1_split = value; break;
        case VFEM_OPT_STENCIL_SPLIT: t.stencil_split = value != 0; break;
        case VFEM_OPT_GS_MARCH:      if (value < 0 || value > 2) throw Error("marching sweep mode 0..2"); t.gs_march = value; break;
        case VFEM_OPT_GS_MARCH_CHUNKS: if (value < 0) throw Error("negative chunk count"); t.gs_march_chunks = value; break;
        case VFEM_OPT_L1_STORED:     if (value < 0 || value > 2) throw Error("level-1 storage mode 0..2"); t.l1_stored = value; ++sim->operator_version; break;
        case VFEM_OPT_L1_MERGED:     if (value < 0 || value > 2) throw Error("level-1 row mode 0..2"); t.l1_merged = value; break;
        case VFEM_OPT_L1_DIAG:       t.l1_diag = value != 0; ++sim->operator_version; break;   // hierarchies (re)build the blocks
        default: throw Error("unknown simulator option " + std::to_string(key));
    }
    VFEM_CATCH
}
int vfem_sim_k0(const vfem_sim *sim, double *K0_host) {
    VFEM_TRY std::memcpy(K0_host, sim->K0, sizeof(sim->K0)); VFEM_CATCH
}
int vfem_sim_set_dirichlet(vfem_sim *sim, const uint8_t *mask_host, const double *values_host) {
    VFEM_TRY
    sim->hmask.assign(mask_host, mask_host + sim->d.nn);
    sim->nonzero_dirichlet = false;
    if (values_host) {
        sim->hvals.assign(values_host, values_host + 3 * sim->d.nn);
        for (long long n = 0; n < sim->d.nn; ++n)
            for (int c = 0; c < 3; ++c)
                if (((sim->hmask[n] >> c) & 1) && sim->hvals[3 * n + c] != 0.0) sim->nonzero_dirichlet = true;
    } else sim->hvals.assign((size_t) sim->d.nn * 3, 0.0);
    ++sim->operator_version;                    // (the level-0 solve data of the marching sweeps carries the mask)
    VFEM_HIP(hipMemcpy(sim->dmask.p, sim->hmask.data(), (size_t) sim->d.nn, hipMemcpyHostToDevice));
    VFEM_HIP(hipMemcpy(sim->dvals.p, sim->hvals.data(), (size_t) sim->d.nn * 3 * sizeof(double), hipMemcpyHostToDevice));
    VFEM_CATCH
}
int vfem_sim_set_loads(vfem_sim *sim, const double *f, void *stream) {
    VFEM_TRY
    VFEM_HIP(hipMemcpyAsync(sim->loads.p, f, (size_t) sim->d.nn * 3 * sizeof(double), hipMemcpyDeviceToDevice, S(stream)));
    VFEM_CATCH
}
int vfem_sim_build_load_vector(const vfem_sim *sim, double *f, void *stream) {
    VFEM_TRY
    VFEM_HIP(hipMemcpyAsync(f, sim->loads.p, (size_t) sim->d.nn * 3 * sizeof(double), hipMemcpyDeviceToDevice, S(stream)));
    VFEM_CATCH
}
int vfem_sim_set_densities(vfem_sim *sim, const double *rho, void *stream) {
    VFEM_TRY
    VFEM_HIP(hipMemcpyAsync(sim->rho.p, rho, (size_t) sim->n_store() * sizeof(double), hipMemcpyDeviceToDevice, S(stream)));
    ++sim->operator_version;
    launch_simp(sim->n_store(), sim->rho.p, sim->E0, sim->Emin, sim->gamma, sim->E.p, S(stream));
    VFEM_CATCH
}
int vfem_sim_set_uniform_density(vfem_sim *sim, double rho, void *stream) {
    VFEM_TRY
    if (rho > 1.0 || rho < 0.0)
        throw Error("Density value (" + std::to_string(rho) + ") has to be in between 0 and 1");   // TPS.hh:457-458
    ++sim->operator_version;
    launch_fill(sim->n_store(), rho, sim->rho.p, S(stream));
    launch_simp(sim->n_store(), sim->rho.p, sim->E0, sim->Emin, sim->gamma, sim->E.p, S(stream));
    VFEM_CATCH
}
int vfem_sim_get_densities(const vfem_sim *sim, double *rho, void *stream) {
    VFEM_TRY
    VFEM_HIP(hipMemcpyAsync(rho, sim->rho.p, (size_t) sim->n_store() * sizeof(double), hipMemcpyDeviceToDevice, S(stream)));
    VFEM_CATCH
}
int vfem_sim_apply_k(const vfem_sim *sim, const double *u, double *out, int variant, void *stream) {
    VFEM_TRY
    ScopedTimer tm("applyK");
    if (variant != 1 && sim->fast_ok) {
        bool done = false;
        if (variant == 0 && sim->tune.apply_impl == 0)
            done = launch_apply_dma(sim->d, sim->Dm, sim->Ep(), sim->E.p + sim->n_store(), u, out, S(stream), 0, -1,
                                    sim->tune.dma_chunks, sim->tune.dma_strip, nullptr, nullptr, sim->tune.dma_lx);
        if (!done) launch_apply_fast(sim->d, sim->Dm, sim->Ep(), u, nullptr, nullptr, 0, out, S(stream), sim->tune.apply_pd);
    }
    else launch_apply_gather(sim->d, OP_MF0, sim->dK0.p, sim->Ep(), u, nullptr, nullptr, 0, out, S(stream));
    VFEM_CATCH
}
int vfem_sim_apply_k_planes(const vfem_sim *sim, const double *u, double *out, int64_t plane_lo, int64_t plane_hi, void *stream) {
    VFEM_TRY
    if (plane_lo < 0 || plane_hi > sim->d.NX - 1) throw Error("plane range outside the node grid");
    if (plane_lo > plane_hi) return 0;
    if (!sim->fast_ok) throw Error("plane-range apply needs the mode-space kernel (box voxels, isotropic or grid-aligned orthotropic tensor)");
    if (!launch_apply_dma(sim->d, sim->Dm, sim->Ep(), sim->E.p + sim->n_store(), u, out, S(stream), (int) plane_lo, (int) plane_hi,
                          sim->tune.dma_chunks, sim->tune.dma_strip, nullptr, nullptr, sim->tune.dma_lx))
        throw Error("plane-range apply needs 8-byte aligned device buffers");
    VFEM_CATCH
}
int vfem_sim_compliance_gradient(const vfem_sim *sim, const double *u, double *g, void *stream) {
    VFEM_TRY
    launch_compliance_gradient(sim->d, sim->dK0.p, sim->rhop(), sim->E0, sim->Emin, sim->gamma, u, g, S(stream));
    VFEM_CATCH
}
int vfem_compliance(const vfem_sim *sim, const double *f, const double *u, double *value_host, void *stream) {
    VFEM_TRY *value_host = compliance(3 * sim->d.nn, f, u, S(stream)); VFEM_CATCH
}
int vfem_sim_direct_solve(vfem_sim *sim, const double *f, double *u, void *stream) {
    VFEM_TRY
    if (sim->nonzero_dirichlet) throw Error("Nonzero Dirichlet constraints currently unsupported");
    const int ne[3] = {sim->d.nx, sim->d.ny, sim->d.nz};
    band_direct_solve(sim->direct, sim->operator_version, 3, 1, ne, sim->dK0.p, sim->Ep(), sim->dmask.p, f, u, S(stream));
    VFEM_CATCH
}
int64_t vfem_sim_direct_factorizations(const vfem_sim *sim) { return sim->direct.factorizations; }
int64_t vfem_sim_direct_band_bytes(const vfem_sim *sim) {
    const int ne[3] = {sim->d.nx, sim->d.ny, sim->d.nz};
    long long n, w;
    band_geometry(3, 1, ne, n, w);
    return band_spd_doubles(n, w) * (int64_t) sizeof(double);
}

}  // extern "C"
