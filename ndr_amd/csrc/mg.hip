// The multigrid hierarchy of the trilinear simulator: creation (levels, coarsened Dirichlet masks, coarsened reference matrices),
// operator updates, V-cycle / FMG / PCG drivers and the vfem_mg_* entry points of include/vfem.h (the slab solve: mg_slab.hip).
//
// The hierarchy follows the reference's MultigridSolver constructor (levels, Dirichlet coarsening: VoxelFEM/MultigridSolver.hh:22-90
// of the reference checkout); the cycles and the PCG loop are those of mg_cycle.h, launched as TunedOps says.
#include "mg_cycle.h"

#include <algorithm>
#include <cstring>
#include <memory>

using namespace vfem;

// ------------------------------------------------------------------------------------------
// shared with the generic hierarchies (generic.hip)
// ------------------------------------------------------------------------------------------
void vfem::coarsen_dirichlet_mask(int N, int p, const int fine_nn[3], const std::vector<uint8_t> &fm, const int coarse_ne[3],
                                  std::vector<uint8_t> &cm) {
    long long nf_total = 1, nc_total = 1;
    int cnn[3] = {1, 1, 1};
    for (int a = 0; a < N; ++a) { cnn[a] = p * coarse_ne[a] + 1; nf_total *= fine_nn[a]; nc_total *= cnn[a]; }
    cm.assign((size_t) nc_total, 0);
    for (long long nf = 0; nf < nf_total; ++nf) {
        const uint8_t m = fm[nf];
        if (!m) continue;
        int g[3] = {0, 0, 0};
        { long long q = nf; for (int a = N - 1; a >= 0; --a) { g[a] = (int) (q % fine_nn[a]); q /= fine_nn[a]; } }
        int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
        bool any = false;
        for (int a = 0; a < N; ++a) {
            const int e = std::min(g[a] / (2 * p), coarse_ne[a] - 1), t = g[a] - 2 * p * e;
            if (t == 0) { lo[a] = hi[a] = p * e; any = true; }
            else if (t == 2 * p) { lo[a] = hi[a] = p * e + p; any = true; }
            else { lo[a] = p * e; hi[a] = p * e + p; }
        }
        if (!any) throw Error("Dirichlet constraints on internal nodes are not supported");
        for (int a0 = lo[0]; a0 <= hi[0]; ++a0)
            for (int a1 = lo[1]; a1 <= hi[1]; ++a1)
                for (int a2 = lo[2]; a2 <= hi[2]; ++a2) {
                    const int gg[3] = {a0, a1, a2};
                    long long node = gg[0];
                    for (int a = 1; a < N; ++a) node = node * cnn[a] + gg[a];
                    cm[node] |= m;
                }
    }
}

void vfem::galerkin_project(const double *K, int ke, int N, int npe, const double *Phi, double *T, double *out) {
    for (int i = 0; i < ke; ++i)
        for (int j = 0; j < ke; ++j) {
            const int m = j / N, b = j % N;
            double v = 0.0;
            for (int qn = 0; qn < npe; ++qn) v += K[(size_t) i * ke + N * qn + b] * Phi[qn * npe + m];
            T[(size_t) i * ke + j] = v;
        }
    for (int i = 0; i < ke; ++i)
        for (int j = 0; j < ke; ++j) {
            const int n = i / N, a = i % N;
            double v = 0.0;
            for (int pn = 0; pn < npe; ++pn) v += Phi[pn * npe + n] * T[(size_t) (N * pn + a) * ke + j];
            out[(size_t) i * ke + j] = v;
        }
}

// ------------------------------------------------------------------------------------------
// multigrid internals
// ------------------------------------------------------------------------------------------

static const double *level_K(const vfem_mg *mg, int l) {
    return l == 0 ? mg->fine->dK0.p : mg->cK0.p;
}
// fine-moduli pointer seen by the matrix-free kernels of level l (0 or 1): element (ex,ey,ez) of the level's node grid
// must land on the right entry of the fine array, which may hold extra x-layers (slab decomposition)
static const double *level_E(const vfem_mg *mg, int l) {
    const vfem_sim *sim = mg->fine;
    if (l == 0) return sim->Ep();
    return sim->E.p + 2 * mg->lv[1].ex_lo * (long long) sim->d.ny * sim->d.nz;
}

// level 1 with its operator stored as a stencil (VFEM_OPT_L1_STORED): the kernels of the deeper levels apply
static bool level_uses_stencil(const vfem_mg *mg, int l) {
    const MgLevel &L = mg->lv[l];
    return L.kind == OP_STENCIL || (l == 1 && L.kind == OP_MF1 && mg->fine->tune.l1_stored == 1 && L.S.p);
}
static bool level_uses_half_stencil(const vfem_mg *mg, int l) {
    const MgLevel &L = mg->lv[l];
    return l == 1 && L.kind == OP_MF1 && mg->fine->tune.l1_stored == 2 && L.Sh.p;
}

// level 1 evaluated per mirror class (VFEM_OPT_L1_MERGED): needs the mirror symmetry of the coarsened matrices
static bool level_uses_merged_rows(const vfem_mg *mg, int l) {
    const MgLevel &L = mg->lv[l];
    return l == 1 && L.kind == OP_MF1 && mg->mf1_sym && mg->fine->tune.l1_merged && mg->fine->tune.gs_variant == 0 && mg->l1mtab.p &&
           l1_merged_usable(L.d);
}

void vfem::mg_apply(vfem_mg *mg, int l, const double *u, const double *b, int res, double *out, hipStream_t s) {
    MgLevel &L = mg->lv[l];
    if (level_uses_half_stencil(mg, l)) launch_apply_stencil_half(L.d, L.Sh.p, u, b, L.maskp, res, out, s);
    else if (level_uses_stencil(mg, l)) launch_apply_stencil(L.d, L.S.p, u, b, L.maskp, res, out, s);
    else if (L.kind == OP_MF0 && mg->fine->fast_ok) {
        const vfem_sim *sim = mg->fine;
        const Tuning &t = sim->tune;
        if (t.apply_impl == 0 &&
            launch_apply_dma(L.d, sim->Dm, level_E(mg, 0), sim->E.p + sim->n_store(), u, out, s, 0, -1, t.dma_chunks, t.dma_strip,
                             res ? b : nullptr, res ? L.maskp : nullptr, t.dma_lx)) return;
        launch_apply_fast(L.d, sim->Dm, level_E(mg, 0), u, b, L.maskp, res, out, s, t.apply_pd);
    }
    else if (level_uses_merged_rows(mg, l)) launch_l1_merged_apply(L.d, mg->l1mtab.p, level_E(mg, l), u, b, L.maskp, res, out, s);
    else launch_apply_gather(L.d, L.kind, level_K(mg, l), level_E(mg, l), u, b, L.maskp, res, out, s);
}

void vfem::mg_smooth(vfem_mg *mg, int l, double *u, const double *b, int forward, hipStream_t s, int first, int count) {
    MgLevel &L = mg->lv[l];
    if (level_uses_half_stencil(mg, l)) launch_gs_sweep_stencil_half(L.d, L.Sh.p, u, b, L.maskp, forward, L.xparity, first, count, s);
    else if (level_uses_stencil(mg, l)) launch_gs_sweep_stencil(L.d, L.S.p, u, b, L.maskp, forward, L.xparity, first, count, s, L.Sn.p, mg->fine->tune.stencil_split);
    else if (level_uses_merged_rows(mg, l)) launch_l1_merged_sweep(L.d, mg->l1mtab.p, level_E(mg, l), u, b, L.maskp, forward, L.xparity, first, count, s,
                                                                   mg->fine->tune.l1_merged == 2);
    else launch_gs_sweep_mf(L.d, L.kind, level_K(mg, l), l == 0 ? mg->fine->dGsTab.p : mg->mf1diag.p, level_E(mg, l), u, b, L.maskp,
                            forward, L.xparity, first, count, s, mg->fine->tune, mg->mf1_sym,
                            (l == 1 && mg->fine->tune.l1_diag) ? L.Mdiag.p : nullptr);
}

// gs_march: 0 row kernels, 1 marching kernel on grids where it wins (measured per sweep, marching / rows, profiles/r04_gs_march_chunks.txt:
// 512^3 6.27 / 9.76 ms, 256^3 0.98 / 1.43, 160^3 0.26 / 0.44, 128^3 0.20 / 0.23, 96^3 0.08 / 0.105; slabs 64 x 512^2 0.90 / 1.42,
// 32 x 256^2 0.18 / 0.23), 2 marching kernel always
static bool gs_march_wanted(const MgLevel &L, const Tuning &t) {
    return t.gs_march == 2 || (t.gs_march == 1 && L.d.nn >= 800000);
}

// the marching sweep sums a node row per neighbour kind, which needs K0 with the mirror symmetry of a box voxel and an isotropic tensor:
// the neighbour-kind table of K0, or null (then the row kernels do the sweep)
static const double *march_table(const vfem_sim *sim) {
    return sim->k0_mirror_ok ? sim->dGsTab.p + GS_TABLE_DOUBLES + 84 : nullptr;
}

// level l is level 0 of a hierarchy that sweeps it with the marching kernel (kernels_gs_march.hip)
static bool level0_marches(const vfem_mg *mg, int l) {
    const vfem_sim *sim = mg->fine;
    const Tuning &t = sim->tune;
    return l == 0 && mg->lv[0].kind == OP_MF0 && gs_march_wanted(mg->lv[0], t) && t.gs_variant == 0 && t.gs_resident && sim->dGsTab.p &&
           sim->k0_mirror_ok;
}

// level 0: solve data of the marching sweeps, recomputed when the moduli (or the material / Dirichlet mask: both bump the version) changed
static void gs_solve_data(vfem_mg *mg, hipStream_t s) {
    MgLevel &L = mg->lv[0];
    const vfem_sim *sim = mg->fine;
    if (L.gs_sd.p && L.gs_sd_version == sim->operator_version) return;
    L.gs_sd.reserve((size_t) L.d.nn * 3);
    launch_gs_solve_data(L.d, sim->dK0.p, level_E(mg, 0), L.maskp, L.gs_sd.p, s);
    L.gs_sd_version = sim->operator_version;
}

// n consecutive sweeps of level l in one direction.  Level 0 runs them as marching half sweeps (kernels_gs_march.hip) when
// it can: those are out of place, so the planes of either parity alternate between u and the level's scratch vector; an even
// number of sweeps ends in u, an odd one is followed by a copy of the planes left in the scratch vector.
static void mg_smooth_n(vfem_mg *mg, int l, double *u, const double *b, int forward, int n, hipStream_t s) {
    MgLevel &L = mg->lv[l];
    const vfem_sim *sim = mg->fine;
    const Tuning &t = sim->tune;
    if (!(level0_marches(mg, l) && n > 0)) {
        for (int i = 0; i < n; ++i) mg_smooth(mg, l, u, b, forward, s);
        return;
    }
    L.tmp.reserve((size_t) L.d.nn * 3);
    gs_solve_data(mg, s);
    double *cur[2] = {u, u};                         // where the planes of local parity 0 / 1 currently live
    for (int i = 0; i < n; ++i)
        for (int half = 0; half < 2; ++half) {
            const int cx = forward ? half : 1 - half;                    // colour groups 0-3 / 4-7 of MG.hh:292-310, reversed for a backward sweep
            const int cxl = cx ^ (L.xparity & 1);
            if (cxl > L.d.NX - 1) continue;
            double *dst = cur[cxl] == u ? L.tmp.p : u;
            if (!launch_gs_march_mf0(L.d, march_table(sim), level_E(mg, 0), cur[cxl], cur[1 - cxl], dst, b, L.gs_sd.p,
                                     cxl, forward, t.gs_march_chunks, s, 0, -1)) {
                // buffers the kernel cannot take: finish in place with the row kernels
                for (int par = 0; par < 2; ++par)
                    if (cur[par] != u) { launch_copy_planes(L.d, par, cur[par], u, s); cur[par] = u; }
                mg_smooth(mg, l, u, b, forward, s, 4 * half, 4);
                continue;
            }
            cur[cxl] = dst;
        }
    for (int par = 0; par < 2; ++par)
        if (cur[par] != u) launch_copy_planes(L.d, par, cur[par], u, s);
}

bool vfem::mg_smooth_half(vfem_mg *mg, int l, double *u, const double *b, int forward, int half, hipStream_t s, int plane_lo, int plane_hi) {
    MgLevel &L = mg->lv[l];
    const vfem_sim *sim = mg->fine;
    const Tuning &t = sim->tune;
    if (!level0_marches(mg, l)) return false;
    const int cx = forward ? half : 1 - half;
    const int cxl = cx ^ (L.xparity & 1);
    if (cxl > L.d.NX - 1) return true;
    L.tmp.reserve((size_t) L.d.nn * 3);
    gs_solve_data(mg, s);
    if (!launch_gs_march_mf0(L.d, march_table(sim), level_E(mg, 0), u, u, L.tmp.p, b, L.gs_sd.p,
                             cxl, forward, t.gs_march_chunks, s, plane_lo, plane_hi)) return false;
    launch_copy_planes(L.d, cxl, L.tmp.p, u, s, plane_lo, plane_hi);
    return true;
}

// coarsest level: dense inverse, or the plane-block factorisation (plane_spd.hip) where the mode asks for it -- auto: above the
// dense path's limit.  Both refuse before anything is allocated
static void factor_coarsest(vfem_mg *mg, hipStream_t s) {
    const int L = mg->L;
    MgLevel &cl = mg->lv[L];
    CoarsestSolver &cs = mg->coarsest;
    const long long n = 3 * cl.d.nn;
    const bool planes = cs.wants_planes(n);
    cs.refuse_if_too_large(n, planes ? &cl.d : nullptr);
    const double *Sc = cl.S.p;
    DevBuf<double> tmpS;
    if (L < 2) {
        tmpS.alloc((size_t) stencil_storage_doubles(cl.d));
        launch_stencil_from_mf(cl.d, L == 0 ? OP_MF0 : OP_MF1, level_K(mg, L), level_E(mg, L), tmpS.p, s);
        Sc = tmpS.p;
    }
    if (planes) cs.factor_planes(cl.d, Sc, cl.maskp, s);
    else {
        launch_dense_from_stencil(cl.d, Sc, cl.maskp, cs.dense_matrix(n, s), s);
        cs.factor_dense(3, cl.maskp, s);
    }
    VFEM_HIP(hipStreamSynchronize(s));   // tmpS lifetime
}

static void build_reference_tables(vfem_mg *mg);

void vfem::update_operators(vfem_mg *mg, hipStream_t s) {
    vfem_sim *sim = mg->fine;
    // the reference rebuilds the coarse operators at the start of every solve (MG.hh:690-691) because its densities may have
    // changed; here the simulator counts the changes, so a solve on unchanged moduli (a second right-hand side, the objective's
    // constructor solve followed by setVars with the same design) keeps Galerkin matrices, stencils and the dense inverse
    if (mg->operators_valid && mg->operators_version == sim->operator_version) return;
    ScopedTimer tm("updateElementStiffnessMatrices");
    if (mg->material_version != sim->material_version) {     // the material changed since the hierarchy was created
        VFEM_HIP(hipStreamSynchronize(s));
        build_reference_tables(mg);
    }
    const int L = mg->slab ? mg->L - 1 : mg->L;      // the last level of a slab hierarchy only serves the grid transfers
    // Galerkin element matrices for levels >= 2 (level 1 stays virtual: sum_f E_f cK0[f])
    // (element arrays cover lv.da = node grid + extra x-layers; array origins halve exactly from level to level)
    // (a replicated coarse hierarchy of a slab decomposition may be handed the element matrices of its first active level,
    // vfem_mg_import_level_ke: it then never looks at its simulator's moduli)
    for (int l = mg->external_ke_level > 0 ? mg->external_ke_level + 1 : 2; l <= L; ++l) {
        MgLevel &lv = mg->lv[l];
        lv.Ke.alloc((size_t) lv.da.ne * 576);
        if (l == 2) launch_coarsen_ke(lv.da, 3, mg->c2K0.p, sim->E.p, nullptr, lv.Ke.p, s);
        else        launch_coarsen_ke(lv.da, 2, nullptr, nullptr, mg->lv[l - 1].Ke.p, lv.Ke.p, s);
    }
    if (mg->L >= 1 && mg->first_active <= 1 && mg->mf1_sym && sim->tune.l1_diag) {   // level 1: diagonal blocks of the virtual operator
        MgLevel &l1 = mg->lv[1];
        l1.Mdiag.alloc((size_t) l1.d.nn * 9);
        launch_mf1_diag(l1.d, mg->mf1diag.p, level_E(mg, 1), l1.Mdiag.p, s);
    }
    if (mg->L >= 1 && mg->first_active <= 1 && !mg->slab) {                           // level 1 stored as a stencil (option, off by default)
        MgLevel &l1 = mg->lv[1];
        if (sim->tune.l1_stored == 1 && l1.kind == OP_MF1 && L >= 2) {
            l1.S.alloc((size_t) stencil_storage_doubles(l1.d));
            launch_stencil_from_mf(l1.d, OP_MF1, level_K(mg, 1), level_E(mg, 1), l1.S.p, s);
            l1.Sn.release();
            l1.Sh.release();
        } else if (sim->tune.l1_stored == 2 && l1.kind == OP_MF1 && L >= 2) {
            l1.Sh.alloc((size_t) stencil_half_storage_doubles(l1.d));
            launch_stencil_half_from_mf1(l1.d, level_K(mg, 1), level_E(mg, 1), l1.Sh.p, s);
            l1.S.release();
        } else if (l1.kind == OP_MF1) { l1.S.release(); l1.Sh.release(); }
    }
    for (int l = std::max(2, mg->first_active); l <= L; ++l) {
        MgLevel &lv = mg->lv[l];
        lv.S.alloc((size_t) stencil_storage_doubles(lv.d));
        launch_stencil_from_ke(lv.d, lv.Ke.p + lv.ex_lo * (long long) lv.d.ny * lv.d.nz * 576, lv.S.p, s);
        if (lv.d.nn <= WAVE_SWEEP_MAX_NODES) {
            lv.Sn.alloc((size_t) stencil_storage_doubles(lv.d));
            launch_stencil_node_major(lv.d, lv.S.p, lv.Sn.p, s);
        } else lv.Sn.release();
    }
    if (!mg->slab) factor_coarsest(mg, s);            // (a slab's coarse levels live in the replicated hierarchy)
    mg->operators_valid = true;
    mg->operators_version = sim->operator_version;
}

// how the trilinear hierarchy launches the steps of mg_cycle.h (work vectors: the levels' own; the CG vectors: the hierarchy's)
namespace {
struct TunedOps {
    vfem_mg *mg;
    hipStream_t s;
    MgLevel &lv(int l) const { return mg->lv[(size_t) l]; }

    int last_level() const { return mg->L; }
    void last_level_cycle(bool) { mg->coarsest.solve(lv(mg->L).b.p, lv(mg->L).x.p, s); }
    bool symmetric() const { return mg->symmetric_gs; }
    double *x(int l) const { return lv(l).x.p; }
    double *b(int l) const { return lv(l).b.p; }
    void enforce_dirichlet(int l, bool residual_system, bool dirichlet_zeroed) {
        if (!(dirichlet_zeroed && residual_system))
            launch_enforce_dirichlet(lv(l).d.nn, lv(l).maskp, l == 0 ? mg->fine->dvals.p : nullptr, x(l), residual_system ? 1 : 0, s);
    }
    void smooth(int l, int forward, int n) { mg_smooth_n(mg, l, x(l), b(l), forward, n, s); }
    void residual(int l) { mg_apply(mg, l, x(l), b(l), 1, lv(l).r.p, s); }                 // computeResidual (Dirichlet zeroed)
    // ... and the zero initial guess of the coarse level in the same launch
    void restrict_residual(int l) { launch_restrict(lv(l + 1).d, lv(l).d.NX, lv(l + 1).xshift, lv(l).r.p, b(l + 1), s, x(l + 1)); }
    void restrict_rhs(int l) { launch_restrict(lv(l + 1).d, lv(l).d.NX, lv(l + 1).xshift, b(l), b(l + 1), s); }
    void prolong_correction(int l) { launch_prolong(lv(l + 1).d, lv(l).d.NX, lv(l + 1).xshift, x(l + 1), x(l), 1, s); }
    bool prolong_start(int l, bool residual_system) {
        launch_prolong(lv(l + 1).d, lv(l).d.NX, lv(l + 1).xshift, x(l + 1), x(l), 0, s, residual_system ? lv(l).maskp : nullptr);
        return residual_system;
    }
    // the vector work between the cycle and the apply is fused: three passes fewer than one kernel per line of MG.hh:713-725 (same
    // sums in the same order: iterates and residuals are unchanged bit for bit)
    long long n_dofs() const { return 3 * lv(0).d.nn; }
    mg_cycle::CgWork cg() const { return {n_dofs(), mg->pd.p, mg->pAd.p, mg->scal.p, s}; }
    double *s_vector(bool preconditioned) const { return preconditioned ? x(0) : mg->ps.p; }
    void dot(const double *a, const double *b, double *out) { launch_dot(n_dofs(), a, b, mg->scratch.p, out, s); }
    void initial_residual(const double *x, const double *b, double *r) { mg_apply(mg, 0, x, b, 1, r, s); }
    void shift_and_dot_rs(const double *r, double *sv, double *sc) {
        launch_shift_scalar(sc, s);
        launch_dot_zero_dirichlet(n_dofs(), r, sv, lv(0).maskp, mg->scratch.p, sc + 0, s);
    }
    void apply_dot(const double *d, double *Ad, double *out) {
        mg_apply(mg, 0, d, nullptr, 0, Ad, s);
        launch_dot_zero_dirichlet(n_dofs(), d, Ad, lv(0).maskp, mg->scratch.p, out, s);
    }
    void step_dot(double *x, double *r, const double *d, const double *Ad, double *sc) { launch_pcg_step_dot(n_dofs(), x, r, d, Ad, sc, mg->scratch.p, sc + 3, s); }
};
}  // namespace

void vfem::cycle_from_level(vfem_mg *mg, int l, int nsmooth, bool fmg, hipStream_t s) {
    TunedOps o{mg, s};
    mg_cycle::cycles(o, l, 1, nsmooth, true, fmg);
}

// what the hierarchy derives from the simulator's reference matrix K0 alone; rebuilt when the material changes (update_operators)
static void build_reference_tables(vfem_mg *mg) {
    vfem_sim *fine = mg->fine;
    // interpolation of a coarse element onto its child g = 4gx+2gy+gz: phi[g](fine node, coarse node), nodes numbered x slowest
    double phi[8][64];
    for (int g = 0; g < 8; ++g)
        for (int fn = 0; fn < 8; ++fn)
            for (int cn = 0; cn < 8; ++cn) {
                double v = 1.0;
                for (int dd = 0; dd < 3; ++dd) {
                    const int sh = 2 - dd;
                    const double p = 0.5 * ((fn >> sh) & 1) + 0.5 * ((g >> sh) & 1);
                    v *= ((cn >> sh) & 1) ? p : (1.0 - p);
                }
                phi[g][fn * 8 + cn] = v;
            }
    // coarsened reference matrices cK0[g] = I_g^T K0 I_g (MG.hh:644-648), and c2K0[g][f] = I_g^T cK0[f] I_g: level-2 element
    // matrices are a plain weighted sum of these 64 over the fine moduli
    std::vector<double> c(8 * 576), c2((size_t) 64 * 576), T(576);
    for (int g = 0; g < 8; ++g) galerkin_project(fine->K0, 24, 3, 8, phi[g], T.data(), c.data() + (size_t) g * 576);
    for (int g = 0; g < 8; ++g)
        for (int f = 0; f < 8; ++f)
            galerkin_project(c.data() + (size_t) f * 576, 24, 3, 8, phi[g], T.data(), c2.data() + (size_t) (g * 8 + f) * 576);
    mg->cK0.alloc(c.size());
    VFEM_HIP(hipMemcpy(mg->cK0.p, c.data(), c.size() * sizeof(double), hipMemcpyHostToDevice));
    mg->c2K0.alloc(c2.size());
    VFEM_HIP(hipMemcpy(mg->c2K0.p, c2.data(), c2.size() * sizeof(double), hipMemcpyHostToDevice));
    mg->mf1_sym = coarsened_matrices_are_mirror_images(c.data());
    {
        double dt[96];
        build_mf1_diag_table(c.data(), dt);
        mg->mf1diag.alloc(96);
        VFEM_HIP(hipMemcpy(mg->mf1diag.p, dt, sizeof(dt), hipMemcpyHostToDevice));
        double mt[L1M_TABLE_DOUBLES];
        build_l1_merged_table(c.data(), mt);
        mg->l1mtab.alloc(L1M_TABLE_DOUBLES);
        VFEM_HIP(hipMemcpy(mg->l1mtab.p, mt, sizeof(mt), hipMemcpyHostToDevice));
    }
    mg->material_version = fine->material_version;
}

static void finish_mg_create(vfem_mg *mg) {
    vfem_sim *fine = mg->fine;
    build_reference_tables(mg);
    for (int l = mg->first_active; l <= mg->L; ++l) {
        MgLevel &lv = mg->lv[(size_t) l];
        lv.x.alloc((size_t) lv.d.nn * 3); lv.b.alloc((size_t) lv.d.nn * 3); lv.r.alloc((size_t) lv.d.nn * 3);
        lv.x.zero(nullptr); lv.b.zero(nullptr); lv.r.zero(nullptr);
    }
    if (mg->first_active == 0 && !mg->slab) {
        const size_t n3 = (size_t) fine->d.nn * 3;
        mg->pd.alloc(n3); mg->pAd.alloc(n3); mg->ps.alloc(n3);
    }
    mg->scal.alloc(16); mg->scratch.alloc(REDUCE_SCRATCH_DOUBLES);
    mg->scal.zero(nullptr);
    VFEM_HIP(hipDeviceSynchronize());
}

static int mg_create_common(vfem_mg **out, vfem_sim *fine, int L, int first_active) {
    VFEM_TRY
    if (L < 0) throw Error("numCoarseningLevels must be >= 0");
    if (first_active < 0 || first_active > L) throw Error("first active level out of range");
    if (fine->ex_lo || fine->ex_hi) throw Error("simulators with element padding need vfem_mg_create_slab");
    std::unique_ptr<vfem_mg> mg(new vfem_mg);
    mg->fine = fine; mg->L = L; mg->first_active = first_active;
    mg->lv.resize((size_t) L + 1);
    long long ne[3] = {fine->d.nx, fine->d.ny, fine->d.nz};
    for (int l = 0; l <= L; ++l) {
        MgLevel &lv = mg->lv[l];
        if (l > 0) {
            for (int dd = 0; dd < 3; ++dd) {
                if (ne[dd] % 2 == 1)
                    throw Error("Grid size currently must be divisible by 2^numCoarseningLevels (nonuniform coarsening not yet implemented)");
                ne[dd] /= 2;
            }
        }
        lv.d = Dims(ne[0], ne[1], ne[2]);
        lv.da = lv.d;
        lv.kind = (l == 0) ? OP_MF0 : (l == 1 ? OP_MF1 : OP_STENCIL);
        if (l == 0) { lv.hmask = fine->hmask; lv.maskp = fine->dmask.p; }
        else {
            const Dims &f = mg->lv[l - 1].d;
            const int fnn[3] = {f.NX, f.NY, f.NZ}, cne[3] = {lv.d.nx, lv.d.ny, lv.d.nz};
            coarsen_dirichlet_mask(3, 1, fnn, mg->lv[l - 1].hmask, cne, lv.hmask);
            lv.mask.alloc((size_t) lv.d.nn);
            VFEM_HIP(hipMemcpy(lv.mask.p, lv.hmask.data(), (size_t) lv.d.nn, hipMemcpyHostToDevice));
            lv.maskp = lv.mask.p;
        }
    }
    finish_mg_create(mg.get());
    *out = mg.release();
    VFEM_CATCH
}

static void check_level(const vfem_mg *mg, int level) {
    if (level < 0 || level > mg->L) throw Error("level out of range");
}

extern "C" {

int vfem_mg_create(vfem_mg **out, vfem_sim *fine, int L) { return mg_create_common(out, fine, L, 0); }
int vfem_mg_create_partial(vfem_mg **out, vfem_sim *fine, int L, int first_active_level) {
    return mg_create_common(out, fine, L, first_active_level);
}

int vfem_mg_create_slab(vfem_mg **out, vfem_sim *fine, int n_levels, const vfem_slab_level *lv_in,
                        const uint8_t *const *masks_host) {
    VFEM_TRY
    if (n_levels < 1) throw Error("need at least one level");
    if (!fine->fast_ok || !fine->k0_mirror_ok)
        throw Error("slab hierarchies need a material on the mode-space kernels (isotropic or grid-aligned orthotropic tensor): "
                    "the plane-range apply has no general form");
    std::unique_ptr<vfem_mg> mg(new vfem_mg);
    mg->fine = fine; mg->L = n_levels - 1; mg->slab = true;
    mg->lv.resize((size_t) n_levels);
    long long ny = fine->d.ny, nz = fine->d.nz;
    for (int l = 0; l < n_levels; ++l) {
        MgLevel &lv = mg->lv[l];
        if (l > 0) {
            if (ny % 2 || nz % 2) throw Error("Grid size currently must be divisible by 2^numCoarseningLevels (nonuniform coarsening not yet implemented)");
            ny /= 2; nz /= 2;
        }
        lv.d = Dims(lv_in[l].nx, ny, nz);
        lv.ex_lo = lv_in[l].elem_extra_lo; lv.ex_hi = lv_in[l].elem_extra_hi;
        lv.da = Dims(lv_in[l].nx + lv.ex_lo + lv.ex_hi, ny, nz);
        lv.xshift = (int) lv_in[l].xshift; lv.xparity = lv_in[l].xparity & 1;
        lv.kind = (l == 0) ? OP_MF0 : (l == 1 ? OP_MF1 : OP_STENCIL);
        if (l > 0 && l < n_levels - 1 && mg->lv[l - 1].da.nx != 2 * lv.da.nx)
            throw Error("slab element arrays must halve exactly between levels");   // (the last level only serves the transfers)
        lv.hmask.assign(masks_host[l], masks_host[l] + lv.d.nn);
        lv.mask.alloc((size_t) lv.d.nn);
        VFEM_HIP(hipMemcpy(lv.mask.p, lv.hmask.data(), (size_t) lv.d.nn, hipMemcpyHostToDevice));
        lv.maskp = lv.mask.p;
    }
    if (fine->d.nx != mg->lv[0].d.nx || fine->ex_lo != mg->lv[0].ex_lo || fine->ex_hi != mg->lv[0].ex_hi)
        throw Error("level 0 of the slab hierarchy does not match the simulator");
    finish_mg_create(mg.get());
    *out = mg.release();
    VFEM_CATCH
}
int vfem_mg_destroy(vfem_mg *mg) {
    VFEM_TRY
    delete mg;
    VFEM_CATCH
}
int vfem_mg_num_levels(const vfem_mg *mg) { return mg->L + 1; }
int vfem_mg_level_dims(const vfem_mg *mg, int level, int64_t ne[3]) {
    VFEM_TRY
    const Dims &d = mg->lv.at((size_t) level).d;
    ne[0] = d.nx; ne[1] = d.ny; ne[2] = d.nz;
    VFEM_CATCH
}
int64_t vfem_mg_level_num_nodes(const vfem_mg *mg, int level) {
    if (level < 0 || level > mg->L) return -1;
    return mg->lv[(size_t) level].d.nn;
}
int vfem_mg_level_dirichlet_mask(const vfem_mg *mg, int level, uint8_t *mask_host) {
    VFEM_TRY
    const MgLevel &lv = mg->lv.at((size_t) level);
    std::memcpy(mask_host, lv.hmask.data(), lv.hmask.size());
    VFEM_CATCH
}
int vfem_mg_set_symmetric_gauss_seidel(vfem_mg *mg, int symmetric) { mg->symmetric_gs = symmetric != 0; return 0; }
int vfem_mg_tensor_paths(const vfem_mg *mg) {
    // (the level-1 flag is that of the reference matrices the hierarchy currently holds: they follow the material at the next update)
    return vfem_sim_tensor_paths(mg->fine) | (mg->mf1_sym ? VFEM_PATH_L1_MIRROR : 0);
}
const double *vfem_mg_field_ptr(const vfem_mg *mg, int which, int level) {
    if (which == 2) return mg->lv[0].b.p;          // the PCG residual lives in the level-0 right-hand side
    if (level < 0 || level > mg->L) return nullptr;
    return which == 0 ? mg->lv[(size_t) level].x.p : mg->lv[(size_t) level].b.p;
}

int vfem_mg_update_operators(vfem_mg *mg, void *stream) { VFEM_TRY update_operators(mg, S(stream)); VFEM_CATCH }

int vfem_mg_export_level_ke(vfem_mg *mg, int level, int64_t child_first_layer, int64_t count_x, double *ke_out, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (level < 2) throw Error("element matrices exist from level 2 on (level 1 is virtual)");
    if (count_x < 0 || child_first_layer < 0) throw Error("negative layer range");
    update_operators(mg, S(stream));
    const MgLevel &lv = mg->lv[(size_t) level];
    const Dims c(count_x, lv.d.ny, lv.d.nz);
    if (level == 2) {         // straight from the fine moduli (64 per element): layers child_first_layer .. of the simulator's array
        const vfem_sim *sim = mg->fine;
        if (child_first_layer + 4 * count_x > sim->d.nx + sim->ex_lo + sim->ex_hi) throw Error("layer range outside the fine element array");
        launch_coarsen_ke(c, 3, mg->c2K0.p, sim->E.p + child_first_layer * (long long) sim->d.ny * sim->d.nz, nullptr, ke_out, S(stream));
    } else {
        const MgLevel &ch = mg->lv[(size_t) level - 1];
        if (!ch.Ke.p) throw Error("the child level holds no element matrices");
        if (child_first_layer + 2 * count_x > ch.da.nx) throw Error("layer range outside the child level's element array");
        launch_coarsen_ke(c, 2, nullptr, nullptr, ch.Ke.p + child_first_layer * (long long) ch.da.ny * ch.da.nz * 576, ke_out, S(stream));
    }
    VFEM_CATCH
}
int vfem_mg_import_level_ke(vfem_mg *mg, int level, const double *ke, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (level < 2 || level != mg->first_active) throw Error("element matrices can be supplied for the first active level (>= 2) of a partial hierarchy");
    MgLevel &lv = mg->lv[(size_t) level];
    lv.Ke.alloc((size_t) lv.da.ne * 576);
    VFEM_HIP(hipMemcpyAsync(lv.Ke.p, ke, (size_t) lv.da.ne * 576 * sizeof(double), hipMemcpyDeviceToDevice, S(stream)));
    mg->external_ke_level = level;
    mg->operators_valid = false;              // rebuilt from these matrices at the next update
    VFEM_CATCH
}

int vfem_mg_apply_k(vfem_mg *mg, int level, const double *u, double *out, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (level >= 1) update_operators(mg, S(stream));          // no-op when the operators match the current moduli
    mg_apply(mg, level, u, nullptr, 0, out, S(stream));
    VFEM_CATCH
}
int vfem_mg_residual(vfem_mg *mg, int level, const double *u, const double *b, double *r, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (level >= 1) update_operators(mg, S(stream));          // no-op when the operators match the current moduli
    mg_apply(mg, level, u, b, 1, r, S(stream));
    VFEM_CATCH
}
int vfem_mg_smooth(vfem_mg *mg, int level, double *u, const double *b, int forward, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (level >= 1) update_operators(mg, S(stream));          // no-op when the operators match the current moduli
    mg_smooth_n(mg, level, u, b, forward, 1, S(stream));
    VFEM_CATCH
}
int vfem_mg_smooth_sweeps(vfem_mg *mg, int level, double *u, const double *b, int forward, int sweeps, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (sweeps < 0) throw Error("negative sweep count");
    if (level >= 1) update_operators(mg, S(stream));
    mg_smooth_n(mg, level, u, b, forward, sweeps, S(stream));
    VFEM_CATCH
}
int vfem_mg_zero_dirichlet(vfem_mg *mg, int level, double *u, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    launch_zero_dirichlet(mg->lv[(size_t) level].d.nn, mg->lv[(size_t) level].maskp, u, S(stream));
    VFEM_CATCH
}
int vfem_mg_restrict(vfem_mg *mg, int fine_level, const double *fine, double *coarse, void *stream) {
    VFEM_TRY
    check_level(mg, fine_level + 1);
    launch_restrict(mg->lv[(size_t) fine_level + 1].d, mg->lv[(size_t) fine_level].d.NX, mg->lv[(size_t) fine_level + 1].xshift, fine, coarse, S(stream));
    VFEM_CATCH
}
int vfem_mg_interpolate(vfem_mg *mg, int fine_level, const double *coarse, double *fine, int accumulate, void *stream) {
    VFEM_TRY
    check_level(mg, fine_level + 1);
    launch_prolong(mg->lv[(size_t) fine_level + 1].d, mg->lv[(size_t) fine_level].d.NX, mg->lv[(size_t) fine_level + 1].xshift, coarse, fine, accumulate, S(stream));
    VFEM_CATCH
}
int vfem_mg_coarsest_solve(vfem_mg *mg, const double *b, double *x, void *stream) {
    VFEM_TRY
    update_operators(mg, S(stream));
    mg->coarsest.solve(b, x, S(stream));
    VFEM_CATCH
}
int vfem_mg_set_coarsest_solver(vfem_mg *mg, int mode) {
    VFEM_TRY
    if (mg->coarsest.set_mode(mode)) mg->operators_valid = false;      // the kept factorisation belongs to the old mode
    VFEM_CATCH
}
int64_t vfem_mg_coarsest_bytes(const vfem_mg *mg) {
    if (!mg->operators_valid || mg->slab) return 0;
    return mg->coarsest.bytes();
}

int vfem_mg_smooth_colors(vfem_mg *mg, int level, double *u, const double *b, int forward, int first, int count, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (first < 0 || count < 0 || first + count > 8) throw Error("colour range out of [0, 8)");
    if (level >= 1) update_operators(mg, S(stream));          // no-op when the operators match the current moduli
    if (first % 4 == 0 && count == 4 && mg_smooth_half(mg, level, u, b, forward, first / 4, S(stream))) return 0;
    mg_smooth(mg, level, u, b, forward, S(stream), first, count);
    VFEM_CATCH
}
/* one colour group (colours [4 group, 4 group + 4) of the sweep order) restricted to the node planes [plane_lo, plane_hi] of the
 * level's local grid: what a slab rank needs to relax its interface planes first, start the halo exchange, and relax the
 * interior meanwhile.  Only the marching finest-level sweep can do this (out of place, plane by plane); the return value of
 * vfem_mg_can_smooth_planes says whether this level of this hierarchy does. */
int vfem_mg_can_smooth_planes(vfem_mg *mg, int level) {
    return (mg && level <= mg->L && level0_marches(mg, level)) ? 1 : 0;
}
int vfem_mg_smooth_group_planes(vfem_mg *mg, int level, double *u, const double *b, int forward, int group, int64_t plane_lo, int64_t plane_hi,
                                void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (group < 0 || group > 1) throw Error("colour group must be 0 or 1");
    if (plane_lo < 0 || plane_hi > mg->lv[(size_t) level].d.NX - 1) throw Error("plane range outside the level's node grid");
    if (plane_lo > plane_hi) return 0;
    if (!mg_smooth_half(mg, level, u, b, forward, group, S(stream), (int) plane_lo, (int) plane_hi))
        throw Error("plane-range sweeps need the marching finest-level kernel (vfem_mg_can_smooth_planes)");
    VFEM_CATCH
}
int vfem_mg_cycle_from_level(vfem_mg *mg, int level, double *x, const double *b, int nsmooth, int fmg, void *stream) {
    VFEM_TRY
    check_level(mg, level);
    if (level < mg->first_active) throw Error("level below the first active level of this hierarchy");
    if (mg->slab) throw Error("slab hierarchies are cycled by the distributed driver");
    hipStream_t s = S(stream);
    update_operators(mg, s);
    TunedOps o{mg, s};
    mg_cycle::cycles_on(o, level, 3 * mg->lv[(size_t) level].d.nn, x, b, 1, nsmooth, true, fmg != 0, s);
    VFEM_CATCH
}

int vfem_mg_solve(vfem_mg *mg, double *x, const double *f, int num_steps, int nsmooth, int stiffness_updated,
                  int zero_dirichlet, int fmg, void *stream) {
    VFEM_TRY
    ScopedTimer tm("MG Solver");
    hipStream_t s = S(stream);
    (void) stiffness_updated;                       // the simulator tracks changes of the moduli itself
    update_operators(mg, s);
    if (num_steps == 0) return 0;
    TunedOps o{mg, s};
    mg_cycle::cycles_on(o, 0, o.n_dofs(), x, f, num_steps, nsmooth, zero_dirichlet != 0, fmg != 0, s);
    VFEM_CATCH
}

int vfem_mg_pcg(vfem_mg *mg, double *x, const double *b, int max_iter, double tol, int mg_iterations,
                int mg_smoothing, int fmg, vfem_residual_cb residual_cb, void *cb_user, int *iters_out,
                double *relres_out, void *stream) {
    VFEM_TRY
    hipStream_t s = S(stream);
    vfem_sim *sim = mg->fine;
    if (mg->slab || mg->first_active != 0) throw Error("this hierarchy is driven by the distributed solver");
    launch_enforce_dirichlet(sim->d.nn, mg->lv[0].maskp, sim->dvals.p, x, 0, s);    // MG.hh:687-688
    update_operators(mg, s);                                                      // MG.hh:690-691
    ScopedTimer tm("CG Iterations");
    TunedOps o{mg, s};
    mg_cycle::pcg(o, x, b, max_iter, tol, mg_iterations, mg_smoothing, fmg != 0, residual_cb, cb_user, iters_out, relres_out);
    VFEM_CATCH
}

}  // extern "C"
