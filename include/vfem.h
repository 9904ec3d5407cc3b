/*
 * vfem.h -- C ABI of libvfem, the MI355X-native voxel-FEM hot path.
 *
 * This is the drop-in boundary for the one path of Nikronic/ndr this repository accelerates
 * (SURVEY.md section 8): the matrix-free SIMP stiffness apply, the geometric-multigrid
 * preconditioned CG compliance solve, the compliance sensitivity and the Fourier-feature
 * MLP density field.  Each entry point names the reference interface it replaces
 * (paths relative to the reference checkout; "TPS" = VoxelFEM/TensorProductSimulator.hh,
 * "MG" = VoxelFEM/MultigridSolver.hh, "VoxelFEM.cc" = VoxelFEM/python_bindings/VoxelFEM.cc).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; vfem_last_error() then
 *     holds the message (the reference throws std::runtime_error -> Python RuntimeError).
 *   - all `double*` / `float*` / `uint8_t*` array arguments are DEVICE pointers (HBM) unless
 *     the parameter name ends in `_host`.  vfem_malloc / vfem_copy_* are provided so a caller
 *     without another HIP allocator (cgo, JNI, plain C) can stage data.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls enqueue work
 *     and return; calls that return scalars to the host synchronise that stream.
 *   - grids: row-major, last axis fastest (NDVector.hh:284-292); nodal fields are
 *     [numNodes][3] doubles (TPS.hh:227); densities/gradients are [numElements] doubles.
 *   - vfem_sim / vfem_mg are the tuned degree-1 3-D path (TensorProductSimulator<1,1,1>); vfem_gsim / vfem_gmg
 *     cover the other instantiations (2-D, degree 2) with the same semantics.
 */
#ifndef VFEM_H
#define VFEM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vfem_sim vfem_sim;     /* TensorProductSimulator<1,1,1>                            (TPS.hh:219) */
typedef struct vfem_mg  vfem_mg;      /* MultigridSolver<1,1,1>                                    (MG.hh:11)   */
typedef struct vfem_mlp vfem_mlp;     /* networks.MLP (Fourier features + ReLU MLP)                (networks.py:128) */
typedef struct vfem_gsim vfem_gsim;   /* TensorProductSimulator<p,..,p>, N = 2 or 3, p = 1 or 2; <2,2,2> = 27-node hexahedra,
                                         unbound in the reference (VoxelFEM.cc:226-229) */
typedef struct vfem_hom_mg vfem_hom_mg; /* the multigrid hierarchy of one periodic cell (vfem_hom_mg_*) */
typedef struct vfem_gmg vfem_gmg;     /* MultigridSolver<p,..,p> of the generic path */
typedef struct vfem_thermal_mg vfem_thermal_mg; /* the multigrid hierarchy of one heat-conduction problem (vfem_thermal_mg_*) */

const char *vfem_last_error(void);
int  vfem_device_count(void);                 /* number of visible HIP devices (0 => no GPU) */
int  vfem_set_device(int device);
int  vfem_version(void);

/* Per-simulator choice between implementations that agree to rounding (cross-checks in tests/, tuning); the defaults are
   the production kernels.  (Timing ablations that produce wrong results are not part of this library: they exist only in
   the separate `make ablation` build used by tools/.) */
enum {
    VFEM_OPT_APPLY_PLANES = 0,   /* register-staged apply: node planes in flight, 2..4 */
    VFEM_OPT_GS_VARIANT   = 2,   /* 0 production sweeps, 1 plain gather sweeps */
    VFEM_OPT_APPLY_IMPL   = 4,   /* 0 LDS-DMA apply, 1 register-staged apply */
    VFEM_OPT_Q2_IMPL      = 6,   /* vfem_gsim: degree-2 apply 0 marching, 1 dense gather, 2 pencil */
    VFEM_OPT_DMA_CHUNKS   = 7,   /* x-chunks of the marching apply (0 = default: the balanced one-block-per-CU schedule; n > 0: one block per tile and chunk, 8 = its default tiling) */
    VFEM_OPT_DMA_STRIP    = 9,   /* z-remainder strip tiles: 0 off, 1 on, 2 on with the main chunk length */
    VFEM_OPT_DMA_LX       = 11,  /* z tiling of the LDS-DMA apply whose tile boundaries fall on 128-byte lines of the result (tiles advance by 57 columns):
                                    0 off (default: measured 8 % slower at 512^3 -- nine full tiles against eight and a strip --, profiles/r04_apply_lx.txt),
                                    1 where it needs no extra tile (513 = 9 x 57), 2 always */
    VFEM_OPT_GS_PAIR      = 10,  /* level-0 Gauss-Seidel: fused z-colour pairs (1) or one launch per colour (0) */
    VFEM_OPT_L1_DIAG      = 12,  /* level-1 Gauss-Seidel: diagonal blocks precomputed per operator update (1) or inside every sweep (0) */
    VFEM_OPT_GS_RESIDENT  = 13,  /* level-0 Gauss-Seidel: K0 held in SGPRs (1, when K0 has the 36-value structure) or coefficient table (0) */
    VFEM_OPT_L1_SPLIT     = 15,  /* level-1 Gauss-Seidel (degree 1): waves sharing the eight element slots of a node, 1 / 2 / 4 / 8 */
    VFEM_OPT_STENCIL_SPLIT = 18, /* stored-stencil levels: the 27 neighbour blocks of a node shared by three waves (1, default) or one lane (0) */
    VFEM_OPT_GS_MARCH     = 19,  /* level-0 Gauss-Seidel: plane-resident x-marching half sweeps on grids of at least 0.8 M nodes (1, default), always (2),
                                    or the row-streaming kernels (0); the two agree to rounding (different summation order) */
    VFEM_OPT_GS_MARCH_CHUNKS = 20, /* x-chunks of the marching sweep (0 = default) */
    VFEM_OPT_L1_STORED    = 21,  /* level 1 (degree 1): operator evaluated on the fly from the child moduli (0), stored as a 27-point block stencil, 1944 B
                                    per node (1), or stored as half of it using the symmetry, 1008 B per node (2); DESIGN section 3.2 */
    VFEM_OPT_L1_MERGED    = 22,  /* level 1 (degree 1), operator evaluated on the fly: node rows summed per incident element (0), per mirror class of the
                                    child matrices by three waves per node (1), or per class with the two z colours of a row relaxed by one launch (2,
                                    default: the result of 1 bit for bit, half the moduli traffic); 0 and 1 agree to rounding */
    VFEM_OPT_Q2_GS_IMPL   = 16,  /* vfem_gsim: finest-level degree-2 sweep 0 element by element, 1 neighbour node by neighbour node, 2 the same with
                                    the neighbour rows staged through LDS by coalesced loads (default) */
    VFEM_OPT_TRANSFER_AXIS = 17, /* vfem_gsim: restriction / interpolation of 3-D levels above 100 k nodes axis by axis (1, default) or in one pass (0) */
    VFEM_OPT_Q2_L1_VIRTUAL = 14  /* vfem_gsim: level 1 of a degree-2 hierarchy evaluated as sum_f E_f cK0[f] on the fly (1), from stored 81 x 81
                                    element matrices (0), or chosen by their size (2, default: on the fly above 1.5 GB); read by the next
                                    vfem_gmg_update_operators */
};

/* ---- raw device memory helpers (for callers without their own HIP allocator) ---- */
int vfem_malloc(void **ptr, size_t bytes);
int vfem_free(void *ptr);
int vfem_copy_h2d(void *dst, const void *src_host, size_t bytes, void *stream);
int vfem_copy_d2h(void *dst_host, const void *src, size_t bytes, void *stream);
int vfem_copy_d2d(void *dst, const void *src, size_t bytes, void *stream);
int vfem_memset(void *dst, int value, size_t bytes, void *stream);
int vfem_stream_sync(void *stream);

/* ---- simulator: TensorProductSimulator(domain, numElemsPerDim), TPS.hh:252-316 ---- */
int vfem_sim_create(vfem_sim **out, const double bbox_min_host[3], const double bbox_max_host[3],
                    const int64_t nelems_host[3]);
int vfem_sim_destroy(vfem_sim *sim);
int64_t vfem_sim_num_nodes(const vfem_sim *sim);      /* TPS::numNodes,    TPS.hh:1134 */
int64_t vfem_sim_num_elements(const vfem_sim *sim);   /* TPS::numElements, TPS.hh:1137 */

/* ElasticityTensor::setIsotropic via readMaterial/setETensor (TPS.hh:326-339; ElasticityTensor.hh:100-115) */
int vfem_sim_set_isotropic(vfem_sim *sim, double young, double poisson);
/* Any elasticity tensor (orthotropic, anisotropic; TPS::ETensor, ElasticityTensor.hh): D is the 6 x 6 flattened tensor, row-major, in
 * the order xx yy zz yz xz xy of Flattening.hh, holding TENSOR components (a shear row is C_yzyz = mu_yz, no factor 2), so that
 * C_apbq = D[flat(a,p)][flat(b,q)] and K0[(n,a),(m,b)] = vol sum_pq C_apbq int d_p N_n d_q N_m.  Refused: entries that are not
 * finite, asymmetry above 1e-10 of the largest entry, a non-positive diagonal entry (positive definiteness is the caller's to check:
 * ndr_amd.ElasticityTensor does).  Like vfem_sim_set_isotropic it rebuilds K0 and invalidates every operator derived from it; an
 * existing hierarchy rebuilds its coarsened reference matrices at its next operator update.  vfem_sim_set_isotropic keeps its own
 * arithmetic: an isotropic D passed here gives the same K0 to rounding, not bit for bit. */
int vfem_sim_set_elasticity_tensor(vfem_sim *sim, const double D_host[36]);
/* Which tuned kernels the current K0 runs on: update_k0 verifies numerically what each of them assumes about K0 and everything
 * that assumes a property checks its flag (a tensor that fails one runs the general kernel, or the entry point raises).
 * Grid-aligned orthotropic tensors on box voxels set every flag; a rotated (fully anisotropic) tensor sets none. */
enum {
    VFEM_PATH_MODE_SPACE    = 1,  /* the 45-entry mode-space pattern: LDS-DMA / register-staged apply and residual, plane-range apply; else k_apply_gather */
    VFEM_PATH_GS_RESIDENT   = 2,  /* the 36 magnitudes of the resident level-0 sweeps (VFEM_OPT_GS_RESIDENT is ignored without it); else the coefficient table */
    VFEM_PATH_K0_MIRROR     = 4,  /* K0 commutes with the axis reflections: marching level-0 sweep, plane-range sweeps; else the row kernels */
    VFEM_PATH_L1_MIRROR     = 8,  /* vfem_mg_tensor_paths: the coarsened matrices are mirror images: level 1 per mirror class (VFEM_OPT_L1_MERGED, _L1_DIAG,
                                     _L1_SPLIT); else per incident element with all eight matrices */
    VFEM_PATH_Q2_MODE_SPACE = 16  /* vfem_gsim_tensor_paths, degree-2 hexahedra: block-diagonal mode-space K0 (marching / pencil apply); else the dense gather apply */
};
int vfem_sim_tensor_paths(const vfem_sim *sim);
/* E_0 / E_min / gamma properties (VoxelFEM.cc:77-79; TPS.hh:1170-1175) */
int vfem_sim_set_simp(vfem_sim *sim, double E0, double Emin, double gamma);
/* fullDensityElementStiffnessMatrix (TPS.hh:755): 24x24 doubles, row-major, to HOST */
int vfem_sim_set_option(vfem_sim *sim, int key, int value);
int vfem_sim_k0(const vfem_sim *sim, double *K0_host);

/* dirichletMask / dirichletValues properties (TPS.hh:413-442): mask[numNodes] bit c = component c fixed;
 * values[numNodes][3].  Loads: the nodal force field of buildLoadVector (TPS.hh:893-901). */
int vfem_sim_set_dirichlet(vfem_sim *sim, const uint8_t *mask_host, const double *values_host);
int vfem_sim_set_loads(vfem_sim *sim, const double *f, void *stream);   /* f: device [numNodes][3] */
int vfem_sim_build_load_vector(const vfem_sim *sim, double *f, void *stream);

/* setElementDensities / setUniformDensities / getDensities (TPS.hh:456-461, 567-570, 1157-1161).
 * Precomputes the SIMP moduli E_e = Emin + rho^gamma (E0-Emin) once (TPS.hh:725-727). */
int vfem_sim_set_densities(vfem_sim *sim, const double *rho, void *stream);
int vfem_sim_set_uniform_density(vfem_sim *sim, double rho, void *stream);
int vfem_sim_get_densities(const vfem_sim *sim, double *rho, void *stream);

/* applyK (TPS.hh:905-952): out = K(rho) u, Dirichlet conditions ignored.
 * variant 0 = production kernel, 1 = plain gather kernel (cross-check). */
int vfem_sim_apply_k(const vfem_sim *sim, const double *u, double *out, int variant, void *stream);
/* the same operator for the output node planes plane_lo..plane_hi (x index, inclusive) only; other planes of `out` are left
 * untouched.  Used by the slab-decomposed apply to overlap the halo exchange with the interior planes. */
int vfem_sim_apply_k_planes(const vfem_sim *sim, const double *u, double *out, int64_t plane_lo, int64_t plane_hi, void *stream);
/* complianceGradient (TPS.hh:730-751): g_e = -1/2 gamma rho^(gamma-1) (E0-Emin) u_e^T K0 u_e */
int vfem_sim_compliance_gradient(const vfem_sim *sim, const double *u, double *g, void *stream);
/* ComplianceObjective::compliance (TopologyOptimizationObjective.hh:39-41): 1/2 sum f.u, to host */
int vfem_compliance(const vfem_sim *sim, const double *f, const double *u, double *value_host, void *stream);

/* ---- multigrid: tps.multigridSolver(numCoarseningLevels), MG.hh:22-90 ---- */
int vfem_mg_create(vfem_mg **out, vfem_sim *fine, int num_coarsening_levels);
int vfem_mg_destroy(vfem_mg *mg);

/* ---- x-slab decomposition support (one process per GPU).  The reference is single-process; these entry
 * points let a host-side driver (ndr_amd/distributed.py) run the same V-cycle / PCG control flow (MG.hh:447-732) over
 * slabs, with one ghost node plane per interior side at every level.
 *   - vfem_sim_create_padded: vfem_sim_create with element arrays (densities, moduli) that hold extra_lo / extra_hi
 *     additional x-layers in front of / behind the node grid (so that the Galerkin operators of the ghost elements of
 *     coarser levels can be built locally); vfem_sim_set_densities then expects all stored layers.
 *   - vfem_mg_create_slab: local hierarchy with explicit per-level extents and Dirichlet masks (masks_host[l] has the
 *     level's local numNodes bytes); no coarsest-level solver.
 *   - vfem_mg_create_partial: hierarchy on a whole (replicated) grid whose levels < first_active_level are never cycled.
 *   - vfem_mg_smooth_colors: colours [first, first+count) of one sweep (halo exchanges happen between half sweeps).
 *   - vfem_mg_cycle_from_level: V-cycle (x in/out) or full-multigrid cycle (x out) of the residual system at `level`. */
typedef struct {
    int64_t nx;               /* local elements in x (owned layers + one ghost layer per interior side) */
    int64_t elem_extra_lo;    /* extra element x-layers stored in front of the node grid at this level */
    int64_t elem_extra_hi;
    int64_t xshift;           /* level >= 1: (finer level's local plane of this level's local plane 0) = xshift (0 or -1) */
    int32_t xparity;          /* global x-parity of local node plane 0 (Gauss-Seidel colours follow the global grid) */
} vfem_slab_level;
int vfem_sim_create_padded(vfem_sim **out, const double bbox_min_host[3], const double bbox_max_host[3], const int64_t nelems_host[3],
                           int64_t extra_lo, int64_t extra_hi);
int64_t vfem_sim_num_stored_elements(const vfem_sim *sim);
int vfem_mg_create_slab(vfem_mg **out, vfem_sim *fine_local, int n_levels, const vfem_slab_level *levels_host,
                        const uint8_t *const *masks_host);
int vfem_mg_create_partial(vfem_mg **out, vfem_sim *fine, int num_coarsening_levels, int first_active_level);
int vfem_mg_smooth_colors(vfem_mg *mg, int level, double *u, const double *b, int forward, int first, int count, void *stream);
/* Colour group `group` (0: colours 0-3, 1: colours 4-7 of the sweep order = the four colours of one x parity, MG.hh:292-310) on the
 * node planes [plane_lo, plane_hi] of the level's local grid only: a slab rank relaxes its interface planes, starts the halo
 * exchange and relaxes the interior planes meanwhile.  vfem_mg_can_smooth_planes: 1 when the level is swept by the out-of-place
 * marching kernel, which is what makes plane ranges possible. */
int vfem_mg_can_smooth_planes(vfem_mg *mg, int level);
int vfem_mg_smooth_group_planes(vfem_mg *mg, int level, double *u, const double *b, int forward, int group, int64_t plane_lo, int64_t plane_hi,
                                void *stream);
int vfem_mg_cycle_from_level(vfem_mg *mg, int level, double *x, const double *b, int num_smoothing_steps, int fmg, void *stream);
int vfem_mg_num_levels(const vfem_mg *mg);                       /* = numCoarseningLevels + 1 */
int vfem_mg_level_dims(const vfem_mg *mg, int level, int64_t nelems_host[3]);
int64_t vfem_mg_level_num_nodes(const vfem_mg *mg, int level);
int vfem_mg_level_dirichlet_mask(const vfem_mg *mg, int level, uint8_t *mask_host);  /* coarsened masks, MG.hh:57-84 */
int vfem_mg_set_symmetric_gauss_seidel(vfem_mg *mg, int symmetric);                  /* MG.hh:92-94 */
int vfem_mg_tensor_paths(const vfem_mg *mg);          /* vfem_sim_tensor_paths of the simulator | VFEM_PATH_L1_MIRROR of this hierarchy */
/* debug_get_x / debug_get_b (MG.hh:734-735) and the PCG residual handed to it_callback (MG.hh:726-729):
 * device pointer of an internal field; which = 0: m_x[level], 1: m_b[level], 2: PCG residual r (level ignored). */
const double *vfem_mg_field_ptr(const vfem_mg *mg, int which, int level);

/* updateElementStiffnessMatrices + updateBlockKs (MG.hh:415-441): rebuild the coarse operators
 * (Galerkin, MG.hh:604-669) and the coarsest-level factorisation from the current densities. */
int vfem_mg_update_operators(vfem_mg *mg, void *stream);
/* Slab decomposition without a global density field.  export: the Galerkin element matrices (MG.hh:604-669) of `level` (>= 2)
 * for `count_x` element layers, built from this (local) hierarchy's moduli -- the children start at layer `child_first_layer`
 * of the child level's element array (of the fine array for level 2): [count_x * ny * nz][576] doubles.  import: hand a
 * partial (replicated) hierarchy the element matrices of its first active level; its operators are then rebuilt from them. */
int vfem_mg_export_level_ke(vfem_mg *mg, int level, int64_t child_first_layer, int64_t count_x, double *ke_out, void *stream);
int vfem_mg_import_level_ke(vfem_mg *mg, int level, const double *ke, void *stream);
/* MG::applyK(l,u) (MG.hh:353-358), computeResidual (MG.hh:401-413), smoothingMulticoloredGS
 * (MG.hh:336-340; forward != 0 => forward colour/component order), zeroOutDirichletComponents
 * (MG.hh:364-378), restriction (MG.hh:146-161), interpolation / accum_interpolation (MG.hh:116-141),
 * coarsest TPS::solve (TPS.hh:834-865). `level` fields have vfem_mg_level_num_nodes(level) x 3 doubles. */
int vfem_mg_apply_k(vfem_mg *mg, int level, const double *u, double *out, void *stream);
int vfem_mg_residual(vfem_mg *mg, int level, const double *u, const double *b, double *r, void *stream);
int vfem_mg_smooth(vfem_mg *mg, int level, double *u, const double *b, int forward, void *stream);
/* `sweeps` consecutive calls of smoothingMulticoloredGS in one direction, as vcycle makes them (MG.hh:525-528, 546-549).  On the
 * finest level the sweeps are out-of-place marching half sweeps (kernels_gs_march.hip) alternating between u and a scratch
 * vector: an even count ends in u without a copy. */
int vfem_mg_smooth_sweeps(vfem_mg *mg, int level, double *u, const double *b, int forward, int sweeps, void *stream);
int vfem_mg_zero_dirichlet(vfem_mg *mg, int level, double *u, void *stream);
int vfem_mg_restrict(vfem_mg *mg, int fine_level, const double *fine, double *coarse, void *stream);
int vfem_mg_interpolate(vfem_mg *mg, int fine_level, const double *coarse, double *fine, int accumulate, void *stream);
int vfem_mg_coarsest_solve(vfem_mg *mg, const double *b, double *x, void *stream);
/* How the coarsest level is solved exactly (the reference: CHOLMOD, TPS.hh:834-865, at any size).
 *   VFEM_COARSEST_DENSE   the dense n x n inverse applied as a GEMV; refuses more than 40 000 dofs.
 *   VFEM_COARSEST_PLANES  block tridiagonal Cholesky over the x planes (plane_spd.hip): one dense inverse T_j of m = 3 NY NZ dofs per
 *                         node plane, NX m^2 doubles, the solve a forward and a backward march over the planes (about 4 NX launches,
 *                         stream-ordered).  Refuses when the blocks and the factorisation's workspace exceed 8 GiB.
 *   VFEM_COARSEST_AUTO    (default) dense up to 40 000 dofs, plane blocks above.
 * Both treat a fixed dof alike (x = 0 there, b ignored) and agree to rounding (different elimination orders).  Changing the mode
 * discards the kept factorisation; the next solve or vfem_mg_update_operators builds the other one.  An unknown mode is an error.
 * vfem_mg_coarsest_bytes: device bytes the kept factorisation holds (the dense inverse, or the plane blocks with the solver's
 * copy of the coupling entries); 0 while none is kept. */
enum { VFEM_COARSEST_AUTO = 0, VFEM_COARSEST_DENSE = 1, VFEM_COARSEST_PLANES = 2 };
int vfem_mg_set_coarsest_solver(vfem_mg *mg, int mode);
int64_t vfem_mg_coarsest_bytes(const vfem_mg *mg);
/* The factorisation behind the exact coarsest solve (TPS::solve with CholmodFactorizer, TPS.hh:834-865, SparseMatrices.hh:1875-1965),
 * as this library does it: A (n x n doubles, row-major, symmetric positive definite, both triangles) is replaced in place by
 * its inverse (both triangles).  Own blocked Cholesky / triangular inverse / product kernels on `stream`, fixed summation
 * order: the same matrix gives the same inverse bit for bit in every run.  Fails ("not positive definite") on a pivot <= 0. */
int vfem_dense_spd_inverse(int64_t n, double *A, void *stream);

/* ---- direct solve: band Cholesky (band_spd.hip; the reference's TPS::solve, TPS.hh:834-865, factorises with CHOLMOD) ----
 * Band layout of an n x n symmetric positive definite matrix A of half-bandwidth w (A[i][j] = 0 for |i - j| > w), lower band in
 * 64 x 64 tiles: nb = ceil(n / 64) tile rows, bt = ceil(w / 64); tile row I holds bt + 2 tiles of 4096 doubles (row-major).  Slot
 * d = 0..bt is the tile A[64 I + r][64 (I - d) + c] (r, c < 64); slot bt + 1 belongs to the factorisation (its input is ignored, the
 * factor leaves L_II^-1 there).  A[i][j], j <= i <= j + w, is
 *     band[((i / 64) (bt + 2) + i / 64 - j / 64) 4096 + (i % 64) 64 + j % 64],
 * nb (bt + 2) 4096 doubles in all.  Stored entries above the diagonal, outside the band, left of column 0 or in the padding rows
 * i >= n are not read: vfem_band_spd_factor overwrites them (0; 1 on the padding diagonal).
 *   vfem_band_spd_factor  A = L L^T in place (L in the lower band, same layout).  Fails with "band matrix is not positive definite
 *                         (pivot k of n)", k the 1-based index of the first pivot <= 0.  Synchronises the stream.
 *   vfem_band_spd_solve   x [nrhs][n] (right-hand sides in, solutions out) <- A^-1 x from the factor.
 * Own kernels, no atomics, fixed summation order: the same matrix gives the same bits on every run.  The factorisation is 3 launches
 * per tile row (1 in the last), the solve 2 per right-hand side.
 * vfem_sim_direct_solve / vfem_gsim_direct_solve: u = K^-1 f on the free dofs, 0 on the fixed ones (f is ignored there).  The band
 * of the full-size K, a fixed dof's row and column replaced by the identity, is assembled on the device from K0, the SIMP moduli and
 * the Dirichlet mask, factorised, and kept in the handle until the densities, the SIMP parameters, the material or the Dirichlet
 * conditions change (the reference's m_numericFactorizationUpToDate).  Half-bandwidth w = N d + N - 1 dofs, d = sum over the axes of
 * p x the node stride of the axis.  Nonzero Dirichlet values are refused.  *_direct_factorizations: factorisations done so far;
 * *_direct_band_bytes: the band storage a factorisation of this handle holds. */
int vfem_band_spd_factor(int64_t n, int64_t w, double *band, void *stream);
int vfem_band_spd_solve(int64_t n, int64_t w, const double *factor, double *x, int64_t nrhs, void *stream);
int vfem_sim_direct_solve(vfem_sim *sim, const double *f, double *u, void *stream);
int64_t vfem_sim_direct_factorizations(const vfem_sim *sim);
int64_t vfem_sim_direct_band_bytes(const vfem_sim *sim);
int vfem_gsim_direct_solve(vfem_gsim *sim, const double *f, double *u, void *stream);
int64_t vfem_gsim_direct_factorizations(const vfem_gsim *sim);
int64_t vfem_gsim_direct_band_bytes(const vfem_gsim *sim);

/* MG::solve (MG.hh:447-472): numSteps V-cycles (first one a full-multigrid cycle if fmg) on K x = f
 * starting from x (in/out). */
int vfem_mg_solve(vfem_mg *mg, double *x, const double *f, int num_steps, int num_smoothing_steps,
                  int stiffness_updated, int zero_dirichlet, int fmg, void *stream);

/* preconditionedConjugateGradient (MG.hh:679-732).  x is in/out (initial guess u -> solution).
 * residual_cb, if non-NULL, is called after every iteration with (it, ||r||) on the calling thread
 * (MultigridComplianceObjective::residual_cb, TopologyOptimizationObjective.hh:87-89, 101). */
typedef void (*vfem_residual_cb)(void *user, int iteration, double residual_norm);
int vfem_mg_pcg(vfem_mg *mg, double *x, const double *b, int max_iter, double tol,
                int mg_iterations, int mg_smoothing_iterations, int fmg,
                vfem_residual_cb residual_cb, void *cb_user,
                int *iterations_out_host, double *relres_out_host, void *stream);

/* A rank's whole slab-decomposed MG-PCG solve in one call (DistributedMGSolver.pcg of ndr_amd/distributed.py, i.e.
 * preconditionedConjugateGradient / vcycle / fullMultigrid of MG.hh:486-553, 679-732 over x-slabs).  `local` = the rank's
 * vfem_mg_create_slab hierarchy (levels 0 .. first_replicated_level), `replicated` = the vfem_mg_create_partial hierarchy of the
 * whole grid that every rank cycles identically from that level down.  All work vectors are the caller's (device memory):
 * per level the iterate / right-hand side / residual of the local node grid, the replicated level's two vectors, two PCG vectors of
 * the local fine grid and 8 doubles of scalars.  The two operations only the caller can do are callbacks, invoked on the calling
 * thread with the stream's work enqueued so far ordered before them:
 *   halo(user, level, field, left, right, phase): refresh the ghost planes of `field` (one of the vectors handed in) from the
 *        left / right neighbour; phase 0 = exchange and return, 1 = start (the interior planes are swept meanwhile), 2 = finish;
 *   allreduce(user, buf, n): sum n doubles at `buf` (device) over the ranks, in place.
 * Both return 0 on success.  Operators must be current (vfem_mg_update_operators on both hierarchies, plus the caller's own
 * assembly of the replicated level for sharded densities). */
typedef struct {
    int64_t n_planes, plane_nodes;      /* local node planes of the level, nodes per plane */
    int64_t first_owned, last_owned;    /* local planes this rank computes (ghost planes lie outside) */
    int64_t xoffn;                      /* global plane index of local plane 0 */
    int32_t gl, gr;                     /* ghost planes towards the left / right neighbour (0 or 1) */
    double *x, *b, *r;                  /* work vectors [n_planes * plane_nodes][3] (r unused on the last level) */
} vfem_dist_level;
typedef int (*vfem_halo_fn)(void *user, int level, double *field, int left, int right, int phase);
typedef int (*vfem_allreduce_fn)(void *user, double *device_buffer, int64_t n);
int vfem_mg_pcg_slab(vfem_mg *local, vfem_mg *replicated, int first_replicated_level, const vfem_dist_level *levels_host, int rank,
                     int world, double *replicated_x, double *replicated_b, double *x, const double *b, double *work_d, double *work_Ad,
                     double *scalars8, int max_iter, double tol, int mg_iterations, int mg_smoothing_iterations, int full_multigrid,
                     int overlap_sweeps, vfem_halo_fn halo, vfem_allreduce_fn allreduce, void *callback_user,
                     vfem_residual_cb residual_cb, void *residual_user, int *iterations_out, double *relres_out, void *stream);

/* ---- generic path: every instantiation other than the tuned <1,1,1> one.  TensorProductSimulator<1,1> / <2,2> (2-D, plane
 * stress, ElasticityTensor.hh:100-133; the reference binds <1,1>, VoxelFEM.cc:226) and <2,2,2>; MultigridSolver of the same
 * degrees (MG.hh, templates generic in Degrees...).  Nodal fields [numNodes][N], node grid (p*ne+1) per axis, last axis
 * fastest; Dirichlet mask 1 byte per node (bit c = component c).  Same semantics as the vfem_sim_ / vfem_mg_ entry points of the
 * same name. */
int vfem_gsim_create(vfem_gsim **out, int dim, int degree, const double *bbox_min_host, const double *bbox_max_host,
                     const int64_t *nelems_host);
/* slab decomposition (no reference counterpart; the domain decomposition north_star asks for, 3-D only): a simulator whose
 * density / modulus arrays hold elem_extra_lo / _hi further element layers below / above the node grid along x.
 * vfem_gsim_set_densities then takes all stored layers (vfem_gsim_num_stored_elements values, x slowest); every other entry
 * point sees the elements of the node grid only. */
int vfem_gsim_create_padded(vfem_gsim **out, int dim, int degree, const double *bbox_min_host, const double *bbox_max_host,
                            const int64_t *nelems_host, int64_t elem_extra_lo, int64_t elem_extra_hi);
int64_t vfem_gsim_num_stored_elements(const vfem_gsim *sim);
int vfem_gsim_destroy(vfem_gsim *sim);
int64_t vfem_gsim_num_nodes(const vfem_gsim *sim);
int64_t vfem_gsim_num_elements(const vfem_gsim *sim);
int vfem_gsim_ke_size(const vfem_gsim *sim);                       /* N * (p+1)^N */
int vfem_gsim_set_isotropic(vfem_gsim *sim, double young, double poisson);
/* vfem_sim_set_elasticity_tensor for the generic path: D is n x n row-major, n = 6 in 3-D (xx yy zz yz xz xy) and n = 3 in 2-D
 * (xx yy xy; a plane-stress material arrives already reduced).  K0 is integrated by the same Gauss loop as the isotropic one. */
int vfem_gsim_set_elasticity_tensor(vfem_gsim *sim, const double *D_host, int n);
int vfem_gsim_tensor_paths(const vfem_gsim *sim);     /* VFEM_PATH_Q2_MODE_SPACE or 0 */
int vfem_gsim_set_simp(vfem_gsim *sim, double E0, double Emin, double gamma);
int vfem_gsim_k0(const vfem_gsim *sim, double *K0_host);           /* ke x ke row-major */
int vfem_gsim_set_dirichlet(vfem_gsim *sim, const uint8_t *mask_host, const double *values_host);
int vfem_gsim_set_densities(vfem_gsim *sim, const double *rho, void *stream);
int vfem_gsim_get_densities(const vfem_gsim *sim, double *rho, void *stream);
int vfem_gsim_set_option(vfem_gsim *sim, int key, int value);
int vfem_gsim_apply_k(const vfem_gsim *sim, const double *u, double *out, void *stream);              /* TPS.hh:905-952 */
int vfem_gsim_compliance_gradient(const vfem_gsim *sim, const double *u, double *g, void *stream);    /* TPS.hh:730-751 */
int vfem_gsim_compliance(const vfem_gsim *sim, const double *f, const double *u, double *value_host, void *stream);  /* 1/2 f.u */
int vfem_gmg_create(vfem_gmg **out, vfem_gsim *fine, int num_coarsening_levels);                      /* MG.hh:22-90 */
/* The same three pieces as vfem_mg_create_slab / vfem_mg_create_partial / vfem_mg_{export,import}_level_ke for the generic path
 * (degree-2 hexahedra over the GPUs of a node, BASELINE config 5).  A rank's local hierarchy keeps two ghost element layers
 * (2 p node planes) towards each neighbour on every level: the restriction to an interface node reaches 2 p - 1 fine planes
 * to either side.  vfem_slab_level.xshift here: local plane of level l-1 = 2 * (local plane of level l) + xshift (<= 0);
 * xparity must be 0 (slabs start at even global elements on every distributed level).  Element matrices are ke x ke doubles
 * per element (81 x 81 for degree 2). */
int vfem_gmg_create_slab(vfem_gmg **out, vfem_gsim *fine_local, int n_levels, const vfem_slab_level *levels_host,
                         const uint8_t *const *masks_host);
int vfem_gmg_create_partial(vfem_gmg **out, vfem_gsim *fine, int num_coarsening_levels, int first_active_level);
int vfem_gmg_smooth_colors(vfem_gmg *mg, int level, double *u, const double *b, int forward, int first, int count, void *stream);
int vfem_gmg_cycle_from_level(vfem_gmg *mg, int level, double *x, const double *b, int num_smoothing_steps, int fmg, void *stream);
int vfem_gmg_export_level_ke(vfem_gmg *mg, int level, int64_t child_first_layer, int64_t count_x, double *ke_out, void *stream);
/* import: into the first active level of a replicated hierarchy -- level `first_active_level` of vfem_gmg_create_partial, or
 * level 0 of an ordinary hierarchy created on the coarse grid itself (its level 0 then applies the imported matrices instead of
 * E_e K0; this is how the slab driver keeps every global object at the size of the first replicated level) */
int vfem_gmg_import_level_ke(vfem_gmg *mg, int level, const double *ke, void *stream);
int vfem_gmg_destroy(vfem_gmg *mg);
int vfem_gmg_num_levels(const vfem_gmg *mg);
int vfem_gmg_level_dims(const vfem_gmg *mg, int level, int64_t nelems_host[3]);
int64_t vfem_gmg_level_num_nodes(const vfem_gmg *mg, int level);
int vfem_gmg_level_dirichlet_mask(const vfem_gmg *mg, int level, uint8_t *mask_host);
int vfem_gmg_set_symmetric_gauss_seidel(vfem_gmg *mg, int symmetric);
int vfem_gmg_update_operators(vfem_gmg *mg, void *stream);                                            /* MG.hh:415-425 */
int vfem_gmg_apply_k(vfem_gmg *mg, int level, const double *u, double *out, void *stream);
int vfem_gmg_residual(vfem_gmg *mg, int level, const double *u, const double *b, double *r, void *stream);
int vfem_gmg_smooth(vfem_gmg *mg, int level, double *u, const double *b, int forward, void *stream);  /* MG.hh:285-340 */
int vfem_gmg_zero_dirichlet(vfem_gmg *mg, int level, double *u, void *stream);
int vfem_gmg_restrict(vfem_gmg *mg, int fine_level, const double *fine, double *coarse, void *stream);
int vfem_gmg_interpolate(vfem_gmg *mg, int fine_level, const double *coarse, double *fine, int accumulate, void *stream);
int vfem_gmg_solve(vfem_gmg *mg, double *x, const double *f, int num_steps, int num_smoothing_steps, int stiffness_updated,
                   int zero_dirichlet, int full_multigrid, void *stream);                             /* MG.hh:447-472 */
int vfem_gmg_pcg(vfem_gmg *mg, double *x, const double *b, int max_iter, double tol, int mg_iterations, int mg_smoothing_iterations,
                 int full_multigrid, vfem_residual_cb residual_cb, void *cb_user, int *iterations_out, double *relres_out,
                 void *stream);                                                                       /* MG.hh:679-732 */

/* ---- design-update path, element-grid arrays [n0][n1][n2] fp64 (2-D grids: n2 = 1) ----
 * SmoothingFilter apply / backprop (TopologyOptimizationFilter.hh:105-162; transpose != 0 => A^T), ProjectionFilter apply /
 * backprop (:55-79), mean for TotalVolumeConstraint (TopologyOptimizationConstraint.hh:21-34), and the OC candidate step
 * clip(x0 sqrt(dJ/(dc lambda)), max(x0-m,0), min(x0+m,1)) of OCOptimizer::step (OptimalityCriterion.hh:47-50); where
 * dJ/(dc lambda) < 0 the candidate is the lower edge max(x0-m,0) (the reference: NaN).  vfem_mean refuses n < 1. */
int vfem_box_filter(const int64_t n_host[3], int radius, const double *in, double *out, int transpose, void *stream);
/* The box filter on an x-slab: `in` holds the layers [x_first, x_first + n_local[0]) of a grid of nx_global x-layers (n_local[1],
 * n_local[2] are the global y, z extents); the local layers [out_first, out_first + out_layers) are written to `out` (out_layers
 * layers).  Neighbourhoods and row counts are clipped to the global grid, so the result equals the matching slice of
 * vfem_box_filter on the whole grid bit for bit.  Refused (nothing read): a negative radius, local or output layers outside
 * their ranges, and a written layer whose neighbour layers inside the global grid are not all local (too few ghost layers). */
int vfem_box_filter_slab(const int64_t n_local[3], int64_t x_first, int64_t nx_global, int64_t out_first, int64_t out_layers,
                         int radius, const double *in, double *out, int transpose, void *stream);
/* The box filter on a PERIODIC grid (a homogenisation cell): out_i = (2 radius + 1)^-3 sum over the offsets in [-radius, radius]^3
 * of in[(i + offset) mod n].  Every offset counts once, also where the window is wider than the grid and wraps onto an element
 * again; an axis of extent 1 is therefore the identity (2-D grids).  The operator is symmetric (its own transpose: apply and
 * backprop are the same call), translation invariant and preserves the mean.  in and out are two arrays.  Refused: a negative
 * radius, and a window of more than 2^31 - 1 offsets. */
int vfem_box_filter_periodic(const int64_t n_host[3], int radius, const double *in, double *out, void *stream);
int vfem_projection(int64_t n, double beta, const double *x, double *out, void *stream);
int vfem_projection_backprop(int64_t n, double beta, const double *g, const double *vars, double *out, void *stream);
int vfem_oc_candidate(int64_t n, const double *x0, const double *dJ, const double *dc, double lambda, double move, double *out,
                      void *stream);
int vfem_mean(int64_t n, const double *x, double *mean_host, void *stream);
/* LangelaarFilter (TopologyOptimizationFilter.hh:164-278; the reference fixes eps = 1e-4, p = 40, q = 40 - 1.58).  The layer
 * axis is n[2], so 2-D grids [nx][ny] are passed as {nx, 1, ny} (same flat order).  apply writes out and the smax cache
 * (smax = 1 on layer 0); backprop takes both caches of the apply it differentiates plus `vars`, and returns
 * grad = lambda dsmin_dx1(vars, smax) with the adjoint march over n[2] layers (the reference's computeLagrangeMultipliers,
 * :211-226, bounds it by n[1] instead; identical when n[1] == n[2] and in 2-D).  A support whose sum of out^p is 0 (below the
 * smallest normal double) contributes 0, where the reference computes 0 * inf.  work: caller-provided device scratch of
 * 2 n[0] n[1] doubles.  Both run ceil(n[2] / 8) kernel launches on `stream`. */
int vfem_langelaar_apply(const int64_t n_host[3], double eps, double p, double q, const double *in, double *out, double *smax,
                         void *stream);
int vfem_langelaar_backprop(const int64_t n_host[3], double eps, double p, double q, const double *g, const double *vars,
                            const double *out, const double *smax, double *work, double *grad, void *stream);

/* ---- Fourier-feature MLP density field: networks.MLP (networks.py:128-185), out_features = 1 ----
 * n_layers counts Linear layers as the reference does: Linear(2 es, nn), (n_layers - 2) x Linear(nn, nn), Linear(nn, 1).
 * Weights are handed over as fp32 arrays (host or device memory) in torch layout ([out][in] row-major) and converted to fp16:
 *   B [es][3] (MLP.B, already multiplied by `scale`), W_first [nn][2 es], W_hidden [(n_layers-2)][nn][nn],
 *   biases [(n_layers-1)][nn] (first layer, then hidden layers), w_out [nn], b_out.
 * Requirements of the MFMA tiling: es % 32 == 0, nn % 32 == 0, nn <= 512. */
int vfem_mlp_create(vfem_mlp **out, int embedding_size, int n_neurons, int n_layers, int sigmoid_output);
int vfem_mlp_destroy(vfem_mlp *mlp);
/* options of one network: VFEM_MLP_OPT_BWD_TERMS = 3 (default; every product of the backward pass is hi hi + hi lo + lo hi of split
 * fp16 operands: the reference's fp32 autograd to rounding) or 1 (hi hi only in the weight-gradient GEMMs, three times fewer MFMAs) */
#define VFEM_MLP_OPT_BWD_TERMS 1
/* VFEM_MLP_OPT_KEEP_FIRST = 1: a reference-precision GRID forward keeps the first layer's activations (2 KB per voxel: 68.7 GB at
 * 512 x 256 x 256, at most 96 GB, dropped silently when the allocation fails), and vfem_mlp_backward_grid* of the same grid, voxel range
 * and weights start from them instead of recomputing the first layer (two thirds of the forward's products).  0 (default): nothing is kept.
 * Results are the same bit for bit. */
#define VFEM_MLP_OPT_KEEP_FIRST 2
int vfem_mlp_set_option(vfem_mlp *mlp, int key, int value);
int vfem_mlp_load_weights(vfem_mlp *mlp, const float *B, const float *W_first, const float *W_hidden, const float *biases,
                          const float *w_out, float b_out);
/* forward on an explicit coordinate list [nvox][3] fp32 (device); either output pointer may be NULL */
int vfem_mlp_forward(vfem_mlp *mlp, const float *coords, int64_t nvox, float *out_f32, double *out_f64, void *stream);
/* forward on the regular grid of utils.get_mgrid (utils.py:35-53): n[d] points linspace(lo[d], hi[d]) incl. both ends,
 * flattened z-fastest = the solver's element order (train_xdg.py:245-247, 287) */
int vfem_mlp_forward_grid(vfem_mlp *mlp, const int64_t n_host[3], const double lo_host[3], const double hi_host[3],
                          float *out_f32, double *out_f64, void *stream);
/* the same for the voxels [first_voxel, first_voxel + num_voxels) of that grid (flat index, z fastest); outputs are indexed from
 * the start of the range.  A rank of an x-slab decomposition evaluates its own planes with this (the field needs no exchange). */
int vfem_mlp_forward_grid_range(vfem_mlp *mlp, const int64_t n_host[3], const double lo_host[3], const double hi_host[3],
                                int64_t first_voxel, int64_t num_voxels, float *out_f32, double *out_f64, void *stream);
/* The same two forwards in the reference's own arithmetic: fp32 features with accurate sin / cos of 2 pi x . B, fp32 GEMMs
 * (networks.py:170-185 runs in torch's default dtype).  Parity mode: several times slower than the fused fp16-operand kernel,
 * which moves the densities by ~1e-3 relative. */
int vfem_mlp_forward_f32(vfem_mlp *mlp, const float *coords, int64_t nvox, float *out_f32, double *out_f64, void *stream);
int vfem_mlp_forward_grid_range_f32(vfem_mlp *mlp, const int64_t n_host[3], const double lo_host[3], const double hi_host[3],
                                    int64_t first_voxel, int64_t num_voxels, float *out_f32, double *out_f64, void *stream);
/* Training (what torch.autograd does for networks.MLP in train_xdg.py:282-329): gradients of a scalar loss wrt the
 * parameters given g_out[v] = dL/d(out[v]) (device, fp32).  Outputs are overwritten, fp32, same layouts as vfem_mlp_load_weights:
 * dW1 [nn][2 es], dWh [n_layers-2][nn][nn], dbias [n_layers-1][nn], dwout [nn], dbout [1].  Split fp16 operands (hi + lo) on the
 * matrix pipe with fp32 accumulation = the reference's fp32 autograd to rounding; no library GEMM, the first layer's Fourier
 * features are regenerated inside the weight-gradient kernel.  `loss_scale` multiplies g_out before it enters fp16 and is
 * divided out of the results (power of two recommended). */
int vfem_mlp_backward(vfem_mlp *mlp, const float *coords, int64_t nvox, const float *g_out, float loss_scale, float *dW1,
                      float *dWh, float *dbias, float *dwout, float *dbout, void *stream);
int vfem_mlp_backward_grid(vfem_mlp *mlp, const int64_t n_host[3], const double lo_host[3], const double hi_host[3],
                           const float *g_out, float loss_scale, float *dW1, float *dWh, float *dbias, float *dwout, float *dbout,
                           void *stream);
/* the same for the voxels [first_voxel, first_voxel + num_voxels) of the grid (g_out indexed from the start of the range): the
 * partial gradient a rank of the slab decomposition contributes; the ranks' results are summed by one all-reduce */
int vfem_mlp_backward_grid_range(vfem_mlp *mlp, const int64_t n_host[3], const double lo_host[3], const double hi_host[3],
                                 int64_t first_voxel, int64_t num_voxels, const float *g_out, float loss_scale, float *dW1,
                                 float *dWh, float *dbias, float *dwout, float *dbout, void *stream);
/* torch.optim.Adam update (amsgrad off, weight_decay 0) of one fp32 parameter tensor, in place; step counts from 1 */
int vfem_adam_step(int64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float lr, float beta1,
                   float beta2, float eps, int step, void *stream);

/* ---- periodic homogenisation of a voxel cell (TPPeriodicHomogenization.hh; DESIGN "Periodic homogenisation") ----
 * Handle-free, degree-1 elements, dim = 2 or 3.  Every entry point takes the cell and its element constants:
 *   nelems_host[dim]   elements per axis (>= 2 each); periodic node (i_0, .., i_{dim-1}), last axis fastest, is the unknown of every
 *                      grid node congruent to it modulo nelems, so there are prod(nelems) periodic nodes; node 0 is pinned (w = 0)
 *   K0_host [ke][ke]   full-density element matrix, ke = dim 2^dim, local nodes with the last axis fastest, dof = dim node + component
 *   L_host  [ke][S]    L[:, q] = element load of the constant stress C : e_q, S = 3 (xx yy xy) or 6 (xx yy zz yz xz xy), e_q with
 *                      0.5 on both off-diagonal entries of a shear case
 *   D_host  [S][S]     flattened tensor (row q = C : e_q), vol = voxel volume
 *   E (device) [prod(nelems)]  element moduli E_min + rho^gamma (E_0 - E_min), last axis fastest
 * W (device) is [S][periodic nodes][dim].
 * vfem_hom_apply: W_out[s] = K_per W_in[s], K_per the periodic stiffness matrix with the pin's row and column replaced by the identity.
 * vfem_hom_solve_cells: K_per w_q = - sum_e E_e L[:, q] for all S cases together by block-Jacobi PCG from w = 0; a case is frozen
 *   once |r| / |b| <= tol, the host tests convergence once every 8 iterations; error (with the worst case's residual in the message,
 *   the two output arrays filled) when a case has not converged after max_iter iterations, or ("breakdown in strain case q") when
 *   every case froze and one is short of tol because its r . z is not positive: a singular cell (a node with only zero moduli
 *   around it, non-finite moduli); the residual reported for a case with a non-finite |b| is NaN.  Results are bit-identical run to run.
 * vfem_hom_tensor: Eh[q][r] = (1 / cell_volume) sum_e E_e (w_{q,e} . L[:, r] + vol D[q][r]) to the host (not symmetrised).
 * vfem_hom_tensor_gradient: G (device) [prod(nelems)][S][S] = dE[e] / cell_volume *
 *   (w_{q,e}^T K0 w_{r,e} + w_{q,e} . L[:, r] + L[:, q] . w_{r,e} + vol D[q][r]), upper triangle mirrored; dE (device, dE_e / drho_e)
 *   may be NULL for a factor 1.  sum_e E_e G_e (dE = NULL) = Eh at the exact solution.
 * vfem_hom_tensor_gradient_contract: g (device) [prod(nelems)], g[e] = sum_{q,r} C_host[q][r] G[e][q][r] with the G that
 *   vfem_hom_tensor_gradient writes for the same arguments, which is never formed: the vector-Jacobian product of the tensor (C a
 *   weight matrix, 2 (Eh - E*) / |E*|^2, or the incoming gradient of an autograd node).  G_e is symmetric, so only (C + C^T) / 2
 *   acts: C and C^T give the same bits, an antisymmetric C gives 0.  One thread per element, no atomics: bit-identical run to run.
 *   Refused: a non-finite C. */
int vfem_hom_apply(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host, const double *D_host, double vol,
                   const double *E, const double *W_in, double *W_out, void *stream);
int vfem_hom_solve_cells(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host, const double *D_host,
                         double vol, const double *E, double *W, double tol, int max_iter, int *iterations_out_host,
                         double *relres_out_host, void *stream);
int vfem_hom_tensor(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host, const double *D_host, double vol,
                    const double *E, const double *W, double cell_volume, double *Eh_host, void *stream);
int vfem_hom_tensor_gradient(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host, const double *D_host,
                             double vol, const double *E, const double *W, double cell_volume, const double *dE, double *G,
                             void *stream);
int vfem_hom_tensor_gradient_contract(int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host,
                                      const double *D_host, double vol, const double *E, const double *W, double cell_volume,
                                      const double *dE, const double *C_host, double *g, void *stream);

/* ---- multigrid-preconditioned PCG for the cell problems (DESIGN "Periodic homogenisation") ----
 * vfem_hom_mg_create builds the hierarchy of one cell from the arguments every vfem_hom_* call starts with; the handle keeps the
 * pointer E (device), which must stay valid and unchanged until vfem_hom_mg_destroy.  Level 0 is the cell (matrix-free); level
 * l + 1 has n_d / 2 periodic nodes per axis and stores the Galerkin operator P^T A_l P, P the periodic N-linear interpolation.  A
 * level is coarsened while every n_d is even and at least 4 and fewer than max_coarsenings coarsenings are made (negative: no
 * cap).  The last level is solved exactly by a dense inverse: error when it has more dofs than that solver takes (the message names
 * the level sizes and the limit).  On every level node 0 is pinned: the operator's row and column of node 0 are the identity.
 * Vectors of level l (device) are [S][nodes_l][dim].
 * vfem_hom_mg_level_dims: n_out[dim] = nodes per axis of level l.  vfem_hom_mg_bytes: device memory the handle holds.
 * vfem_hom_mg_level_apply: W_out = A_l W_in.
 * vfem_hom_mg_smooth: one 2^dim-colour block Gauss-Seidel sweep of A_l X = B on X (colour = parity of the node index per axis, axis 0
 *   the most significant bit), colours ascending (forward != 0) or descending; every n_d of the level must be even.
 * vfem_hom_mg_restrict: coarse (level l + 1) = P^T fine (level l), zero at node 0.  vfem_hom_mg_prolong_add: fine += P coarse, the
 *   coarse value of node 0 counting as zero.
 * vfem_hom_mg_vcycle: X = V-cycle(B) on level 0 from a zero initial guess: `smoothing` ascending sweeps, the coarse correction,
 *   `smoothing` descending sweeps; a symmetric positive definite operator.  A one-level hierarchy applies the exact inverse.
 * vfem_hom_mg_solve_cells: vfem_hom_solve_cells with z = V-cycle(r) as the preconditioner; same freeze criterion, outputs and errors.
 * Results are bit-identical run to run. */
int vfem_hom_mg_create(vfem_hom_mg **out, int dim, const int64_t *nelems_host, const double *K0_host, const double *L_host,
                       const double *D_host, double vol, const double *E, int max_coarsenings, void *stream);
int vfem_hom_mg_destroy(vfem_hom_mg *h);
int vfem_hom_mg_num_levels(vfem_hom_mg *h);
int64_t vfem_hom_mg_bytes(vfem_hom_mg *h);
int vfem_hom_mg_level_dims(vfem_hom_mg *h, int l, int64_t *n_out);
int vfem_hom_mg_level_apply(vfem_hom_mg *h, int l, const double *W_in, double *W_out, void *stream);
int vfem_hom_mg_smooth(vfem_hom_mg *h, int l, double *X, const double *B, int forward, void *stream);
int vfem_hom_mg_restrict(vfem_hom_mg *h, int l, const double *fine, double *coarse, void *stream);
int vfem_hom_mg_prolong_add(vfem_hom_mg *h, int l, const double *coarse, double *fine, void *stream);
int vfem_hom_mg_vcycle(vfem_hom_mg *h, const double *B, double *X, int smoothing, void *stream);
int vfem_hom_mg_solve_cells(vfem_hom_mg *h, double *W, double tol, int max_iter, int smoothing, int *iterations_out_host,
                            double *relres_out_host, void *stream);

/* ---- element stresses of a degree-1 grid: field, p-norm measure, adjoint load, density gradient ----
 * Handle-free, dim = 2 (plane stress) or 3.  Every grid entry point starts with
 *   nelems_host[dim]   elements per axis (>= 1 each), last axis fastest; the node grid has nelems + 1 nodes per axis
 *   h_host[dim]        the voxel's edge lengths (> 0)
 *   D_host [S][S]      flattened tensor, S = 3 (xx yy xy) or 6 (xx yy zz yz xz xy), TENSOR components (shear columns count twice)
 * u, a, lambda (device) are [nodes][dim]; m, dm, dE, vm, g (device) are [elements]; strain, stress (device) are [elements][S].
 * Device pointers need 8-byte alignment only.  Element e with nodal values u_e:
 *   eps_e = mean over the element of sym(grad u) (TensorProductSimulator::elementStrain, the strain at the centroid),
 *   sigma_e = m[e] C : eps_e, vm_e = von Mises stress of sigma_e (2-D: sqrt(sxx^2 - sxx syy + syy^2 + 3 sxy^2)).
 * vfem_stress_fields: writes whichever of strain, stress, vm is not NULL (at least one); m may be NULL when only strain is asked for.
 * vfem_stress_pnorm: J = (sum_i vm[i]^P)^(1/P) over n values, computed as vmax (sum (vm / vmax)^P)^(1/P) so that it cannot
 *   overflow; J = 0 when vmax = 0.  J and (unless NULL) vmax go to the host.  Fixed summation order: bit-identical run to run.
 * vfem_stress_adjoint_load: a = dJ/du at fixed m: a[node j] = sum over the incident elements of
 *   (vm_e / J)^(P-1) m_e Bbar_j^T (C : dvm/dsigma at sigma_e), 0 where vm_e = 0, and 0 at the components the mask fixes (mask, device,
 *   1 byte per node, bit c = component c; may be NULL).  J is the measure of the same u, m, P (J = 0: a = 0).  work (device) is
 *   [elements][S] doubles of scratch: an element kernel leaves there what each element sends to its nodes, then one thread per node
 *   gathers from its incident elements in a fixed order.  No atomics: bit-identical run to run.
 * vfem_stress_pnorm_gradient: g[e] = (vm_e / J)^(P-1) dm[e] vm_e / m_e - dE[e] lambda_e^T K0 u_e: the derivative of J with respect
 *   to a design variable rho_e with dm = dm/drho, dE = d(stiffness modulus)/drho, lambda the solution of K lambda = a, K0_host
 *   [ke][ke] the full-density element matrix (ke = dim 2^dim, dof = dim node + component).
 * Refused before any device call: NULL pointers, dim not 2 or 3, extents < 1, h <= 0, non-finite D or K0, a non-finite P or P < 1,
 * a negative or non-finite J. */
int vfem_stress_fields(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *m,
                       const double *u, double *strain, double *stress, double *vm, void *stream);
int vfem_stress_pnorm(int64_t n, const double *vm, double P, double *J_host, double *vmax_host, void *stream);
int vfem_stress_adjoint_load(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *m,
                             const double *u, double J, double P, const uint8_t *mask, double *work, double *a, void *stream);
int vfem_stress_pnorm_gradient(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *K0_host,
                               const double *m, const double *dm, const double *dE, const double *u, const double *lambda, double J,
                               double P, double *g, void *stream);

/* ---- Method of Moving Asymptotes (Svanberg 1987 / 2007 with a_i = 0, d_i = 1, c_i = c) ----
 * min f_0(x) subject to f_i(x) <= 0, i = 1 .. m (1 <= m <= 8), xmin <= x <= xmax, one convex separable subproblem per step.
 * x, L, U, xmin, xmax, g0, xnew (device) are [n]; g (device) is [m][n], row i the gradient of f_i; f, b, lambda, y and the outputs
 * of the dual evaluation are host arrays of m (hess: m x m row-major).  Device pointers need 8-byte alignment only (16-byte
 * aligned buffers are read 16 bytes per lane).  With xm = max(xmax - xmin, 1e-5), per variable and per gradient g:
 *   p = (U - x)^2 (1.001 g+ + 0.001 g- + 1e-5 / xm),  q = (x - L)^2 (0.001 g+ + 1.001 g- + 1e-5 / xm),
 *   alpha = max(xmin, L + 0.1 (x - L), x - move xm),  beta = min(xmax, U - 0.1 (U - x), x + move xm),
 *   x_j(lambda) = clamp((sqrt(P) L + sqrt(Q) U) / (sqrt(P) + sqrt(Q)), alpha, beta),  P = p_0 + lambda . p,  Q = q_0 + lambda . q,
 *   y_i = max(0, lambda_i - c),  b_i = sum_j (p_ij / (U - x) + q_ij / (x - L)) - f_i.
 * vfem_mma_asymptotes: L, U in place for step `iter` (from 1).  Steps 1 and 2: x -+ asyinit xm.  Later, with
 *   s = (x - xold1)(xold1 - xold2) and the factor asyincr (s > 0), asydecr (s < 0) or 1: L = x - factor (xold1 - L), kept within
 *   [x - 10 xm, x - 0.01 xm]; U mirrored.  xold1, xold2 may be NULL in steps 1 and 2.
 * vfem_mma_dual_eval: one fused pass at lambda >= 0.  W = sum_j (P / (U - x_j) + Q / (x_j - L)) - lambda . b - 0.5 sum y_i^2,
 *   grad_i = dW/dlambda_i = G_i - b_i - y_i with G_i = sum_j (p_ij / (U - x_j) + q_ij / (x_j - L)),  scale_i = G_i + |b_i| + y_i,
 *   hess = -d2W/dlambda2 = sum over the j strictly inside (alpha, beta) of h_ij h_kj / psi''_j, plus 1 on the diagonal where
 *   lambda_i > c.  Fixed summation order, no atomics: bit-identical run to run.
 * vfem_mma_subproblem: computes b from f (host, the values f_i(x)), maximises W over lambda >= 0 and writes xnew = x(lambda).
 *   It stops when max_i |r_i| <= tol scale_i, r_i = grad_i where lambda_i > 0, else max(grad_i, 0); if max_iter Newton iterations
 *   do not get there it fails and names the residual.  lambda_out [m] is required; y_out [m], iters_out, residual_out (the largest
 *   |r_i| / scale_i) may be NULL.
 * Refused before any device call: n < 1, m outside 1 .. 8, NULL pointers, move <= 0, asyinit <= 0, asydecr outside (0, 1),
 * asyincr < 1, tol <= 0, max_iter < 1, c < 0, a negative or non-finite lambda, a non-finite f or b, and an xnew that overlaps an input. */
int vfem_mma_asymptotes(int64_t n, int iter, const double *x, const double *xold1, const double *xold2, const double *xmin,
                        const double *xmax, double asyinit, double asyincr, double asydecr, double *L, double *U, void *stream);
int vfem_mma_dual_eval(int64_t n, int m, const double *x, const double *L, const double *U, const double *xmin, const double *xmax,
                       double move, const double *g0, const double *g, const double *b_host, double c, const double *lambda_host,
                       double *W_host, double *grad_host, double *scale_host, double *hess_host, void *stream);
int vfem_mma_subproblem(int64_t n, int m, const double *x, const double *L, const double *U, const double *xmin, const double *xmax,
                        double move, const double *f_host, const double *g0, const double *g, double c, double tol, int max_iter,
                        double *xnew, double *lambda_out, double *y_out, int *iters_out, double *residual_out, void *stream);

/* ---- natural frequencies of a degree-1 grid: mass operator, block operations, density gradient ----
 * Handle-free, dim = 2 or 3.  Every grid entry point starts with nelems_host[dim] and h_host[dim] as the element-stress section
 * has them.  A block of vectors (device) is [column][node][dim]: every column is a vector of the simulators; for the two block
 * operations a block is [column][n].  m, dE, dm, g (device) are [elements].  Device pointers need 8-byte alignment only.
 * The consistent mass matrix of a unit-density voxel, M0, is the tensor product of the 1-D h_d / 6 [[2, 1], [1, 2]], the identity
 * across components;  M(m) = sum_e m[e] M0;  P zeroes the components a node mask fixes (mask, device, 1 byte per node, bit c =
 * component c; may be NULL: P = I).
 * vfem_modal_mass_apply: Y_c = P M(m) P X_c for the ncols (1 .. 24) columns; one thread per node reads its multipliers once for
 *   all columns.  Y must not overlap X.
 * vfem_modal_project: X_c = P X_c in place.
 * vfem_block_gram: G = A^T B (ka x kb row-major, ka, kb in 1 .. 24) of the blocks A [ka][n], B [kb][n], by per-workgroup partials
 *   and one finishing kernel.  G (device) and G_host may each be NULL, not both: with G_host the matrix is copied to the host and
 *   the stream is synchronised, without it the call is asynchronous.
 * vfem_block_combine: B_j = sum_i C_host[i][j] A_i, i ascending, for A [kin][n], B [kout][n], C_host kin x kout row-major (kin,
 *   kout in 1 .. 24).  B must not overlap A.  Asynchronous.
 * vfem_modal_gradient: g[e] = sum_i (cK_host[i] dE[e] phi_ie^T K0 phi_ie + cM_host[i] dm[e] phi_ie^T M0 phi_ie) over the nmodes
 *   (1 .. 8) columns of Phi; K0_host [ke][ke] as in vfem_stress_pnorm_gradient.
 * No atomics, fixed summation order: results are bit-identical run to run.
 * Refused before any device call: NULL pointers (but mask), dim not 2 or 3, extents < 1, h <= 0, a column count out of range,
 * n < 1, non-finite coefficients or K0, and an output that overlaps an input. */
int vfem_modal_mass_apply(int dim, const int64_t *nelems_host, const double *h_host, const double *m, const uint8_t *mask, int ncols,
                          const double *X, double *Y, void *stream);
int vfem_modal_project(int dim, const int64_t *nelems_host, const double *h_host, const uint8_t *mask, int ncols, double *X,
                       void *stream);
int vfem_block_gram(int64_t n, int ka, const double *A, int kb, const double *B, double *G, double *G_host, void *stream);
int vfem_block_combine(int64_t n, int kin, int kout, const double *A, const double *C_host, double *B, void *stream);
int vfem_modal_gradient(int dim, const int64_t *nelems_host, const double *h_host, int nmodes, const double *K0_host,
                        const double *cK_host, const double *cM_host, const double *dE, const double *dm, const double *Phi, double *g,
                        void *stream);

/* ---- linearised buckling of a degree-1 grid: geometric stiffness, adjoint load, density gradient ----
 * Handle-free, dim = 2 or 3.  Every entry point starts with nelems_host[dim], h_host[dim] and the flattened tensor D_host [S][S] as
 * the element-stress section has them.  Blocks, the node mask and the alignment rule are those of the natural-frequency section;
 * mG, dmG, dE, g (device) are [elements], u, v, a (device) are [node][dim].
 * The consistent geometric stiffness of element e is the same scalar matrix on every component, linear in its displacements:
 *   K_G,e[(n, a), (m, b)] = delta_ab mG[e] sum_j u_ej T_j[n][m],  T_j[n][m] = int_e grad N_n^T (C : B_j(x)) grad N_m dV,
 * B_j the strain of a unit displacement at dof j; the 2^dim dim tables T_j are formed on the host from D_host and h_host by two
 * Gauss points per axis (exact), uploaded once per (device, dim, h, D) and kept for the life of the process (at most 8 of them).
 * vfem_buckling_geom_apply: Y_c = P K_G(mG, u) P X_c for the ncols (1 .. 24) columns; one thread per node forms its 3^dim couplings
 *   once for all columns and components.  Y must not overlap X or u.
 * vfem_buckling_adjoint_load: a = sum_i c_host[i] d(phi_i^T K_G(mG, u) phi_i)/du over the nmodes (1 .. 8) columns of Phi, zero where
 *   the mask fixes a component: element e gives mG[e] phi_ie^T T_j phi_ie (summed over the dim components of the mode) at dof j.
 * vfem_buckling_gradient: g[e] = dmG[e] sum_i cG_host[i] sum_j u_ej phi_ie^T T_j phi_ie
 *   + dE[e] (sum_i cK_host[i] phi_ie^T K0 phi_ie - v_e^T K0 u_e); K0_host [ke][ke] as in vfem_stress_pnorm_gradient.
 * No atomics, fixed summation order: results are bit-identical run to run.  vfem_buckling_geom_apply and
 * vfem_buckling_adjoint_load are asynchronous (but for the first call with a new h or D, which uploads the tables);
 * vfem_buckling_gradient uploads K0 and synchronises the stream, as vfem_modal_gradient does.
 * Refused before any device call: NULL pointers (but mask), dim not 2 or 3, extents < 1, h <= 0, a column or mode count out of
 * range, a non-finite tensor, K0 or coefficient, and an output that overlaps an input. */
int vfem_buckling_geom_apply(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *mG,
                             const double *u, const uint8_t *mask, int ncols, const double *X, double *Y, void *stream);
int vfem_buckling_adjoint_load(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, const double *mG,
                               const uint8_t *mask, int nmodes, const double *c_host, const double *Phi, double *a, void *stream);
int vfem_buckling_gradient(int dim, const int64_t *nelems_host, const double *h_host, const double *D_host, int nmodes,
                           const double *K0_host, const double *cG_host, const double *cK_host, const double *dmG, const double *dE,
                           const double *u, const double *v, const double *Phi, double *g, void *stream);

/* ---- load cases of a degree-1 grid: design-dependent loads and the gradient of a sum of compliances ----
 * Handle-free, dim = 2 or 3.  Both entry points start with nelems_host[dim] and h_host[dim] as the natural-frequency section has
 * them; the node mask and the alignment rule are those of that section.  m, E, dE, dm, g (device) are [elements], f_in, f_out
 * (device) are [node][dim], U (device) is the block [case][node][dim].  An element pattern has ke = dim 2^dim entries, dof = dim
 * node + component in the local node order of K0:
 *   Lb[(n, a)] = vol / 2^dim g[a]  (the body force of an acceleration g on a unit mass density),
 *   Lt[(n, a)] = sum_q sigma*[a][q] s_nq vol / (2^(dim-1) h_q),  sigma* = C : eps*, s_nq = +-1  (int B^T sigma* of an eigenstrain).
 * vfem_loads_assemble: f_out = P (f_in + sum_e m[e] Lb + sum_e E[e] Lt).  Lb_host with m, or Lt_host with E, may be NULL, not both
 *   pairs; f_in and mask may be NULL (zero; P = I).  f_out may be f_in; it overlaps nothing else.  One thread per node gathers its
 *   2^dim elements in ascending local-node order; the patterns travel in the kernel arguments.  Asynchronous.
 * vfem_loads_gradient: g[e] = dE[e] sum_i cK_host[i] u_ie^T K0 u_ie + dm[e] sum_i cB_host[i] Lb_i . u_ie
 *   + dE[e] sum_i cT_host[i] Lt_i . u_ie over the ncases (1 .. 8) columns of U; K0_host [ke][ke] as in vfem_stress_pnorm_gradient,
 *   Lb_host and Lt_host [ncases][ke].  Lb_host, cB_host and dm are NULL together, and so are Lt_host and cT_host.  One thread per
 *   element reads its multipliers once for all cases.  It uploads K0 and the patterns and synchronises the stream, as
 *   vfem_modal_gradient does.  g overlaps no input.
 * No atomics, fixed summation order: results are bit-identical run to run.
 * Refused before any device call: NULL pointers where one is required, dim not 2 or 3, extents < 1, h <= 0, ncases out of range,
 * non-finite patterns, K0 or coefficients, and the overlaps named above. */
int vfem_loads_assemble(int dim, const int64_t *nelems_host, const double *h_host, const double *Lb_host, const double *Lt_host,
                        const double *m, const double *E, const uint8_t *mask, const double *f_in, double *f_out, void *stream);
int vfem_loads_gradient(int dim, const int64_t *nelems_host, const double *h_host, int ncases, const double *K0_host,
                        const double *cK_host, const double *cB_host, const double *cT_host, const double *Lb_host,
                        const double *Lt_host, const double *dE, const double *dm, const double *U, double *g, void *stream);

/* ---- steady heat conduction on a degree-1 grid: scalar operator, solvers, gradient, flux ----
 * Handle-free, dim = 2 or 3.  Every entry point starts with nelems_host[dim]; the two that need the voxel's edge lengths take
 * h_host[dim] next.  The unknown is one temperature per node, nodes and elements numbered as in the natural-frequency section.
 * kappa, dkappa, q, g (device) are [elements]; b, x, diag, f_in, f_out, T (device) are [nodes]; X, Y, A, B (device) are blocks
 * [column][node]; flux (device) is [elements][dim]; fixed (device) is 1 byte per node, not 0 = the temperature is fixed at zero,
 * and may be NULL (no fixed node).  Device pointers need 8-byte alignment only.  Kc0_host [2^dim][2^dim] is the conductivity
 * matrix of a full-density voxel, int grad N_a^T k grad N_b dV, in the local node order of K0 (axis 0 the most significant bit).
 * The operator is  A(kappa) = P (sum_e kappa[e] Kc0) P + (I - P),  P zeroing the fixed nodes: their rows and columns are the identity.
 * vfem_thermal_apply: Y_c = A X_c for the ncols (1 .. 8) columns; one thread per node forms its 3^dim couplings once for all
 *   columns.  Y overlaps no input.  Asynchronous.
 * vfem_thermal_diagonal: diag = the diagonal of A (1 at a fixed node).  Asynchronous.
 * vfem_thermal_source: f_out = P (f_in + sum_e q[e] vol / 2^dim), vol the voxel's volume: a nodal source and a volumetric source per
 *   element.  q or f_in may be NULL, not both; f_out may be f_in and overlaps nothing else.  Asynchronous.
 * vfem_thermal_band_assemble: the lower band of A in the tile layout of vfem_band_spd_factor, with n = nodes and w = the sum of the
 *   node strides (1 + (ne[1] + 1) in 2-D, 1 + (ne[2] + 1) + (ne[1] + 1)(ne[2] + 1) in 3-D); band holds nb (bt + 2) 4096 doubles and every
 *   entry of its slots 0 .. bt is written.  vfem_band_spd_factor and vfem_band_spd_solve do the rest.  Asynchronous.
 * vfem_thermal_pcg: conjugate gradients with the Jacobi preconditioner on A x = b from the x given, until |r| / |b| <= tol (the
 *   recurrence residual).  The host reads the residual once before the first iteration and then every 8 iterations, so the count
 *   it returns is 0, a multiple of 8 or max_iter (after a breakdown: the iteration of the breakdown); b = 0 gives x = 0 in 0 iterations.  iterations_out_host and relres_out_host are
 *   written on success and on the two failures: max_iter reached ("not converged after ..."), and a p . Ap that is not positive
 *   ("breakdown at iteration ...": a singular operator or non-finite data; x is then unspecified).  Both messages carry the
 *   residual.  x overlaps no input.  Synchronises the stream.
 * vfem_thermal_gradient: g[e] = dkappa[e] sum_i c_host[i] a_ie^T Kc0 b_ie over the ncols (1 .. 8) column pairs of A and B; B may be
 *   A.  One thread per element.  g overlaps no input.  Asynchronous.
 * vfem_thermal_flux: flux[e] = -kappa[e] k grad T at the centre of element e, k_host [dim][dim] the conductivity tensor.  Asynchronous.
 * No atomics, fixed summation order: results are bit-identical run to run.
 * Refused before any device call: NULL pointers where one is required, dim not 2 or 3, extents < 1, h <= 0, a non-finite Kc0, tensor
 * or coefficient, a column count out of range, tol <= 0, max_iter < 1, and the overlaps named above. */
int vfem_thermal_apply(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                       int ncols, const double *X, double *Y, void *stream);
int vfem_thermal_diagonal(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                          double *diag, void *stream);
int vfem_thermal_source(int dim, const int64_t *nelems_host, const double *h_host, const double *q, const uint8_t *fixed,
                        const double *f_in, double *f_out, void *stream);
int vfem_thermal_band_assemble(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                               double *band, void *stream);
int vfem_thermal_pcg(int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa, const uint8_t *fixed,
                     const double *b, double *x, double tol, int max_iter, int *iterations_out_host, double *relres_out_host,
                     void *stream);
int vfem_thermal_gradient(int dim, const int64_t *nelems_host, int ncols, const double *Kc0_host, const double *c_host,
                          const double *dkappa, const double *A, const double *B, double *g, void *stream);
int vfem_thermal_flux(int dim, const int64_t *nelems_host, const double *h_host, const double *k_host, const double *kappa,
                      const double *T, double *flux, void *stream);

/* ---- multigrid-preconditioned CG for the scalar conduction operator ----
 * vfem_thermal_mg_create builds the hierarchy of one grid, one set of element multipliers and one mask from the arguments of
 * vfem_thermal_apply; the handle keeps the pointers kappa and fixed (device; fixed may be NULL), which must stay valid and
 * unchanged until vfem_thermal_mg_destroy.  Level 0 is the grid (matrix-free from kappa); level l + 1 exists while every extent of
 * level l is even and at least 4 elements and max_coarsenings (negative: no limit) allows it, and has half the elements per axis.
 * A coarse node is fixed exactly when the fine node it coincides with is.  With I_l the N-linear interpolation and F_l the 0/1
 * diagonal of the free nodes, P_l = F_l I_l F_{l+1},  A'_0 = F_0 (sum_e kappa[e] Kc0) F_0,  A'_{l+1} = P_l^T A'_l P_l,
 * A_l = A'_l + (I - F_l); levels >= 1 store A'_l as a 3^dim-point stencil.  The coarsest level is inverted densely and may have at
 * most 40 000 nodes: create fails with a message that lists the level sizes otherwise, before anything large is allocated, and with
 * "breakdown at the coarsest level ..." when that matrix is not positive definite (a singular operator).  A grid with an odd
 * extent is a one-level hierarchy, whose cycle is the exact inverse.  Create synchronises the stream.
 * vfem_thermal_mg_level_dims: n_out[dim] = elements per axis of level l.  vfem_thermal_mg_bytes: device memory the handle holds.
 * vfem_thermal_mg_level_fixed: fixed_out (device, one byte per node of level l) = the level's mask, 0 or 1.
 * vfem_thermal_mg_level_apply: Y = A_l X on the nodes of level l.
 * vfem_thermal_mg_smooth: one sweep of A_l X = B on X over the 2^dim colours (the parity of the node index per axis, axis 0 the most
 *   significant bit), ascending (forward) or descending: x += (b - A_l x) / diag A_l on every node of the colour.
 * vfem_thermal_mg_restrict: coarse (level l + 1) = P_l^T fine (level l).  vfem_thermal_mg_prolong_add: fine += P_l coarse; fixed fine
 *   nodes are not written.
 * vfem_thermal_mg_vcycle: X = V-cycle(B) on level 0 from a zero iterate: `smoothing` ascending sweeps, the residual, the coarse
 *   correction, `smoothing` descending sweeps; the coarsest level is solved exactly.  A symmetric positive definite operator.
 * vfem_thermal_mg_pcg: vfem_thermal_pcg with z = V-cycle(r) as the preconditioner; the same stopping rule, outputs and two errors,
 *   but the host reads the residual after every iteration, so the count it returns is exact.  Synchronises the stream.
 * All gathers in a fixed order, no atomics: bit-identical run to run.  Device pointers need 8-byte alignment only.
 * Refused before any device call: a NULL handle or pointer, a level out of range (restrict and prolong_add: l + 1 must exist),
 * smoothing outside [1, 16], tol <= 0, max_iter < 1, an output that overlaps its input, and at create what vfem_thermal_apply refuses. */
int vfem_thermal_mg_create(vfem_thermal_mg **out, int dim, const int64_t *nelems_host, const double *Kc0_host, const double *kappa,
                           const uint8_t *fixed, int max_coarsenings, void *stream);
int vfem_thermal_mg_destroy(vfem_thermal_mg *h);
int vfem_thermal_mg_num_levels(vfem_thermal_mg *h);
int64_t vfem_thermal_mg_bytes(vfem_thermal_mg *h);
int vfem_thermal_mg_level_dims(vfem_thermal_mg *h, int l, int64_t *n_out);
int vfem_thermal_mg_level_fixed(vfem_thermal_mg *h, int l, uint8_t *fixed_out, void *stream);
int vfem_thermal_mg_level_apply(vfem_thermal_mg *h, int l, const double *X, double *Y, void *stream);
int vfem_thermal_mg_smooth(vfem_thermal_mg *h, int l, double *X, const double *B, int forward, void *stream);
int vfem_thermal_mg_restrict(vfem_thermal_mg *h, int l, const double *fine, double *coarse, void *stream);
int vfem_thermal_mg_prolong_add(vfem_thermal_mg *h, int l, const double *coarse, double *fine, void *stream);
int vfem_thermal_mg_vcycle(vfem_thermal_mg *h, const double *B, double *X, int smoothing, void *stream);
int vfem_thermal_mg_pcg(vfem_thermal_mg *h, const double *b, double *x, double tol, int max_iter, int smoothing,
                        int *iterations_out_host, double *relres_out_host, void *stream);

/* ---- thermo-elastic coupling of a degree-1 grid: a temperature field as a load, its transpose, its gradient ----
 * Handle-free, dim = 2 or 3.  The three entry points start as the load-case section's do; the node mask, the numbering and the
 * alignment rule are those of that section.  E, dE, g_in, g_out (device) are [elements], T and q (device) are [node], f_in, f_out
 * (device) are [node][dim], U (device) is the block [case][node][dim].  A coupling matrix G (host) is row-major [ke = dim 2^dim]
 * [npe = 2^dim], dof = dim node + component in the local node order of K0:
 *   G[(n, a)][m] = int beta_aq dN_n/dx_q N_m dV,  beta = C : alpha  (the temperature is interpolated inside the element).
 * vfem_thermoelastic_load: f_out = P (f_in + sum_e E[e] G (T_e - T_ref)).  f_in and mask may be NULL (zero; P = I).  f_out may be
 *   f_in; it overlaps nothing else.  One thread per node gathers its 2^dim elements in ascending local-node order; G travels in
 *   the kernel arguments.  Asynchronous.
 * vfem_thermoelastic_adjoint_source: q = P_T sum_i a_host[i] sum_e E[e] G_i^T u_ie over the ncases (1 .. 8) columns of U, G_host
 *   [ncases][ke][npe]: the transpose of the load, the source of the thermal adjoint.  fixed (one byte per node, nonzero = fixed
 *   temperature; may be NULL) zeroes q there.  Cases, then elements, then rows ascending.  q overlaps no input.  It uploads the
 *   matrices and synchronises the stream, as vfem_loads_gradient does.
 * vfem_thermoelastic_gradient: g_out[e] = g_in[e] + dE[e] sum_i a_host[i] u_ie^T G_i (T_e - Tref_host[i]).  g_in may be NULL
 *   (zero); g_out may be g_in and overlaps nothing else.  One thread per element reads its temperatures once for all cases.  It
 *   uploads the matrices and synchronises the stream.
 * No atomics, fixed summation order: results are bit-identical run to run.
 * Refused before any device call: NULL pointers where one is required, dim not 2 or 3, extents < 1, h <= 0, ncases out of range,
 * non-finite matrices, coefficients or reference temperatures, and the overlaps named above. */
int vfem_thermoelastic_load(int dim, const int64_t *nelems_host, const double *h_host, const double *G_host, double T_ref,
                            const double *E, const double *T, const uint8_t *mask, const double *f_in, double *f_out, void *stream);
int vfem_thermoelastic_adjoint_source(int dim, const int64_t *nelems_host, const double *h_host, int ncases, const double *a_host,
                                      const double *G_host, const double *E, const double *U, const uint8_t *fixed, double *q,
                                      void *stream);
int vfem_thermoelastic_gradient(int dim, const int64_t *nelems_host, const double *h_host, int ncases, const double *a_host,
                                const double *G_host, const double *Tref_host, const double *dE, const double *T, const double *U,
                                const double *g_in, double *g_out, void *stream);

/* ---- transient heat conduction on a degree-1 grid: capacity operator, solver, time-accumulated gradient ----
 * Handle-free, dim = 2 or 3; grid, numbering, mask and alignment rule are those of the steady section.  cap, dcap (device) are
 * [elements] beside kappa, dkappa.  The capacity matrix of a voxel is M[a][b] = m[popcount(a xor b)], a function of the number of axes
 * along which two local nodes differ, so it is passed as m_host[dim + 1] (consistent: capacity vol 2^(dim - d) / 6^dim; lumped: vol /
 * 2^dim at d = 0 and zero elsewhere).  The two-term operator is
 *   A(Ka, mb) = P (sum_e kappa[e] Ka + sum_e cap[e] M(mb)) P + iota (I - P),
 * and the caller folds the scalars of the theta-scheme into Ka_host [2^dim][2^dim] and mb_host [dim + 1]: Ka = theta Kc0, mb = m / dt
 * for the system operator of a step, Ka = -(1 - theta) Kc0, mb = m / dt for its right-hand side.
 * vfem_transient_apply: Y_c = A X_c + P b_c for the ncols (1 .. 8) columns; b (a block like X) may be NULL.  identity = iota, 0 or 1:
 *   what a fixed node keeps of its own value.  With b and identity = 0 this is the right-hand side of a step in one pass.  One
 *   thread per node forms its 3^dim couplings of both terms once for all columns.  Y overlaps no input.  Asynchronous.
 * vfem_transient_diagonal: diag = the diagonal of A with iota = 1 (1 at a fixed node).  Asynchronous.
 * vfem_transient_band_assemble: the lower band of A with iota = 1, in the layout and with the n, w of vfem_thermal_band_assemble.
 *   Asynchronous.
 * vfem_transient_pcg: vfem_thermal_pcg on A(Ka, mb) x = b with iota = 1: the same loop, stopping rule, outputs and two errors; the
 *   operator is positive definite without a fixed node when theta, dt and the capacities are positive.  Synchronises the stream.
 * vfem_transient_gradient: with T and Lam (device) the blocks [steps + 1][node] of a march and of its adjoint (row 0 of Lam is not read),
 *   g[e] = -sum_{n = 1 .. steps} (dcap[e] / dt lam_e^n . M(m) (T_e^n - T_e^(n-1)) + dkappa[e] lam_e^n . Kc0 (theta T_e^n + (1 - theta) T_e^(n-1))).
 *   One thread per element marches the steps with the temperatures of the step before in registers; steps has no upper limit but
 *   memory.  g overlaps no input.  Asynchronous.
 * vfem_transient_mg_create: vfem_thermal_mg_create for A(Ka, mb): the handle it returns has the two-term operator (iota = 1) as its
 *   level 0, matrix-free from kappa and cap, which it keeps as it keeps kappa and fixed; the Galerkin levels, the coarsest solve and
 *   every vfem_thermal_mg_* call (level_apply, smooth, vcycle, pcg, destroy, ...) are those of that section, unchanged.  One hierarchy
 *   serves every step of a march and of its adjoint.  Create synchronises the stream.
 * No atomics, fixed summation order: results are bit-identical run to run.
 * Refused before any device call: NULL pointers where one is required, dim not 2 or 3, extents < 1, a non-finite Ka, Kc0, mb or m,
 * identity not 0 or 1, a column count out of range, steps < 1, dt <= 0, theta outside [0.5, 1], tol <= 0, max_iter < 1, and the
 * overlaps named above. */
int vfem_transient_apply(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                         const double *cap, const uint8_t *fixed, int identity, int ncols, const double *X, const double *b, double *Y,
                         void *stream);
int vfem_transient_diagonal(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                            const double *cap, const uint8_t *fixed, double *diag, void *stream);
int vfem_transient_band_assemble(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                                 const double *cap, const uint8_t *fixed, double *band, void *stream);
int vfem_transient_pcg(int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host, const double *kappa,
                       const double *cap, const uint8_t *fixed, const double *b, double *x, double tol, int max_iter,
                       int *iterations_out_host, double *relres_out_host, void *stream);
int vfem_transient_mg_create(vfem_thermal_mg **out, int dim, const int64_t *nelems_host, const double *Ka_host, const double *mb_host,
                             const double *kappa, const double *cap, const uint8_t *fixed, int max_coarsenings, void *stream);
int vfem_transient_gradient(int dim, const int64_t *nelems_host, int64_t steps, const double *Kc0_host, const double *m_host, double dt,
                            double theta, const double *dkappa, const double *dcap, const double *T, const double *Lam, double *g,
                            void *stream);

/* ---- timers: BENCHMARK_* registry (MeshFEM GlobalBenchmark.hh / Timer.hh; VoxelFEM.cc:245-255) ---- */
int vfem_timers_reset(void);
int vfem_timers_report(char *buf_host, size_t buf_len);

#ifdef __cplusplus
}
#endif
#endif /* VFEM_H */
