// Device code shared by the MLP kernel files (kernels_mlp.hip, kernels_mlp_x3.hip, kernels_mlp_bwd.hip).  Training is only correct
// when the backward pass sees what the forward pass multiplied: k_mlp_dw regenerates the Fourier features of k_mlp_forward_x3 bit for
// bit (sincos_f32 at the coordinates of voxel_xyz), and the sign of unscale_lo is the ReLU mask.  Hence one definition of each, here.
#pragma once
#include <hip/hip_runtime.h>

#include "mlp_args.h"

namespace vfem {
namespace mlp {

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef float f16_t __attribute__((ext_vector_type(16)));

// tiling of the split-operand kernels (k_mlp_forward_x3, k_mlp_backward_x3)
constexpr int TM = 64;                    // voxels per block
constexpr int MAXN = 512;                 // hidden width limit
constexpr int HS = MAXN + 8;              // halves per activation row (16-byte pad: conflict-free ds_read_b128)

// split operand: x = hi + lo 2^-11 (kernels_mlp_x3.hip)
constexpr float LO_SCALE = 2048.f, LO_INV = 1.f / 2048.f;
__device__ __forceinline__ void split(float x, _Float16 &hi, _Float16 &lo) {
    hi = (_Float16) x;
    lo = (_Float16) ((x - (float) hi) * LO_SCALE);
}
// the low half without its 2^11 scale (what the backward pass's products take).  A nonzero half never becomes zero: an activation
// of 1e-9 has hi = 0 and lives in its low half alone, whose unscaled value underflows fp16 -- and "h > 0" is the ReLU mask of the
// backward pass (the smallest subnormal, 6e-8, stands in: its value is immaterial, its sign is not)
__device__ __forceinline__ _Float16 unscale_lo(_Float16 ls) {
    const float f = (float) ls;
    _Float16 u = (_Float16) (f * LO_INV);
    if ((float) u == 0.f && f != 0.f) u = (_Float16) (f > 0.f ? 5.9604645e-8f : -5.9604645e-8f);
    return u;
}

// sin and cos of an fp32 argument together, to fp32 rounding (max error 9.2e-8 for |t| <= 1000, tools/ numpy check in DESIGN 3.5; numpy's own
// fp32 sin: 7e-8): one Cody-Waite reduction by pi/2 in three fma steps (pi/2 = c1 + c2 + c3), the cephes single-precision minimax
// polynomials on [-pi/4, pi/4], quadrant by the low bits of n.  ~25 instructions for the pair; two library calls (sinf, cosf) were ~90
// and made feature generation 27 % of the SIMD time of the forward kernel (profiles/r04_mlp_x3_pmc.json: 1686 vector instructions per voxel).
__device__ __forceinline__ void sincos_f32(float t, float &sn, float &cs) {
    const float n = __builtin_rintf(t * 0.636619772367581343f);
    float y = fmaf(-n, 1.5707963705062866f, t);
    y = fmaf(-n, -4.371138828673793e-08f, y);
    y = fmaf(-n, -1.7763568394002505e-15f, y);
    const float z = y * y;
    float ps = fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    ps = fmaf(ps, z, -1.6666654611e-1f);
    const float s = fmaf(ps * z, y, y);
    float pc = fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    pc = fmaf(pc, z, 4.166664568298827e-2f);
    const float c = fmaf(z * z, pc, fmaf(-0.5f, z, 1.0f));
    const int q = (int) n;
    const float a = (q & 1) ? c : s, b = (q & 1) ? s : c;
    sn = (q & 2) ? -a : a;
    cs = ((q + 1) & 2) ? -b : b;
}

// coordinates of voxel v of the chunk: from the explicit list, or generated on the regular grid
__device__ __forceinline__ void voxel_xyz(const MlpArgs &a, long long v, float x[3]) {
    if (a.coords) { x[0] = a.coords[3 * v]; x[1] = a.coords[3 * v + 1]; x[2] = a.coords[3 * v + 2]; return; }
    v += a.v_offset;
    const long long k = v % a.gn[2], j = (v / a.gn[2]) % a.gn[1], i = v / ((long long) a.gn[2] * a.gn[1]);
    x[0] = a.glo[0] + a.gstep[0] * (float) i;
    x[1] = a.glo[1] + a.gstep[1] * (float) j;
    x[2] = a.glo[2] + a.gstep[2] * (float) k;
}

}  // namespace mlp
}  // namespace vfem
