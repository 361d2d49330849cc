// degrade.hip -- the blind-SR degradation of the training inputs, LR = (HR * k) downsampled + n, around the existing
// bicubic: a per-sample separable Gaussian blur of the uint8 HR batch (ofasr_degrade_blur_u8) and per-sample additive
// noise on a uint8 LR batch (ofasr_degrade_noise_u8).  Both are exact integer functions; the host statement is
// degrade.py (blur_np, noise_np) and the kernels equal it bit for bit.  One int32 table [n, 48] serves both:
//   0, 1   r_x, r_y      2  a      3  gray      4  stream      5  0
//   6..26  t_x, the tap for offset d at 16 + d, zero outside the radius       27..47  t_y likewise (at 37 + d)
//
// Blur.  h[y][x] = (sum_{|d| <= r_x} t_x[d] * p[y][clamp(x + d, 0, W - 1)] + 2^13) >> 14, then
//        out[y][x] = (sum_{|d| <= r_y} t_y[d] * h[clamp(y + d, 0, H - 1)][x] + 2^13) >> 14.
// The taps are non-negative and sum to 2^14 (degrade.blur_taps), so both are bytes without a clip and the sums stay
// below 2^22.  Whatever the table holds, a radius is clamped to [0, max_radius] and nothing is read outside the plane.
// One workgroup owns a DG_TW x DG_TH output tile of one plane.  It stages the tile plus a DG_HALO halo on every side
// in LDS as bytes, each byte from an address clamped into the plane -- the clamp IS the border rule, and a row of the
// halo beyond the plane is a copy of the edge row, so its horizontal result is the edge row's -- writes the
// horizontally filtered rows (tile columns only, halo rows included) back to LDS, and runs the vertical pass from there.
// Every global load is a byte load issued by every lane from a clamped address; lanes past the end of a staging loop
// repeat its last element, so no load stands under a lane-dependent branch.  The taps are uniform per sample: lanes 0 ..
// 41 read them into LDS once per workgroup.  A lane owns 4 adjacent output columns of one row: one dword store where the
// launch layer found W % 4 == 0 and dst 4-byte aligned (VEC), guarded byte stores otherwise.  src needs no alignment.
//
// Noise.  One Philox4x32-10 call per element (Salmon et al., SC'11; multipliers D2511F53, CD9E8D57, key increments
// 9E3779B9, BB67AE85): counter (y * W + x, channel, stream, scale), key (seed_lo, seed_hi).  With s the sum of the 16
// output bytes, c = s - 2040; out = clip(v + ((a * c + 2^15) >> 16), 0, 255), arithmetic shift.  |a * c| <= |a| * 2040:
// a is clamped to [0, 2^19], so the product fits int32 whatever the table holds.  With gray != 0 all three channels use
// channel 0's call.  a = 0 is a copy (the branch is uniform over the workgroup: a sample is grid.y).  A plane is
// contiguous, so y * W + x is the flat index: a lane owns 4 adjacent flat indices of each of the 3 planes.  VEC (H * W % 4
// == 0, src and out_u8 4-byte aligned, out_f32 16-byte aligned): one dword load and one dword / float4 store per plane;
// otherwise byte loads from clamped indices and guarded element stores.  A lane reads its own 12 bytes before it writes
// them, and no lane reads another's: out_u8 == src is allowed.  The fp32 output is __fdiv_rn(v, 255.0f), ToTensor's bits.
#include "ofasr_common.h"

namespace ofasr {

static const int DG_TW = 64, DG_TH = 32;            // the output tile of one workgroup
static const int DG_HALO = 10;                      // = the largest radius
static const int DG_SW = DG_TW + 2 * DG_HALO, DG_SH = DG_TH + 2 * DG_HALO;
static const int DG_THREADS = 256;
static const int DG_COLS = 48, DG_TX = 16;          // t_y's centre stands 2 * DG_HALO + 1 columns after t_x's

__device__ __forceinline__ int dg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid: (x: tile column, y: tile row, z: plane = 3 * sample + channel)
template <bool VEC>
__global__ void __launch_bounds__(DG_THREADS) degrade_blur_kernel(const uint8_t* __restrict__ src,
                                                                  const int* __restrict__ table, int H, int W,
                                                                  int max_radius, uint8_t* __restrict__ dst) {
    __shared__ uint8_t s_in[DG_SH * DG_SW];
    __shared__ uint8_t s_h[DG_SH * DG_TW];
    __shared__ int s_tx[2 * DG_HALO + 1], s_ty[2 * DG_HALO + 1];
    const int tid = (int)threadIdx.x;
    const long long plane = blockIdx.z;
    const int* row = table + (plane / 3) * DG_COLS;
    const int rx = dg_clampi(row[0], 0, max_radius), ry = dg_clampi(row[1], 0, max_radius);
    const uint8_t* p = src + plane * ((long long)H * W);
    const int x0 = (int)blockIdx.x * DG_TW, y0 = (int)blockIdx.y * DG_TH;
    {
        const int k = tid < 2 * (2 * DG_HALO + 1) ? tid : 2 * (2 * DG_HALO + 1) - 1;
        const int v = row[DG_TX - DG_HALO + k];                          // columns 6 .. 47, t_x then t_y
        if (k < 2 * DG_HALO + 1) s_tx[k] = v;
        else s_ty[k - (2 * DG_HALO + 1)] = v;
    }
    for (int i0 = 0; i0 < DG_SH * DG_SW; i0 += DG_THREADS) {
        const int i = i0 + tid < DG_SH * DG_SW ? i0 + tid : DG_SH * DG_SW - 1;   // the tail repeats the last byte
        const int ly = i / DG_SW, lx = i - ly * DG_SW;
        const int gy = dg_clampi(y0 - DG_HALO + ly, 0, H - 1), gx = dg_clampi(x0 - DG_HALO + lx, 0, W - 1);
        s_in[i] = p[(long long)gy * W + gx];
    }
    __syncthreads();
    for (int i = tid; i < DG_SH * DG_TW; i += DG_THREADS) {              // DG_SH * DG_TW is a multiple of DG_THREADS
        const int ly = i / DG_TW, lx = i - ly * DG_TW;
        const uint8_t* q = s_in + ly * DG_SW + lx + DG_HALO;
        int acc = 1 << 13;
        for (int d = -rx; d <= rx; ++d) acc += s_tx[DG_HALO + d] * (int)q[d];
        s_h[i] = (uint8_t)(acc >> 14);
    }
    __syncthreads();
    for (int g = tid; g < DG_TH * DG_TW / 4; g += DG_THREADS) {
        const int ly = g / (DG_TW / 4), lx = (g - ly * (DG_TW / 4)) * 4;
        const uint8_t* q = s_h + (ly + DG_HALO) * DG_TW + lx;
        int acc[4] = {1 << 13, 1 << 13, 1 << 13, 1 << 13};
        for (int d = -ry; d <= ry; ++d) {
            const int t = s_ty[DG_HALO + d];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] += t * (int)q[d * DG_TW + k];
        }
        const int y = y0 + ly, x = x0 + lx;
        if (y < H && x < W) {
            uint8_t* o = dst + plane * ((long long)H * W) + (long long)y * W + x;
            if (VEC) {                                                   // W % 4 == 0: x < W implies x + 3 < W
                *reinterpret_cast<uint32_t*>(o) = (uint32_t)(acc[0] >> 14) | (uint32_t)(acc[1] >> 14) << 8 |
                                                  (uint32_t)(acc[2] >> 14) << 16 | (uint32_t)(acc[3] >> 14) << 24;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x + k < W) o[k] = (uint8_t)(acc[k] >> 14);
            }
        }
    }
}

// ---- noise ---------------------------------------------------------------------------------------------------------------
// the sum of the 16 bytes of philox4x32_10((c0, c1, c2, c3), (k0, k1))
__device__ __forceinline__ int dg_philox_bytes(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    uint32_t s = 0;
    const uint32_t w[4] = {c0, c1, c2, c3};
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (w[k] & 0xffu) + ((w[k] >> 8) & 0xffu) + ((w[k] >> 16) & 0xffu) + (w[k] >> 24);
    return (int)s;
}

// grid: (x: lanes over ceil(H * W / 4) groups of 4 flat indices, y: sample).  src and out_u8 may be the same buffer.
template <bool VEC, bool F32>
__global__ void __launch_bounds__(256) degrade_noise_kernel(const uint8_t* src, const int* __restrict__ table,
                                                            uint32_t seed_lo, uint32_t seed_hi, uint32_t scale,
                                                            long long HW, uint8_t* out_u8, float* __restrict__ out_f32) {
    const long long n = blockIdx.y;
    const int* row = table + n * DG_COLS;
    const int a = dg_clampi(row[2], 0, 1 << 19);
    const bool gray = row[3] != 0;
    const uint32_t stream = (uint32_t)row[4];
    const long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (e0 >= HW) return;                               // whole lanes past the plane leave before any address is formed
    uint32_t v[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t* p = src + (n * 3 + c) * HW;
        if (VEC) {
            const uint32_t d = *reinterpret_cast<const uint32_t*>(p + e0);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = (d >> (8 * k)) & 0xffu;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[c][k] = p[e0 + k < HW ? e0 + k : HW - 1];
        }
    }
    if (a != 0) {                                       // uniform over the workgroup
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t idx = (uint32_t)(e0 + k);
            int nz[3];
            nz[0] = (a * (dg_philox_bytes(idx, 0u, stream, scale, seed_lo, seed_hi) - 2040) + (1 << 15)) >> 16;
            if (gray) {
                nz[1] = nz[2] = nz[0];
            } else {
                nz[1] = (a * (dg_philox_bytes(idx, 1u, stream, scale, seed_lo, seed_hi) - 2040) + (1 << 15)) >> 16;
                nz[2] = (a * (dg_philox_bytes(idx, 2u, stream, scale, seed_lo, seed_hi) - 2040) + (1 << 15)) >> 16;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c][k] = (uint32_t)dg_clampi((int)v[c][k] + nz[c], 0, 255);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long o = (n * 3 + c) * HW + e0;
        if (VEC) {
            *reinterpret_cast<uint32_t*>(out_u8 + o) = v[c][0] | v[c][1] << 8 | v[c][2] << 16 | v[c][3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < HW) out_u8[o + k] = (uint8_t)v[c][k];
        }
        if (F32) {
            float f[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = __fdiv_rn((float)v[c][k], 255.0f);
            if (VEC) {
                *reinterpret_cast<float4*>(out_f32 + o) = make_float4(f[0], f[1], f[2], f[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (e0 + k < HW) out_f32[o + k] = f[k];
            }
        }
    }
}

}  // namespace ofasr

using namespace ofasr;

// the checks the two entry points share
#define DG_REQUIRE_SIZES(n, H, W)                                                                                        \
    OFASR_REQUIRE((n) >= 0 && (H) > 0 && (W) > 0, OFASR_ERR_INVALID_ARG, "%s: negative n or non-positive plane", name);   \
    OFASR_REQUIRE((H) < (1LL << 32) && (W) < (1LL << 32) && (H) * (W) < (1LL << 32), OFASR_ERR_UNSUPPORTED,              \
                  "%s: a plane of %lld x %lld has 2^32 pixels or more", name, (long long)(H), (long long)(W));           \
    OFASR_REQUIRE((n) <= 21845, OFASR_ERR_UNSUPPORTED, "%s: %lld samples in one launch (at most 21845)", name,           \
                  (long long)(n))

OFASR_EXPORT int ofasr_degrade_blur_u8(const void* src, const int32_t* table, int64_t n, int64_t H, int64_t W,
                                       int64_t max_radius, void* dst, void* stream) {
    const char* name = "ofasr_degrade_blur_u8";
    OFASR_REQUIRE(src && table && dst, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    DG_REQUIRE_SIZES(n, H, W);
    OFASR_REQUIRE(max_radius >= 0 && max_radius <= DG_HALO, OFASR_ERR_UNSUPPORTED, "%s: radius %lld (0 .. %d)", name,
                  (long long)max_radius, DG_HALO);
    OFASR_REQUIRE(H < (1LL << 31) && W < (1LL << 31) && cdiv(H, DG_TH) <= 65535, OFASR_ERR_UNSUPPORTED,
                  "%s: a plane of %lld rows (at most %d)", name, (long long)H, 65535 * DG_TH);
    OFASR_REQUIRE(src != dst, OFASR_ERR_INVALID_ARG, "%s: the blur does not run in place", name);
    OFASR_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3) == 0, OFASR_ERR_INVALID_ARG, "%s: the table is not 4-byte aligned",
                  name);
    if (n == 0) return OFASR_OK;
    const dim3 grid((unsigned)cdiv(W, DG_TW), (unsigned)cdiv(H, DG_TH), (unsigned)(3 * n));
    const bool vec = W % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0;
    prof_note((double)n * 3.0 * (double)(H * W) * 2.0, 0.0);
    dispatch_bool(vec, [&](auto VEC) {
        OFASR_LAUNCH((degrade_blur_kernel<VEC>), grid, dim3(DG_THREADS), 0, as_stream(stream), (const uint8_t*)src,
                     (const int*)table, (int)H, (int)W, (int)max_radius, (uint8_t*)dst);
    });
    return check_launch(name);
}

OFASR_EXPORT int ofasr_degrade_noise_u8(const void* src, const int32_t* table, uint32_t seed_lo, uint32_t seed_hi,
                                        int64_t scale, int64_t n, int64_t H, int64_t W, void* out_u8, void* out_f32,
                                        void* stream) {
    const char* name = "ofasr_degrade_noise_u8";
    OFASR_REQUIRE(src && table && out_u8, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    DG_REQUIRE_SIZES(n, H, W);
    OFASR_REQUIRE(scale == 2 || scale == 4, OFASR_ERR_UNSUPPORTED, "%s: scale %lld (2 or 4)", name, (long long)scale);
    OFASR_REQUIRE((reinterpret_cast<uintptr_t>(table) & 3) == 0 && (reinterpret_cast<uintptr_t>(out_f32) & 3) == 0,
                  OFASR_ERR_INVALID_ARG, "%s: the table or the fp32 output is not 4-byte aligned", name);
    if (n == 0) return OFASR_OK;
    const int64_t HW = H * W;
    const dim3 grid((unsigned)cdiv(cdiv(HW, 4), 256), (unsigned)n);
    const bool vec = HW % 4 == 0 && reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(out_u8) % 4 == 0 &&
                     aligned16(out_f32);
    prof_note((double)n * 3.0 * (double)HW * (out_f32 ? 6.0 : 2.0), 0.0);
    dispatch_bool(vec, [&](auto VEC) {
        dispatch_bool(out_f32 != nullptr, [&](auto F32) {
            OFASR_LAUNCH((degrade_noise_kernel<VEC, F32>), grid, dim3(256), 0, as_stream(stream), (const uint8_t*)src,
                         (const int*)table, seed_lo, seed_hi, (uint32_t)scale, (long long)HW, (uint8_t*)out_u8,
                         (float*)out_f32);
        });
    });
    return check_launch(name);
}
