// augment.hip -- the training augmentation on GPU-resident images (ofasr_aug_gather_u8) and on GPU-resident planar
// YUV 4:2:0 video frames with the colour decode fused in (ofasr_aug_gather_yuv420, stated before its kernel below; the
// HR / LR pair of one draw in one launch: ofasr_aug_gather_yuv420_pair, stated before its kernel), and the choice of the
// most detailed of K candidate crops per sample in front of any of the three (ofasr_aug_select, stated before its kernels).
//
// The DIV2K training sample is RandomCrop(S) -> RandomHorizontalFlip -> RandomRotation((-90, 90)) of a decoded RGB image
// (data_providers/div2k_setxx.py).  With the decoded images resident in one uint8 pool, the three transforms are one
// integer gather per output pixel, bit-equal to the PIL calls of the host provider (host statement and the derivation of
// the coefficients: data_providers/augment.py; Pillow's Image.rotate(angle, NEAREST) walks its 2x3 matrix in 16.16 fixed
// point for images below 32768 pixels per side -- affine_fixed in Geometry.c):
//   xin = (a2 + y * a1 + x * a0) >> 16,  yin = (a5 + y * a4 + x * a3) >> 16        (arithmetic shift)
//   out[n, c, y, x] = 0 <= xin, yin < S ? pool[offset + ((i + yin) * W + j + (flip ? S - 1 - xin : xin)) * 3 + c] : 0
// per sample n from the device table row (offset, H, W, i, j, flip, a0 .. a5): the flip applies to the rotation's source
// because the pipeline flips before it rotates.  One launch per batch; the optional second output is the same batch as
// fp32, (float)v / 255.0f with fp32 division (ToTensor, bit for bit).
//
// int32 is enough.  |a0| + |a1| <= 65536 * sqrt 2 (a cosine and a sine of one angle, rounded), x, y <= S - 1 <= 4095, so
// |y * a1 + x * a0| <= 4095 * 92682 < 3.80e8; a2 = FIX(S/2 * (1 - m0 - m1) + (m0 + m1) / 2) has |a2| <= 65536 * (2048 *
// (1 + sqrt 2) + 0.71) < 3.25e8.  The sum stays below 7.1e8 < 2^31; the same holds for the second row.  The kernel adds
// in uint32 all the same, so a table of garbage wraps instead of being undefined, and what it yields is clamped.
//
// Nothing leaves the pool whatever the table holds (aug_row below states it once for both kernels): H and W are clamped
// to [S, 2^24], (i, j) to [0, H - S] x [0, W - S], offset to [0, pool_bytes], and the byte address of every pixel to
// [0, pool_bytes - 3].  Addresses are 64-bit.
//
// Access.  A lane owns 4 adjacent output columns of one row.  Its 12 source bytes are 12 byte loads: after a rotation
// neighbouring output pixels are not neighbours in the source, and a pixel's 3 bytes have no alignment.  Every load is
// issued unconditionally from a clamped address and the zero fill is selected afterwards, so no load waits under a
// lane-dependent branch: the 12 loads are in flight together (the only guard is the exit of lanes past the end of the
// plane, before any address is formed).  Stores: one dword per plane for the uint8 batch and one 16-byte vector per
// plane for the fp32 batch when S % 4 == 0 and the outputs are aligned for them; element stores otherwise (S = 30: rows
// are not dword-aligned).
#include "yuv_block.h"

namespace ofasr {

// row n of the table, clamped as stated above; `yuv`: the frame's sides are even, Se = S rounded up to even in H's and W's
// lower bound (the header of ofasr_aug_gather_yuv420 below)
struct AugRow {
    long long off, H, W, ci, cj;
    bool flip;
    uint32_t a0, a1, a2, a3, a4, a5;
};
__device__ __forceinline__ AugRow aug_row(const long long* __restrict__ table, long long n, int S, long long pool_bytes, bool yuv) {
    const long long* t = table + 12 * n;
    AugRow r;
    r.flip = t[5] != 0;
    r.a0 = (uint32_t)t[6], r.a1 = (uint32_t)t[7], r.a2 = (uint32_t)t[8];
    r.a3 = (uint32_t)t[9], r.a4 = (uint32_t)t[10], r.a5 = (uint32_t)t[11];
    const long long lim = 1LL << 24, Se = yuv ? (S + 1) & ~1 : S;
    r.H = clampll(t[1], Se, lim);
    r.W = clampll(t[2], Se, lim);
    if (yuv) r.H &= ~1LL, r.W &= ~1LL;
    r.ci = clampll(t[3], 0, r.H - S);
    r.cj = clampll(t[4], 0, r.W - S);
    r.off = clampll(t[0], 0, pool_bytes);
    return r;
}

// the lane's group of 4 output columns (y, x0 .. x0 + 3) and the fixed-point walk at its first column; false for whole
// lanes past the end of the plane, which leave before any address is formed.  `e` is the lane's group index inside the
// sample: blockIdx.x * blockDim.x + threadIdx.x in the one-batch kernels, counted from its segment's first block in the
// pair kernel
struct AugWalk { int y, x0; uint32_t fx, fy; };
__device__ __forceinline__ bool aug_walk_start(const AugRow& r, int S, int e, AugWalk& w) {
    const int gw = (S + 3) >> 2;
    const int total = S * gw;
    if (e >= total) return false;
    w.y = e / gw;
    w.x0 = (e - w.y * gw) * 4;
    w.fx = r.a2 + (uint32_t)w.y * r.a1 + (uint32_t)w.x0 * r.a0;
    w.fy = r.a5 + (uint32_t)w.y * r.a4 + (uint32_t)w.x0 * r.a3;
    return true;
}
// one column of the walk: the source row yc and column col inside the crop (clamped into it, the flip applied) and
// whether the pixel is inside at all; then one step to the right
__device__ __forceinline__ bool aug_walk_step(const AugRow& r, int S, AugWalk& w, int& yc, int& col) {
    const int xin = (int)w.fx >> 16, yin = (int)w.fy >> 16;
    const bool ok = xin >= 0 && xin < S && yin >= 0 && yin < S;
    const int xc = xin < 0 ? 0 : (xin > S - 1 ? S - 1 : xin);
    yc = yin < 0 ? 0 : (yin > S - 1 ? S - 1 : yin);
    col = r.flip ? S - 1 - xc : xc;
    w.fx += r.a0;
    w.fy += r.a3;
    return ok;
}

// the store tail: v[k][c] of the group's 4 columns into the uint8 batch and, with F32, v / 255 into the fp32 batch; VEC:
// one dword / one float4 per plane, element stores otherwise
template <bool VEC, bool F32>
__device__ __forceinline__ void aug_store4(const uint32_t (&v)[4][3], long long n, int S, int y, int x0,
                                           uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
    const long long plane = (long long)S * S;
    const long long o = n * 3 * plane + (long long)y * S + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint8_t* d8 = out_u8 + o + c * plane;
        if (VEC) {
            *reinterpret_cast<uint32_t*>(d8) = v[0][c] | v[1][c] << 8 | v[2][c] << 16 | v[3][c] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x0 + k < S) d8[k] = (uint8_t)v[k][c];
        }
        if (F32) {
            float f[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) f[k] = __fdiv_rn((float)v[k][c], 255.0f);
            float* df = out_f32 + o + c * plane;
            if (VEC) {
                *reinterpret_cast<float4*>(df) = make_float4(f[0], f[1], f[2], f[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x0 + k < S) df[k] = f[k];
            }
        }
    }
}

// grid: (x: lanes over S * ceil(S / 4) groups, y: sample)
template <bool VEC, bool F32>
__global__ void __launch_bounds__(256) aug_gather_u8_kernel(const uint8_t* __restrict__ pool, long long pool_bytes,
                                                            const long long* __restrict__ table, int S,
                                                            uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
    const long long n = blockIdx.y;
    const AugRow R = aug_row(table, n, S, pool_bytes, false);
    const long long last = pool_bytes - 3;
    AugWalk wk;
    if (!aug_walk_start(R, S, (int)(blockIdx.x * blockDim.x + threadIdx.x), wk)) return;   // nothing below branches around a load
    uint32_t v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int yc, col;
        const bool ok = aug_walk_step(R, S, wk, yc, col);
        long long b = R.off + ((R.ci + yc) * R.W + R.cj + col) * 3;
        b = b > last ? last : b;
        const uint8_t* p = pool + b;
        const uint32_t r0 = p[0], r1 = p[1], r2 = p[2];
        v[k][0] = ok ? r0 : 0u;
        v[k][1] = ok ? r1 : 0u;
        v[k][2] = ok ? r2 : 0u;
    }
    aug_store4<VEC, F32>(v, n, S, wk.y, wk.x0, out_u8, out_f32);
}

// ---- the same gather from a pool of planar YUV 4:2:0 frames (ofasr_aug_gather_yuv420) --------------------------------
// A frame sits in the pool as it sits in a yuv420p / Y4M file: Y [H, W], U [H/2, W/2], V [H/2, W/2], contiguous, 8 bits
// a sample; `offset` is the byte offset of its Y plane.  With xin, yin, ok from the walk above,
//   py = i + yin,  px = j + (flip ? S - 1 - xin : xin),  out[n, c, y, x] = ok ? RGB(frame)[py, px, c] : 0
// where RGB(frame) is the decode of the WHOLE frame (video.yuv420_to_rgb_host, stated in yuv.hip's header): the chroma
// taps are cy0 = py >> 1 and its neighbour row cy0 - 1 (even py) / cy0 + 1 (odd py), columns alike from px, clamped into
// the PLANE -- chroma replicates at the frame's edge, never at the crop's, and the parity is the frame coordinate's, so a
// crop at an odd corner decodes as the frame does there.  The batch equals aug_gather_u8 of the decoded frames byte for
// byte, and no RGB frame exists.
//
// Nothing leaves the pool whatever the table holds.  With Se = S rounded up to even:  H = clamp(H, Se, 2^24) & ~1 and W
// alike (even, still inside [Se, 2^24]);  (i, j) to [0, H - S] x [0, W - S];  offset to [0, pool_bytes];  then the byte
// address of every one of the 9 samples of a pixel --
//   Y: offset + py * W + px,   U: offset + H * W + cr * (W/2) + cc,   V: offset + H * W + (H/2) * (W/2) + cr * (W/2) + cc
// -- to [0, pool_bytes - 1].  H * W <= 2^48 and offset <= pool_bytes: the sums stay far inside int64.
//
// Access.  As above: a lane owns 4 adjacent output columns of one row; its 36 source bytes (per pixel 1 Y, 4 U, 4 V) are
// 36 byte loads, all issued unconditionally from clamped addresses, and the zero fill is selected after the decode.  The
// only early exit is that of lanes past the end of the plane.  Stores as above.  There is no unrotated fast path: one
// code for every angle.
__device__ __forceinline__ int aug_tap(int p, int last) {      // the neighbour chroma index of frame coordinate p
    const int c0 = p >> 1;
    const int nb = (p & 1) ? c0 + 1 : c0 - 1;
    return nb < 0 ? 0 : (nb > last ? last : nb);
}

// the body of the 4:2:0 gathers: sample n's group e (aug_walk_start) of the S x S crop that row n of `table` cuts from
// `pool`, into out_u8 / out_f32.  Shared by aug_gather_yuv420_kernel and the two segments of the pair kernel below.
template <bool VEC, bool F32>
__device__ __forceinline__ void aug_yuv420_body(const uint8_t* __restrict__ pool, long long pool_bytes,
                                                const long long* __restrict__ table, long long n, int S, int e,
                                                const YuvDec& D, uint8_t* __restrict__ out_u8,
                                                float* __restrict__ out_f32) {
    const AugRow R = aug_row(table, n, S, pool_bytes, true);
    const long long last = pool_bytes - 1;
    const long long CW = R.W >> 1;
    const int chl = (int)(R.H >> 1) - 1, cwl = (int)CW - 1;    // H, W <= 2^24: frame coordinates fit int32
    const long long ub = R.off + R.H * R.W, vb = ub + (R.H >> 1) * CW;
    AugWalk wk;
    if (!aug_walk_start(R, S, e, wk)) return;   // nothing below branches around a load
    int Y[4], U[4][4], V[4][4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int yc, col;
        ok[k] = aug_walk_step(R, S, wk, yc, col);
        const int py = (int)R.ci + yc, px = (int)R.cj + col;
        const long long r0 = (long long)(py >> 1) * CW, r1 = (long long)aug_tap(py, chl) * CW;
        const long long c0 = px >> 1, c1 = aug_tap(px, cwl);
        const long long by = R.off + (long long)py * R.W + px;
        const long long q[4] = {r0 + c0, r0 + c1, r1 + c0, r1 + c1};   // the taps in yuv_decode_px's 9-3-3-1 order
        Y[k] = pool[by > last ? last : by];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const long long bu = ub + q[m], bv = vb + q[m];
            U[k][m] = pool[bu > last ? last : bu];
            V[k][m] = pool[bv > last ? last : bv];
        }
    }
    __builtin_amdgcn_sched_barrier(0);   // the 36 loads stay in front of the decode: none is moved behind a wait
    uint32_t v[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int rgb[3];
        yuv_decode_px<uint8_t>(D, Y[k], U[k], V[k], rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[k][c] = ok[k] ? (uint32_t)rgb[c] : 0u;   // the zero fill, selected after the decode
    }
    aug_store4<VEC, F32>(v, n, S, wk.y, wk.x0, out_u8, out_f32);
}

// grid: (x: lanes over S * ceil(S / 4) groups, y: sample)
template <bool VEC, bool F32>
__global__ void __launch_bounds__(256) aug_gather_yuv420_kernel(const uint8_t* __restrict__ pool, long long pool_bytes,
                                                                const long long* __restrict__ table, int S, YuvDec D,
                                                                uint8_t* __restrict__ out_u8, float* __restrict__ out_f32) {
    aug_yuv420_body<VEC, F32>(pool, pool_bytes, table, blockIdx.y, S, (int)(blockIdx.x * blockDim.x + threadIdx.x), D,
                              out_u8, out_f32);
}

// ---- a paired sample: the HR crop and the LR crop of one draw in ONE launch (ofasr_aug_gather_yuv420_pair) -----------
// Two pools of 4:2:0 frames, HR and LR (the decoded low-resolution stream of the same video, sides 1/f of HR's), and a
// table of two blocks [2][n][12]: block 0 the HR rows (crop side S), block 1 the LR rows (crop side S / f), each row in
// the layout above with its offset relative to its own pool and a0 .. a5 for its own canvas.  Each side is exactly
// aug_gather_yuv420 of its pool and its table block: the decode of its own whole frame, chroma parity and edge
// replication its own frame's, the same clamps against its own pool's size.  The host draws one (i, j, flip, angle) on
// the LR grid and hands HR (f*i, f*j, flip, angle) (augment.draw_pair_params, make_pair_table).
//
// grid: (x: hr_blocks = ceil(S * ceil(S / 4) / 256) blocks of HR lanes, then the blocks of LR lanes; y: sample).  Which
// side a block serves depends on blockIdx.x alone, so the branch is uniform over the block and no wave diverges; each
// side then runs the body above with its own operands.  VEC is chosen per side (S = 24, f = 4: vector stores for HR,
// element stores for the 6-wide LR rows).
struct AugSide {
    const uint8_t* pool;
    long long pool_bytes;
    const long long* table;
    int S;
    uint8_t* out_u8;
    float* out_f32;
};

template <bool VEC_HR, bool VEC_LR, bool F32>
__global__ void __launch_bounds__(256) aug_gather_yuv420_pair_kernel(AugSide hr, AugSide lr, unsigned hr_blocks, YuvDec D) {
    if (blockIdx.x < hr_blocks)
        aug_yuv420_body<VEC_HR, F32>(hr.pool, hr.pool_bytes, hr.table, blockIdx.y, hr.S,
                                     (int)(blockIdx.x * blockDim.x + threadIdx.x), D, hr.out_u8, hr.out_f32);
    else
        aug_yuv420_body<VEC_LR, F32>(lr.pool, lr.pool_bytes, lr.table, blockIdx.y, lr.S,
                                     (int)((blockIdx.x - hr_blocks) * blockDim.x + threadIdx.x), D, lr.out_u8, lr.out_f32);
}

template <bool VEC_HR, bool VEC_LR, bool F32>
static void aug_pair_launch(const AugSide& hr, const AugSide& lr, int64_t n, const YuvDec& D, hipStream_t st) {
    const int64_t hb = cdiv((int64_t)hr.S * cdiv(hr.S, 4), 256), lb = cdiv((int64_t)lr.S * cdiv(lr.S, 4), 256);
    const dim3 grid((unsigned)(hb + lb), (unsigned)n);
    prof_note((double)n * ((double)hr.S * hr.S + (double)lr.S * lr.S) * 3.0 * (F32 ? 6.0 : 2.0), 0.0);
    OFASR_LAUNCH((aug_gather_yuv420_pair_kernel<VEC_HR, VEC_LR, F32>), grid, dim3(256), 0, st, hr, lr, (unsigned)hb, D);
}
template <bool VEC_HR, bool VEC_LR>
static void aug_pair_f32(const AugSide& hr, const AugSide& lr, int64_t n, const YuvDec& D, hipStream_t st) {
    dispatch_bool(hr.out_f32 != nullptr, [&](auto F32) { aug_pair_launch<VEC_HR, VEC_LR, F32>(hr, lr, n, D, st); });
}
static bool aug_vec_ok(const AugSide& s) {
    return s.S % 4 == 0 && reinterpret_cast<uintptr_t>(s.out_u8) % 4 == 0 && aligned16(s.out_f32);
}
static void aug_gather_pair(const AugSide& hr, const AugSide& lr, int64_t n, const YuvDec& D, hipStream_t st) {
    dispatch_bool(aug_vec_ok(hr), [&](auto VEC_HR) {
        dispatch_bool(aug_vec_ok(lr), [&](auto VEC_LR) { aug_pair_f32<VEC_HR, VEC_LR>(hr, lr, n, D, st); });
    });
}

// the launch of either kernel (YUV: the 4:2:0 one, which takes D) and the one VEC / F32 ladder
template <bool YUV, bool VEC, bool F32>
static void aug_launch(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t n, int64_t S, const YuvDec& D,
                       void* out_u8, void* out_f32, hipStream_t st) {
    const dim3 grid((unsigned)cdiv(S * cdiv(S, 4), 256), (unsigned)n);
    prof_note((double)n * (double)(S * S) * 3.0 * (F32 ? 6.0 : 2.0), 0.0);
    if constexpr (YUV)
        OFASR_LAUNCH((aug_gather_yuv420_kernel<VEC, F32>), grid, dim3(256), 0, st, (const uint8_t*)pool, (long long)pool_bytes,
                     (const long long*)table, (int)S, D, (uint8_t*)out_u8, (float*)out_f32);
    else
        OFASR_LAUNCH((aug_gather_u8_kernel<VEC, F32>), grid, dim3(256), 0, st, (const uint8_t*)pool, (long long)pool_bytes,
                     (const long long*)table, (int)S, (uint8_t*)out_u8, (float*)out_f32);
}
template <bool YUV>
static void aug_gather(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t n, int64_t S, const YuvDec& D,
                       void* out_u8, void* out_f32, hipStream_t st) {
    const bool vec = S % 4 == 0 && reinterpret_cast<uintptr_t>(out_u8) % 4 == 0 && aligned16(out_f32);
    dispatch_bool(vec, [&](auto VEC) {
        dispatch_bool(out_f32 != nullptr, [&](auto F32) {
            aug_launch<YUV, VEC, F32>(pool, pool_bytes, table, n, S, D, out_u8, out_f32, st);
        });
    });
}

// ---- best of K candidate crops (ofasr_aug_select) ------------------------------------------------------------------------
// K candidate rows per sample stand in the table [blocks][n * K][12], sample-major; the candidate whose S x S crop
// rectangle holds the largest luma activity wins, ties to the lowest index, and its row (both blocks' rows of a paired
// set) goes into the [blocks][n][12] table the gathers above take unchanged.  The host statement is augment.py
// (crop_activity_np / select_candidates_np; on the pool's bytes with the clamps: aug_select_np), the measure routing.py's:
//   L   the luma sample: the Y plane's byte of a 4:2:0 frame, or (77 R + 150 G + 29 B + 128) >> 8 of an RGB pixel
//   A   over rows i .. i + S - 1, columns j .. j + S - 1 of the frame (before flip and rotation):
//       sum of |L[r][c + 1] - L[r][c]| (r < S, c < S - 1) + sum of |L[r + 1][c] - L[r][c]| (r < S - 1, c < S)
// always from block 0's row (clamped by aug_row as the gathers clamp it) on `pool`.  A <= 510 S^2: int64.
// activity: grid (x: row strip, y: candidate), strips = aug_select_strips(S) (include/ofasr.h).  A strip owns the horizontal
//          terms of its rows and the vertical terms whose upper row it owns.  The 256 threads are LPR lanes along a row
//          (LPR = the power of two >= ceil(S / 4), at most 256) times 256 / LPR row lanes; a row lane walks a contiguous
//          run of the strip's rows downwards and keeps the previous row's lumas in registers.  A thread owns 4 adjacent
//          columns and reads a fifth, its right neighbour.  Wide path: the dwords that cover its 5 samples, read from
//          4-byte aligned addresses (2 for a Y plane, 5 for RGB) and shifted by the row's misalignment, whatever the
//          corner; it is taken when the pool's base is 4-byte aligned and the rectangle ends at least AUG_SELECT_SLACK
//          bytes before the pool does, both uniform over the workgroup.  Byte path otherwise: 5 / 15 byte loads, each
//          address clamped to [0, pool_bytes - 1].  Either way every load is issued from a clamped address by every
//          lane, every trip, and rows, columns and lanes that do not count are masked afterwards: no load stands under a
//          lane-dependent branch.  The workgroup reduces through the waves (shuffles), then 4 words of LDS, and thread 0
//          stores ONE int64, partial[q * strips + s], with a plain store.
// choose:  ONE wave per sample.  Lane c < K folds candidate c's partials in strip order; every lane then scans the K sums
//          in index order and keeps the first largest; lanes copy the winner's 12 words per block, `choice` and the K
//          activities.  With `stats`: three 64-bit integer atomic adds (sum of the chosen, sum of the first candidates,
//          1 per sample) -- integer, so two calls still give identical bytes everywhere.
static const int AUG_SELECT_THREADS = 256;
static const long long AUG_SELECT_STRIP_SAMPLES = 16384;
static const int AUG_SELECT_MAX_STRIPS = 64;
static const int AUG_SELECT_MAX_K = 16;
static const long long AUG_SELECT_SLACK = 20;           // bytes a wide read may pass the rectangle's last byte by, at most

// the strip count, as include/ofasr.h states it (augment.aug_select_strips mirrors it)
inline int64_t aug_select_strips(int64_t S) {
    int64_t s = cdiv(S * S, AUG_SELECT_STRIP_SAMPLES);
    s = s < AUG_SELECT_MAX_STRIPS ? s : AUG_SELECT_MAX_STRIPS;
    s = s < S ? s : S;
    return s < 1 ? 1 : s;
}

__device__ __forceinline__ int aug_luma(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }

// BPS: bytes per sample, 1 (the Y plane of a 4:2:0 frame) or 3 (interleaved RGB)
template <int BPS>
__global__ void __launch_bounds__(AUG_SELECT_THREADS) aug_select_activity_kernel(const uint8_t* __restrict__ pool,
                                                                                 long long pool_bytes,
                                                                                 const long long* __restrict__ table, int S,
                                                                                 long long* __restrict__ partial) {
    __shared__ long long red[AUG_SELECT_THREADS / 64];
    constexpr int NW = BPS == 1 ? 2 : 5;                 // aligned dwords that cover 5 samples at any misalignment
    const long long q = blockIdx.y;
    const AugRow R = aug_row(table, q, S, pool_bytes, BPS == 1);
    long long lo, hi;
    slab_rows(S, blockIdx.x, gridDim.x, lo, hi);
    const int G = (S + 3) >> 2;
    int lpr = 1;
    while (lpr < G && lpr < AUG_SELECT_THREADS) lpr <<= 1;
    const int RL = AUG_SELECT_THREADS / lpr;
    const int cl = (int)threadIdx.x & (lpr - 1), rl = (int)threadIdx.x / lpr;
    // the run of rows of this row lane: [r0, r1) owned; row r1 is read as well, for the vertical terms below r1 - 1
    const long long per = (hi - lo + RL - 1) / RL;
    const long long r0 = lo + rl * per < hi ? lo + rl * per : hi;
    const long long r1 = r0 + per < hi ? r0 + per : hi;
    const long long base = R.off + (R.ci * R.W + R.cj) * BPS;            // the rectangle's first byte
    const long long rect_last = base + ((long long)(S - 1) * R.W + (S - 1)) * BPS + (BPS - 1);
    const long long last = pool_bytes - 1;
    const bool wide = (reinterpret_cast<uintptr_t>(pool) & 3) == 0 && rect_last + AUG_SELECT_SLACK < pool_bytes;
    long long acc = 0;
    for (int g0 = 0; g0 < G; g0 += lpr) {                                // the trip counts are the workgroup's
        const int g = g0 + cl;
        const int c0 = (g < G ? g : G - 1) * 4;                          // lanes past the row repeat its last group, masked
        bool cv[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) cv[k] = g < G && c0 + k < S;
        int P[4] = {0, 0, 0, 0};
        for (long long t = 0; t <= per; ++t) {
            const long long r = r0 + t;
            const long long rc = r < S - 1 ? r : S - 1;
            const bool own = r < r1;                                     // its horizontal terms count
            const bool below = t > 0 && r <= r1 && r < S;                // its vertical terms to the row above count
            int L[5];
            const long long rb = base + rc * R.W * BPS;                  // the row's first byte in the rectangle
            if (wide) {
                const long long a = rb + (long long)c0 * BPS;
                const int sh = 8 * (int)((reinterpret_cast<uintptr_t>(pool) + (uintptr_t)a) & 3);
                const uint32_t* p = reinterpret_cast<const uint32_t*>(pool + (a - (sh >> 3)));
                uint32_t d[NW + 1];
#pragma unroll
                for (int k = 0; k < NW; ++k) d[k] = p[k];
                d[NW] = 0u;
                uint32_t w[NW];                                          // the bytes from `a` on
#pragma unroll
                for (int k = 0; k < NW; ++k) w[k] = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> sh);
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    if constexpr (BPS == 1) {
                        L[k] = (int)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
                    } else {
                        int c[3];
#pragma unroll
                        for (int m = 0; m < 3; ++m) {
                            const int b = 3 * k + m;
                            c[m] = (int)((w[b >> 2] >> (8 * (b & 3))) & 0xffu);
                        }
                        L[k] = aug_luma(c[0], c[1], c[2]);
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const int col = c0 + k < S ? c0 + k : S - 1;
                    const long long a = rb + (long long)col * BPS;
                    if constexpr (BPS == 1) {
                        L[k] = pool[a > last ? last : a];
                    } else {
                        const long long a1 = a + 1, a2 = a + 2;
                        L[k] = aug_luma(pool[a > last ? last : a], pool[a1 > last ? last : a1], pool[a2 > last ? last : a2]);
                    }
                }
            }
            int sum = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sum += own && cv[k + 1] ? abs(L[k + 1] - L[k]) : 0;
                sum += below && cv[k] ? abs(L[k] - P[k]) : 0;
                P[k] = L[k];
            }
            acc += sum;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane_id() == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0;
#pragma unroll
        for (int w = 0; w < AUG_SELECT_THREADS / 64; ++w) s += red[w];
        partial[q * gridDim.x + blockIdx.x] = s;
    }
}

// grid: (x: sample), one wave
__global__ void __launch_bounds__(64) aug_select_choose_kernel(const long long* __restrict__ partial, int strips,
                                                               const long long* __restrict__ cand, int blocks, long long n,
                                                               int K, long long* __restrict__ out_table,
                                                               int* __restrict__ choice, long long* __restrict__ activity,
                                                               unsigned long long* __restrict__ stats) {
    __shared__ long long act[AUG_SELECT_MAX_K];
    const long long s = blockIdx.x;
    const int t = (int)threadIdx.x;
    const int c = t < K ? t : K - 1;                     // lanes past K fold the last candidate again, and store nothing
    long long A = 0;
    for (int k = 0; k < strips; ++k) A += partial[(s * K + c) * strips + k];
    if (t < K) {
        act[t] = A;
        activity[s * K + t] = A;
    }
    __syncthreads();
    int best = 0;
    long long bestA = act[0];
    for (int k = 1; k < K; ++k) {
        const long long v = act[k];
        if (v > bestA) bestA = v, best = k;               // strictly larger: a tie stays with the lower index
    }
    if (t < 12 * blocks) {
        const int b = t / 12, w = t - 12 * b;
        out_table[((long long)b * n + s) * 12 + w] = cand[(((long long)b * n + s) * K + best) * 12 + w];
    }
    if (t == 0) {
        choice[s] = best;
        if (stats) {
            atomicAdd(stats, (unsigned long long)bestA);
            atomicAdd(stats + 1, (unsigned long long)act[0]);
            atomicAdd(stats + 2, 1ull);
        }
    }
}

}  // namespace ofasr

using namespace ofasr;

// the checks the two entry points share
#define AUG_REQUIRE_SIZES(n, S, pool_bytes)                                                                              \
    OFASR_REQUIRE((n) > 0 && (S) > 0 && (pool_bytes) > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);         \
    OFASR_REQUIRE((S) <= 4096, OFASR_ERR_UNSUPPORTED, "%s: crop side %lld above 4096 (the fixed-point walk is int32)", name, \
                  (long long)(S));                                                                                       \
    OFASR_REQUIRE((n) <= 65535, OFASR_ERR_UNSUPPORTED, "%s: %lld samples in one launch (at most 65535)", name, (long long)(n))

OFASR_EXPORT int ofasr_aug_gather_yuv420(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t n, int64_t S,
                                         const int32_t* coeffs, void* out_u8, void* out_f32, void* stream) {
    const char* name = "ofasr_aug_gather_yuv420";
    OFASR_REQUIRE(pool && table && coeffs && out_u8, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    AUG_REQUIRE_SIZES(n, S, pool_bytes);
    OFASR_REQUIRE(yuv_coeffs_ok(coeffs, 6), OFASR_ERR_INVALID_ARG, "%s: coefficient outside the 14-bit tables' range", name);
    // the table lives on the device: the smallest pool that can hold one even-sided frame with H, W >= S is what the
    // host can check
    const int64_t Se = (S + 1) & ~(int64_t)1;
    OFASR_REQUIRE(pool_bytes >= Se * Se * 3 / 2, OFASR_ERR_UNSUPPORTED,
                  "%s: a pool of %lld bytes holds no 4:2:0 frame of at least %lldx%lld (even H, W >= S)", name,
                  (long long)pool_bytes, (long long)Se, (long long)Se);
    aug_gather<true>(pool, pool_bytes, table, n, S, yuv_dec(coeffs), out_u8, out_f32, as_stream(stream));
    return check_launch(name);
}

OFASR_EXPORT int ofasr_aug_gather_yuv420_pair(const void* hr_pool, int64_t hr_bytes, const void* lr_pool, int64_t lr_bytes,
                                              const int64_t* table, int64_t n, int64_t S, int64_t f, const int32_t* coeffs,
                                              void* hr_u8, void* hr_f32, void* lr_u8, void* lr_f32, void* stream) {
    const char* name = "ofasr_aug_gather_yuv420_pair";
    OFASR_REQUIRE(hr_pool && lr_pool && table && coeffs && hr_u8 && lr_u8, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE((hr_f32 == nullptr) == (lr_f32 == nullptr), OFASR_ERR_INVALID_ARG,
                  "%s: both fp32 outputs or neither", name);
    OFASR_REQUIRE(f == 2 || f == 4, OFASR_ERR_UNSUPPORTED, "%s: scale %lld (2 or 4)", name, (long long)f);
    AUG_REQUIRE_SIZES(n, S, hr_bytes);
    OFASR_REQUIRE(lr_bytes > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(S % f == 0, OFASR_ERR_INVALID_ARG, "%s: crop side %lld is no multiple of the scale %lld", name,
                  (long long)S, (long long)f);
    OFASR_REQUIRE(yuv_coeffs_ok(coeffs, 6), OFASR_ERR_INVALID_ARG, "%s: coefficient outside the 14-bit tables' range", name);
    // as in ofasr_aug_gather_yuv420, per pool: the smallest even-sided frame of its crop must fit
    const int64_t s = S / f, Se = (S + 1) & ~(int64_t)1, se = (s + 1) & ~(int64_t)1;
    OFASR_REQUIRE(hr_bytes >= Se * Se * 3 / 2, OFASR_ERR_UNSUPPORTED,
                  "%s: an HR pool of %lld bytes holds no 4:2:0 frame of at least %lldx%lld (even H, W >= S)", name,
                  (long long)hr_bytes, (long long)Se, (long long)Se);
    OFASR_REQUIRE(lr_bytes >= se * se * 3 / 2, OFASR_ERR_UNSUPPORTED,
                  "%s: an LR pool of %lld bytes holds no 4:2:0 frame of at least %lldx%lld (even h, w >= S / f)", name,
                  (long long)lr_bytes, (long long)se, (long long)se);
    const AugSide hr{(const uint8_t*)hr_pool, (long long)hr_bytes, (const long long*)table, (int)S, (uint8_t*)hr_u8,
                     (float*)hr_f32};
    const AugSide lr{(const uint8_t*)lr_pool, (long long)lr_bytes, (const long long*)table + 12 * n, (int)s,
                     (uint8_t*)lr_u8, (float*)lr_f32};
    aug_gather_pair(hr, lr, n, yuv_dec(coeffs), as_stream(stream));
    return check_launch(name);
}

OFASR_EXPORT int ofasr_aug_gather_u8(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t n, int64_t S,
                                     void* out_u8, void* out_f32, void* stream) {
    const char* name = "ofasr_aug_gather_u8";
    OFASR_REQUIRE(pool && table && out_u8, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    AUG_REQUIRE_SIZES(n, S, pool_bytes);
    // the table lives on the device: the smallest pool that can hold one H, W >= S image is what the host can check
    OFASR_REQUIRE(pool_bytes >= 3 * S * S, OFASR_ERR_UNSUPPORTED,
                  "%s: a pool of %lld bytes holds no image of at least %lldx%lld (H, W >= S)", name, (long long)pool_bytes,
                  (long long)S, (long long)S);
    aug_gather<false>(pool, pool_bytes, table, n, S, YuvDec{}, out_u8, out_f32, as_stream(stream));
    return check_launch(name);
}

OFASR_EXPORT int ofasr_aug_select(const void* pool, int64_t pool_bytes, const int64_t* cand, int64_t blocks, int64_t n,
                                  int64_t K, int64_t S, int layout, int64_t* out_table, int32_t* choice, int64_t* activity,
                                  int64_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "ofasr_aug_select";
    OFASR_REQUIRE(pool && cand && out_table && choice && activity, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(K >= 1 && K <= AUG_SELECT_MAX_K, OFASR_ERR_UNSUPPORTED, "%s: %lld candidates per sample (1 .. %d)", name,
                  (long long)K, AUG_SELECT_MAX_K);
    OFASR_REQUIRE(layout == OFASR_AUG_RGB_HWC || layout == OFASR_AUG_YUV420, OFASR_ERR_INVALID_ARG,
                  "%s: layout %d is neither OFASR_AUG_RGB_HWC nor OFASR_AUG_YUV420", name, layout);
    OFASR_REQUIRE(blocks == 1 || blocks == 2, OFASR_ERR_INVALID_ARG, "%s: %lld table blocks (1, or 2 for a paired set)", name,
                  (long long)blocks);
    AUG_REQUIRE_SIZES(n, S, pool_bytes);
    OFASR_REQUIRE(n * K <= 65535, OFASR_ERR_UNSUPPORTED, "%s: %lld candidates in one launch (at most 65535)", name,
                  (long long)(n * K));
    // as the gathers: the smallest pool that can hold one image (one even-sided frame) with H, W >= S
    const int64_t Se = (S + 1) & ~(int64_t)1;
    const int64_t least = layout == OFASR_AUG_YUV420 ? Se * Se * 3 / 2 : 3 * S * S;
    OFASR_REQUIRE(pool_bytes >= least, OFASR_ERR_UNSUPPORTED, "%s: a pool of %lld bytes holds no image of at least %lldx%lld",
                  name, (long long)pool_bytes, (long long)S, (long long)S);
    OFASR_REQUIRE(((reinterpret_cast<uintptr_t>(cand) | reinterpret_cast<uintptr_t>(out_table) |
                    reinterpret_cast<uintptr_t>(activity) | reinterpret_cast<uintptr_t>(stats)) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(choice) & 3) == 0,
                  OFASR_ERR_INVALID_ARG, "%s: a table is not aligned for its element type", name);
    const int64_t strips = aug_select_strips(S);
    OFASR_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
                      workspace_bytes >= (size_t)(n * K * strips) * sizeof(int64_t),
                  OFASR_ERR_WORKSPACE, "%s: the workspace holds n * K * strips = %lld int64 words, 8-byte aligned", name,
                  (long long)(n * K * strips));
    const dim3 grid((unsigned)strips, (unsigned)(n * K));
    prof_note((double)(n * K) * (double)(S * S) * (layout == OFASR_AUG_YUV420 ? 1.0 : 3.0), 0.0);
    dispatch_int<1, 3>(layout == OFASR_AUG_YUV420 ? 1 : 3, [&](auto BPP) {      // bytes per pixel of the plane that is measured
        OFASR_LAUNCH(aug_select_activity_kernel<BPP>, grid, dim3(AUG_SELECT_THREADS), 0, as_stream(stream), (const uint8_t*)pool,
                     (long long)pool_bytes, (const long long*)cand, (int)S, (long long*)workspace);
    });
    prof_note((double)n * (double)K * (8.0 * (double)strips + 8.0) + (double)n * (double)blocks * 192.0, 0.0);
    OFASR_LAUNCH(aug_select_choose_kernel, dim3((unsigned)n), dim3(64), 0, as_stream(stream), (const long long*)workspace,
                 (int)strips, (const long long*)cand, (int)blocks, (long long)n, (int)K, (long long*)out_table, (int*)choice,
                 (long long*)activity, (unsigned long long*)stats);
    return check_launch(name);
}
