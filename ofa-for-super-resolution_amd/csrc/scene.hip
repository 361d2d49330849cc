// scene.hip -- scene cuts of a planar YUV 4:2:0 video: the per-channel colour histogram of a frame with the decode fused
// in (ofasr_rgb_hist_yuv420 / ofasr_rgb_hist_yuv420p16) and the fold of its partials into one histogram plus the squared
// distance to the previous frame's (ofasr_hist_fold_distance).  The host statement is scenes.py (rgb_histogram_host /
// frame_distance_host): with RGB the decode of yuv.hip's header (video.yuv420_to_rgb_host) of the WHOLE frame and
// P = H * W,
//   hist[c][b] = #{pixels whose channel c has bin b},  b = value at depth 8, value >> 2 at depth 10;  sum_b hist[c][b] = P
//   d(prev, cur) = sum_c sum_b (cur[c][b] - prev[c][b])^2 <= 6 P^2  (three channels, all mass moved from one bin to another)
// All of it is integer arithmetic: counts are uint32 (P <= 2^28), the distance int64 (6 P^2 < 2^63 for P <= 2^28, which
// is why these entry points cap the frame there and not at the tile kernels' 2^40).  No RGB frame is written: the kernel
// reads the 1.5 P samples once and stores 3 KB per workgroup.
// histogram: grid (x: row slab of the H / 2 block rows; hist_slabs / slab_rows).  A lane owns a 2 x 4 pixel block whose
//          corner is even in both coordinates and decodes it with yuv_decode_block (yuv_block.h: chroma at clamped
//          indices, luma rows as one wide load where the address is aligned for it and the block is whole, sample by
//          sample elsewhere; every load inside the planes).  A block cut by the right edge (W % 4 == 2) counts its two
//          valid columns; the repeated ones are not counted.  The workgroup counts into LDS with LDS integer atomics, one
//          [3][256] uint32 copy per wave, and then stores its own partial[s][3][256] with plain stores: no global
//          atomics, one writer per word, and integer sums do not depend on their order, so two calls give identical bytes.
//          Flat content (letterbox bars, slides) would send every lane to ONE LDS word, so equal values are merged
//          before the atomic: per channel, where the bin is the same across the wave's active lanes one lane adds the
//          wave's pixel count (the wave-uniform path); elsewhere a lane adds each DISTINCT bin of its up to 8 pixels once,
//          with its multiplicity (the in-lane merge).
//          The workgroup is 1024 lanes, one 2 x 4 block each per trip: a slab of two block rows of a 1920-wide frame is
//          one trip, so a 1080p frame costs one round of loads (with 256 lanes it was four dependent rounds on one wave
//          per SIMD, and latency-bound at that).
// fold:    ONE workgroup of 1024 threads.  Wave w folds the slabs s = w, w + 16, ...; lane q of it holds bins 4 q .. 4 q + 3
//          of each channel, read as one 16-byte load where `partial` is aligned for it, word by word elsewhere.  The 16
//          wave sums meet in LDS; thread t < 768 adds them in wave order, stores word t of hist_out, and the 768 squared
//          differences to hist_prev are summed through LDS in a fixed order; thread 0 stores the int64.  (Thread t
//          folding bin t over all slabs alone, 256 threads, took 112 us for the 270 slabs of a 1080p frame: 810
//          dependent-latency loads per thread on one compute unit.)
#include "yuv_block.h"

namespace ofasr {

static const int HIST_THREADS = 1024;
static const int HIST_WAVES = HIST_THREADS / 64;
static_assert(HIST_THREADS >= 768 && HIST_THREADS % 64 == 0, "thread t < 768 stores word t of a [3][256] table");
static const int HIST_MAX_SLABS = 1024;
// pixels of a frame per workgroup, about: two block rows of a 1920-wide frame (960 blocks, one trip of the workgroup), so
// 1080p is cut into 270 slabs, one workgroup for each of the 256 compute units and a few over
static const long long HIST_SLAB_SAMPLES = 7680;
static const long long HIST_MAX_PIXELS = 1LL << 28;

// slabs of the H / 2 block rows of an H x W frame: 1 .. min(H / 2, HIST_MAX_SLABS), every slab of slab_rows(H / 2, s, S)
// non-empty; 0 for a frame these entry points refuse
__host__ inline int64_t hist_slabs(int64_t H, int64_t W) {
    if (H < 2 || W < 2 || H % 2 || W % 2 || H > HIST_MAX_PIXELS / W) return 0;
    const int64_t R = H / 2;
    int64_t s = cdiv(H * W, HIST_SLAB_SAMPLES);
    s = s < HIST_MAX_SLABS ? s : HIST_MAX_SLABS;
    s = s < R ? s : R;
    const int64_t per = cdiv(R, s);                      // block rows of a slab; the last slab may own fewer
    return cdiv(R, per);
}

template <typename P> __device__ __forceinline__ int hist_bin(int v) { return yuv_px<P>::maxv == 255 ? v : v >> 2; }

template <typename P>
__global__ void __launch_bounds__(HIST_THREADS) rgb_hist_yuv420_kernel(const P* __restrict__ yp, const P* __restrict__ up,
                                                                       const P* __restrict__ vp, long long H, long long W,
                                                                       YuvDec D, uint32_t* __restrict__ partial) {
    __shared__ uint32_t cnt[HIST_WAVES][3][256];
    for (int i = threadIdx.x; i < HIST_WAVES * 3 * 256; i += HIST_THREADS) (&cnt[0][0][0])[i] = 0u;
    __syncthreads();
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id();
    long long lo, hi;
    slab_rows(H >> 1, blockIdx.x, gridDim.x, lo, hi);
    const long long G = (W + 3) >> 2;
    const long long items = (hi - lo) * G;
    // the trip count is the workgroup's, so whole waves reach the ballots; the active lanes of a wave are a prefix of it
    for (long long e0 = 0; e0 < items; e0 += HIST_THREADS) {
        const long long e = e0 + threadIdx.x;
        const bool active = e < items;
        int rgb[2][4][3];
        int valid = 0;
        if (active) {
            const long long br = e / G;
            const long long by = (lo + br) * 2, bx = (e - br * G) * 4;
            yuv_decode_block(yp, up, vp, H, W, by, bx, D, rgb);
            valid = bx + 4 <= W ? 4 : 2;
        }
        const unsigned long long am = __ballot(active);
        if (am == 0ull) continue;                                        // wave-uniform
        const int wave_px = 8 * __popcll(am) - 4 * __popcll(__ballot(active && valid == 2));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            int b[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) b[i] = active ? hist_bin<P>(rgb[i >> 2][i & 3][c]) : 0;
            bool same = true;                                            // the lane's valid pixels share one bin
#pragma unroll
            for (int i = 1; i < 8; ++i) same = same && ((i & 3) >= valid || b[i] == b[0]);
            const int first = __builtin_amdgcn_readfirstlane(b[0]);      // lane 0 is active here
            if (__ballot(active && same && b[0] == first) == am) {       // the wave-uniform path
                if (lane == 0) atomicAdd(&cnt[wave][c][first], (uint32_t)wave_px);
            } else if (active) {                                         // the in-lane merge
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if ((i & 3) >= valid) continue;
                    bool seen = false;
                    int m = 1;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const bool eq = (j & 3) < valid && b[j] == b[i];
                        if (j < i) seen = seen || eq;
                        if (j > i) m += eq ? 1 : 0;
                    }
                    if (!seen) atomicAdd(&cnt[wave][c][b[i]], (uint32_t)m);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 768) {                                                 // word t of the slab's [3][256]
        uint32_t s = 0;
#pragma unroll
        for (int q = 0; q < HIST_WAVES; ++q) s += (&cnt[q][0][0])[threadIdx.x];
        partial[(long long)blockIdx.x * 768 + threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(HIST_THREADS) hist_fold_distance_kernel(const uint32_t* __restrict__ partial, long long S,
                                                                          uint32_t* __restrict__ hist_out,
                                                                          const uint32_t* __restrict__ hist_prev,
                                                                          long long* __restrict__ dist_out) {
    __shared__ uint32_t part[HIST_WAVES][768];
    __shared__ long long red[HIST_THREADS];
    const int t = (int)threadIdx.x, wave = t >> 6, q = lane_id();
    const bool wide = (reinterpret_cast<uintptr_t>(partial) & 15) == 0;     // every [3][256] table is 3072 bytes
    uint32_t h[3][4] = {};
    for (long long s = wave; s < S; s += HIST_WAVES) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t* p = partial + (s * 3 + c) * 256 + 4 * q;
            if (wide) {
                const uint4 w = *reinterpret_cast<const uint4*>(p);
                h[c][0] += w.x, h[c][1] += w.y, h[c][2] += w.z, h[c][3] += w.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) h[c][k] += p[k];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) part[wave][c * 256 + 4 * q + k] = h[c][k];
    __syncthreads();
    long long acc = 0;
    if (t < 768) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < HIST_WAVES; ++w) sum += part[w][t];
        hist_out[t] = sum;
        if (hist_prev) {
            const long long d = (long long)sum - (long long)hist_prev[t];
            acc = d * d;
        }
    }
    red[t] = acc;
    __syncthreads();
#pragma unroll
    for (int o = HIST_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) *dist_out = red[0];
}

template <typename P>
static int rgb_hist(const char* name, const void* y, const void* u, const void* v, int64_t H, int64_t W, const int32_t* coeffs,
                    uint32_t* partial, void* stream) {
    OFASR_REQUIRE(y && u && v && coeffs && partial, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 3) == 0, OFASR_ERR_INVALID_ARG,
                  "%s: the partial table is not 4-byte aligned", name);
    YUV_REQUIRE_FRAME(H, W);
    OFASR_REQUIRE(H <= HIST_MAX_PIXELS / W, OFASR_ERR_UNSUPPORTED,
                  "%s: a frame of more than 2^28 pixels (%lldx%lld): the distance's bound 6 P^2 would leave int64", name,
                  (long long)W, (long long)H);
    OFASR_REQUIRE(yuv_coeffs_ok(coeffs, 6), OFASR_ERR_INVALID_ARG, "%s: coefficient outside the 14-bit tables' range", name);
    const int64_t S = hist_slabs(H, W);
    prof_note((double)(H * W) * 1.5 * sizeof(P), 0.0);
    OFASR_LAUNCH(rgb_hist_yuv420_kernel<P>, dim3((unsigned)S), dim3(HIST_THREADS), 0, as_stream(stream), (const P*)y,
                 (const P*)u, (const P*)v, (long long)H, (long long)W, yuv_dec(coeffs), partial);
    return check_launch(name);
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int64_t ofasr_rgb_hist_slabs(int64_t H, int64_t W) { return hist_slabs(H, W); }

OFASR_EXPORT int ofasr_rgb_hist_yuv420(const void* y, const void* u, const void* v, int64_t H, int64_t W, const int32_t* coeffs,
                                       uint32_t* partial, void* stream) {
    return rgb_hist<uint8_t>("ofasr_rgb_hist_yuv420", y, u, v, H, W, coeffs, partial, stream);
}

OFASR_EXPORT int ofasr_rgb_hist_yuv420p16(const void* y, const void* u, const void* v, int64_t H, int64_t W, int depth,
                                          const int32_t* coeffs, uint32_t* partial, void* stream) {
    const char* name = "ofasr_rgb_hist_yuv420p16";
    YUV_REQUIRE_P16(depth, y, u, v);
    return rgb_hist<uint16_t>(name, y, u, v, H, W, coeffs, partial, stream);
}

OFASR_EXPORT int ofasr_hist_fold_distance(const uint32_t* partial, int64_t slabs, uint32_t* hist_out, const uint32_t* hist_prev,
                                          int64_t* dist_out, void* stream) {
    const char* name = "ofasr_hist_fold_distance";
    OFASR_REQUIRE(partial && hist_out && dist_out, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(slabs > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(slabs <= HIST_MAX_SLABS, OFASR_ERR_INVALID_ARG, "%s: more than %d slabs", name, HIST_MAX_SLABS);
    OFASR_REQUIRE(((reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(hist_out) |
                    reinterpret_cast<uintptr_t>(hist_prev)) & 3) == 0 && (reinterpret_cast<uintptr_t>(dist_out) & 7) == 0,
                  OFASR_ERR_INVALID_ARG, "%s: a table is not aligned for its element type", name);
    OFASR_REQUIRE(hist_out != hist_prev, OFASR_ERR_INVALID_ARG, "%s: hist_out and hist_prev are the same table", name);
    prof_note((double)slabs * 3072.0 + (hist_prev ? 6144.0 : 3072.0), 0.0);
    OFASR_LAUNCH(hist_fold_distance_kernel, dim3(1), dim3(HIST_THREADS), 0, as_stream(stream), partial, (long long)slabs,
                 hist_out, hist_prev, (long long*)dist_out);
    return check_launch(name);
}
