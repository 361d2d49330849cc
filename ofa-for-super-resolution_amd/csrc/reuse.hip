// reuse.hip -- which windows of a tile plan changed between two planar YUV 4:2:0 frames (ofasr_window_diff_yuv420) and
// the compacted tables of those windows (ofasr_window_compact), for upscale.py's YUV420Stream: a window whose input
// bytes are those of the previous frame keeps the previous frame's output core, so only changed windows run the network.
// The host statement is video.py (window_support / changed_windows_host):
//   support of window n at the clamped origin (y0, x0):
//     luma    rows y0 .. y0 + h - 1,                                   columns x0 .. x0 + w - 1
//     chroma  rows max(0, (y0 - 1) >> 1) .. min(H/2 - 1, (y0 + h) >> 1),   columns alike from x0, w, W
//   (the reach of ofasr_tile_gather_yuv420's 9-3-3-1 decode, the neighbour tap included); a window is changed iff any
//   byte of its support differs between the two frames, in y, u or v.
// diff:    grid (x: row slab, y: window).  A workgroup compares its slab of rows of the three rectangles and stores ONE
//          int32, flags[n * S + s] (S = ofasr_window_diff_slabs(h, w)); no atomics, every flag has one writer.
//          A row is cut into the 16-byte chunks of its own address: a chunk that lies whole inside the row is two
//          dwordx4 loads when the two planes' addresses are both 16-byte aligned there, every other chunk goes byte by
//          byte.  A lane touches memory only inside `if (in range)`: there is no load from a masked lane, so no address
//          needs a clamp beyond the origin's.  64-bit addressing.
//          16-bit planes (ofasr_window_diff_yuv420p16): the same kernel with BPS = 2 bytes per sample.  The support is the
//          same in samples; the rectangles are compared as bytes, pitch, first column and width doubled, so the stored
//          words are compared as they are (bits above the tenth included) and a word is never split across two flags.
// compact: ONE workgroup.  Per round of 256 windows: fold the S slab flags, ballot + popcount inside the wave, the four
//          wave totals through LDS; the changed windows' rows go out in plan order.
#include "ofasr_common.h"

namespace ofasr {

static const int REUSE_THREADS = 256;
static const int REUSE_MAX_SLABS = 64;
static const long long REUSE_SLAB_BYTES = 16384;     // luma bytes of a window per workgroup, about

__device__ __forceinline__ long long reuse_clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// OR of cur ^ prev over rows [r0, r1) x columns [c0, c0 + nc) of two [*, pitch] byte planes, this thread's share.
// The caller guarantees the rectangle lies inside the planes.
__device__ __forceinline__ unsigned reuse_rect_diff(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev,
                                                    long long pitch, long long r0, long long r1, long long c0, long long nc) {
    unsigned d = 0;
    const long long K = ((nc + 15) >> 4) + 1;          // chunks of a row: the head may be cut, so one more than ceil(nc / 16)
    const long long items = (r1 - r0) * K;
    for (long long e = threadIdx.x; e < items; e += blockDim.x) {
        const long long r = e / K, k = e - r * K;
        const long long base = (r0 + r) * pitch + c0;                       // the row's first byte, in both planes
        const uint8_t* a = cur + base;
        const uint8_t* b = prev + base;
        const long long mis = (long long)(reinterpret_cast<uintptr_t>(a) & 15);
        const long long o = k * 16 - mis;                                   // chunk k starts at a + o, a 16-byte boundary
        if (o >= nc) continue;
        if (o >= 0 && o + 16 <= nc && (reinterpret_cast<uintptr_t>(b + o) & 15) == 0) {
            const uint4 va = *reinterpret_cast<const uint4*>(a + o);
            const uint4 vb = *reinterpret_cast<const uint4*>(b + o);
            d |= (va.x ^ vb.x) | (va.y ^ vb.y) | (va.z ^ vb.z) | (va.w ^ vb.w);
        } else {
            const long long lo = o < 0 ? 0 : o, hi = o + 16 < nc ? o + 16 : nc;
            for (long long j = lo; j < hi; ++j) d |= (unsigned)(a[j] ^ b[j]);
        }
    }
    return d;
}

// rows [lo, hi) of an nrows-tall rectangle that slab s of S compares
__device__ __forceinline__ void reuse_slab_rows(long long nrows, long long s, long long S, long long& lo, long long& hi) {
    const long long per = (nrows + S - 1) / S;
    lo = s * per < nrows ? s * per : nrows;
    hi = lo + per < nrows ? lo + per : nrows;
}

template <int BPS>                                    // bytes per sample: 1, or 2 for the 16-bit planes
__global__ void __launch_bounds__(REUSE_THREADS) window_diff_yuv420_kernel(
    const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up, const uint8_t* __restrict__ vp,
    const uint8_t* __restrict__ pyp, const uint8_t* __restrict__ pup, const uint8_t* __restrict__ pvp, long long H, long long W,
    const long long* __restrict__ origins, long long h, long long w, int* __restrict__ flags) {
    const long long n = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const long long y0 = reuse_clampll(origins[2 * n], 0, H - h), x0 = reuse_clampll(origins[2 * n + 1], 0, W - w);
    const long long CH = H >> 1, CW = W >> 1;
    const long long cr0 = reuse_clampll((y0 - 1) >> 1, 0, CH - 1), cr1 = reuse_clampll((y0 + h) >> 1, 0, CH - 1);
    const long long cc0 = reuse_clampll((x0 - 1) >> 1, 0, CW - 1), cc1 = reuse_clampll((x0 + w) >> 1, 0, CW - 1);
    long long lo, hi;
    reuse_slab_rows(h, s, S, lo, hi);
    unsigned d = reuse_rect_diff(yp, pyp, W * BPS, y0 + lo, y0 + hi, x0 * BPS, w * BPS);
    reuse_slab_rows(cr1 - cr0 + 1, s, S, lo, hi);
    d |= reuse_rect_diff(up, pup, CW * BPS, cr0 + lo, cr0 + hi, cc0 * BPS, (cc1 - cc0 + 1) * BPS);
    d |= reuse_rect_diff(vp, pvp, CW * BPS, cr0 + lo, cr0 + hi, cc0 * BPS, (cc1 - cc0 + 1) * BPS);
    const int any = __syncthreads_or(d != 0);
    if (threadIdx.x == 0) flags[n * S + s] = any ? 1 : 0;
}

// out_origins [ceil(n / B) * B][2], out_table [n][6], out_index [n], count [1]; see include/ofasr.h
__global__ void __launch_bounds__(REUSE_THREADS) window_compact_kernel(
    const int* __restrict__ flags, long long S, const long long* __restrict__ origins, const long long* __restrict__ table,
    long long n, long long B, long long* __restrict__ out_origins, long long* __restrict__ out_table,
    long long* __restrict__ out_index, long long* __restrict__ count) {
    __shared__ long long wave_total[REUSE_THREADS / 64];
    __shared__ long long last;                          // plan index of the last changed window so far
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) last = 0;
    long long m = 0;                                    // changed windows before this round (the same in every thread)
    for (long long i0 = 0; i0 < n; i0 += REUSE_THREADS) {
        const long long i = i0 + threadIdx.x;
        int f = 0;
        if (i < n)
            for (long long s = 0; s < S; ++s) f |= flags[i * S + s];
        const unsigned long long mask = __ballot(f != 0);
        if (lane == 0) wave_total[wave] = __popcll(mask);
        __syncthreads();
        long long before = m, tot = 0;
#pragma unroll
        for (int q = 0; q < REUSE_THREADS / 64; ++q) {
            before += q < wave ? wave_total[q] : 0;
            tot += wave_total[q];
        }
        if (f) {
            const long long pos = before + __popcll(mask & ((1ull << lane) - 1ull));       // < n: positions are distinct
            out_origins[2 * pos] = origins[2 * i];
            out_origins[2 * pos + 1] = origins[2 * i + 1];
#pragma unroll
            for (int c = 0; c < 6; ++c) out_table[6 * pos + c] = table[6 * i + c];
            out_index[pos] = i;
            if (pos == m + tot - 1) last = i;            // one thread per round at most
        }
        m += tot;
        __syncthreads();                                 // wave_total is rewritten by the next round
    }
    // the last batch is filled up by repeating the last changed window (m = 0: nothing to fill)
    const long long padded = (m + B - 1) / B * B;        // <= ceil(n / B) * B
    for (long long j = m + threadIdx.x; j < padded; j += REUSE_THREADS) {
        out_origins[2 * j] = origins[2 * last];
        out_origins[2 * j + 1] = origins[2 * last + 1];
    }
    if (threadIdx.x == 0) count[0] = m;
}

static int64_t reuse_slabs(int64_t h, int64_t w) {
    if (h <= 0 || w <= 0) return 0;
    int64_t s = h <= (1LL << 40) / w ? cdiv(h * w, REUSE_SLAB_BYTES) : REUSE_MAX_SLABS;
    s = s < REUSE_MAX_SLABS ? s : REUSE_MAX_SLABS;
    s = s < h ? s : h;
    return s < 1 ? 1 : s;
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int64_t ofasr_window_diff_slabs(int64_t h, int64_t w) { return reuse_slabs(h, w); }

template <int BPS>
static int reuse_window_diff(const char* name, const void* y, const void* u, const void* v, const void* py, const void* pu,
                             const void* pv, int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h, int64_t w,
                             int32_t* flags, void* stream) {
    OFASR_REQUIRE(y && u && v && py && pu && pv && origins && flags, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && h > 0 && w > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(H >= 2 && W >= 2, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(H % 2 == 0 && W % 2 == 0, OFASR_ERR_INVALID_ARG, "%s: a 4:2:0 frame needs even sides, got %lldx%lld", name,
                  (long long)H, (long long)W);
    OFASR_REQUIRE(H <= (1LL << 40) / W, OFASR_ERR_UNSUPPORTED, "%s: too large a frame", name);
    OFASR_REQUIRE(h <= H && w <= W, OFASR_ERR_INVALID_ARG, "%s: window %lldx%lld larger than the frame %lldx%lld", name,
                  (long long)h, (long long)w, (long long)H, (long long)W);
    OFASR_REQUIRE(n <= 65535, OFASR_ERR_UNSUPPORTED, "%s: too many windows", name);
    const int64_t S = reuse_slabs(h, w);
    prof_note((double)n * (double)(h * w) * 3.0 * BPS, 0.0);
    OFASR_LAUNCH(window_diff_yuv420_kernel<BPS>, dim3((unsigned)S, (unsigned)n), dim3(REUSE_THREADS), 0, as_stream(stream),
                 (const uint8_t*)y, (const uint8_t*)u, (const uint8_t*)v, (const uint8_t*)py, (const uint8_t*)pu,
                 (const uint8_t*)pv, (long long)H, (long long)W, (const long long*)origins, (long long)h, (long long)w,
                 (int*)flags);
    return check_launch(name);
}

OFASR_EXPORT int ofasr_window_diff_yuv420(const void* y, const void* u, const void* v, const void* py, const void* pu,
                                          const void* pv, int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h,
                                          int64_t w, int32_t* flags, void* stream) {
    return reuse_window_diff<1>("ofasr_window_diff_yuv420", y, u, v, py, pu, pv, H, W, origins, n, h, w, flags, stream);
}

OFASR_EXPORT int ofasr_window_diff_yuv420p16(const void* y, const void* u, const void* v, const void* py, const void* pu,
                                             const void* pv, int64_t H, int64_t W, int depth, const int64_t* origins, int64_t n,
                                             int64_t h, int64_t w, int32_t* flags, void* stream) {
    const char* name = "ofasr_window_diff_yuv420p16";
    OFASR_REQUIRE(depth == 10, OFASR_ERR_INVALID_ARG, "%s: depth %d is not supported (10 only)", name, depth);
    uintptr_t bits = 0;
    for (const void* p : {y, u, v, py, pu, pv}) bits |= reinterpret_cast<uintptr_t>(p);
    OFASR_REQUIRE((bits & 1) == 0, OFASR_ERR_INVALID_ARG, "%s: a 16-bit plane pointer is not 2-byte aligned", name);
    return reuse_window_diff<2>(name, y, u, v, py, pu, pv, H, W, origins, n, h, w, flags, stream);
}

OFASR_EXPORT int ofasr_window_compact(const int32_t* flags, int64_t slabs, const int64_t* origins, const int64_t* table,
                                      int64_t n, int64_t batch, int64_t* out_origins, int64_t* out_table, int64_t* out_index,
                                      int64_t* count, void* stream) {
    const char* name = "ofasr_window_compact";
    OFASR_REQUIRE(flags && origins && table && out_origins && out_table && out_index && count, OFASR_ERR_INVALID_ARG,
                  "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && batch > 0 && slabs > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(n <= 65535 && batch <= 65535, OFASR_ERR_UNSUPPORTED, "%s: too many windows", name);
    OFASR_REQUIRE(slabs <= REUSE_MAX_SLABS, OFASR_ERR_INVALID_ARG, "%s: more than %d slabs", name, REUSE_MAX_SLABS);
    prof_note((double)n * (4.0 * (double)slabs + 136.0), 0.0);
    OFASR_LAUNCH(window_compact_kernel, dim3(1), dim3(REUSE_THREADS), 0, as_stream(stream), (const int*)flags, (long long)slabs,
                 (const long long*)origins, (const long long*)table, (long long)n, (long long)batch, (long long*)out_origins,
                 (long long*)out_table, (long long*)out_index, (long long*)count);
    return check_launch(name);
}
