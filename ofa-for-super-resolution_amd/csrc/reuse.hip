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
//          The origin is window_origin's, the rows of a slab slab_rows' (tile_table.h).
// compact: ONE workgroup: window_compact_by_class (tile_table.h) with one class.  Per round of 256 windows: fold the S
//          slab flags, ballot + popcount inside the wave, the four wave totals through LDS; the changed windows' rows go
//          out in plan order.
#include "yuv_block.h"

namespace ofasr {

static const int REUSE_THREADS = WINDOW_THREADS;
static const long long REUSE_SLAB_BYTES = 16384;     // luma bytes of a window per workgroup, about

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

template <int BPS>                                    // bytes per sample: 1, or 2 for the 16-bit planes
__global__ void __launch_bounds__(REUSE_THREADS) window_diff_yuv420_kernel(
    const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up, const uint8_t* __restrict__ vp,
    const uint8_t* __restrict__ pyp, const uint8_t* __restrict__ pup, const uint8_t* __restrict__ pvp, long long H, long long W,
    const long long* __restrict__ origins, long long h, long long w, int* __restrict__ flags) {
    const long long n = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const WindowOrigin o0 = window_origin(origins, n, H, W, h, w);
    const long long y0 = o0.y0, x0 = o0.x0;
    const long long CH = H >> 1, CW = W >> 1;
    const long long cr0 = clampll((y0 - 1) >> 1, 0, CH - 1), cr1 = clampll((y0 + h) >> 1, 0, CH - 1);
    const long long cc0 = clampll((x0 - 1) >> 1, 0, CW - 1), cc1 = clampll((x0 + w) >> 1, 0, CW - 1);
    long long lo, hi;
    slab_rows(h, s, S, lo, hi);
    unsigned d = reuse_rect_diff(yp, pyp, W * BPS, y0 + lo, y0 + hi, x0 * BPS, w * BPS);
    slab_rows(cr1 - cr0 + 1, s, S, lo, hi);
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
    const auto changed = [&](long long i) {             // the one class: any slab flag set
        int f = 0;
        for (long long s = 0; s < S; ++s) f |= flags[i * S + s];
        return f ? 0 : -1;
    };
    window_compact_by_class<1>(changed, origins, table, n, B, out_origins, out_table, out_index, count);
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int64_t ofasr_window_diff_slabs(int64_t h, int64_t w) { return window_slabs(h, w, REUSE_SLAB_BYTES); }

template <int BPS>
static int reuse_window_diff(const char* name, const void* y, const void* u, const void* v, const void* py, const void* pu,
                             const void* pv, int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h, int64_t w,
                             int32_t* flags, void* stream) {
    OFASR_REQUIRE(y && u && v && py && pu && pv && origins && flags, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && h > 0 && w > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    YUV_REQUIRE_FRAME(H, W);
    TILE_REQUIRE_WINDOWS(n, h, w, H, W, "frame", "too many windows");
    const int64_t S = window_slabs(h, w, REUSE_SLAB_BYTES);
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
    YUV_REQUIRE_P16(depth, y, u, v, py, pu, pv);
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
    OFASR_REQUIRE(slabs <= WINDOW_MAX_SLABS, OFASR_ERR_INVALID_ARG, "%s: more than %d slabs", name, WINDOW_MAX_SLABS);
    prof_note((double)n * (4.0 * (double)slabs + 136.0), 0.0);
    OFASR_LAUNCH(window_compact_kernel, dim3(1), dim3(REUSE_THREADS), 0, as_stream(stream), (const int*)flags, (long long)slabs,
                 (const long long*)origins, (const long long*)table, (long long)n, (long long)batch, (long long*)out_origins,
                 (long long*)out_table, (long long*)out_index, (long long*)count);
    return check_launch(name);
}
