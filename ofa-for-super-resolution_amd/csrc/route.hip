// route.hip -- content-aware routing of tile windows between two networks (upscale.py, TiledUpscaler(easy_net=...)): the
// luma activity of every window of a tile plan (ofasr_window_activity_rgb8 / ofasr_window_activity_plane) and the two-way
// compaction of the plan's tables by class (ofasr_window_route).  The host statement is routing.py:
//   L   the luma sample: the plane's sample as stored, or (77 R + 150 G + 29 B + 128) >> 8 of an RGB pixel
//   A   of the h x w window at the clamped origin (y0, x0): the sum of |L[r][c + 1] - L[r][c]| over r < h, c < w - 1 and of
//       |L[r + 1][c] - L[r][c]| over r < h - 1, c < w, rows and columns counted inside the window rectangle
//   a window is easy iff A <= limit (two int64 values), hard otherwise.
// activity: grid (x: row slab, y: window), as window_diff_yuv420_kernel (csrc/reuse.hip).  A slab owns the horizontal terms
//          of its rows and the vertical terms whose upper row it owns; the workgroup stores ONE int64,
//          partial[n * S + s] (S = ofasr_window_activity_slabs(h, w)): no atomics, one writer per word.  A row is cut
//          into a head of fewer than 16 samples, up to the first sample whose address is 16-byte aligned, and chunks of
//          16 samples behind it; a chunk that lies whole inside the row is read with 16-byte loads where its address is
//          aligned for them (upper and lower row decided separately), everything else sample by sample.  Every load is
//          predicated on the sample lying inside the window rectangle, which lies inside the plane.  A work item sums at
//          most 32 differences of at most 65535 in int32; everything above it is int64.  64-bit addressing.
//          The origin is window_origin's, the rows of a slab slab_rows' (tile_table.h).
// route:   ONE workgroup, as window_compact_kernel: window_compact_by_class (tile_table.h) with two classes.  Per round
//          of 256 windows: fold the S partials, compare with limit, fold the S' changed flags if there are any; per
//          class ballot + popcount inside the wave, the four wave totals through LDS; rows go out in plan order, class 0
//          (hard) and class 1 (easy) into their own tables.
#include "tile_table.h"

namespace ofasr {

static const int ROUTE_THREADS = WINDOW_THREADS;
static const long long ROUTE_SLAB_SAMPLES = 16384;    // samples of a window per workgroup, about

// sample j of a row: BPS 1 / 2: the stored sample; BPS 3: the luma of the RGB pixel
template <int BPS> __device__ __forceinline__ int route_sample(const uint8_t* p, long long j) {
    if constexpr (BPS == 1) {
        return p[j];
    } else if constexpr (BPS == 2) {
        return reinterpret_cast<const uint16_t*>(p)[j];
    } else {
        const uint8_t* q = p + 3 * j;
        return (77 * (int)q[0] + 150 * (int)q[1] + 29 * (int)q[2] + 128) >> 8;
    }
}

// the same from the 16 * BPS bytes of an aligned chunk held in words
template <int BPS> __device__ __forceinline__ int route_unpack(const uint32_t (&wd)[4 * BPS], int j) {
    if constexpr (BPS == 1) {
        return (int)((wd[j >> 2] >> (8 * (j & 3))) & 0xffu);
    } else if constexpr (BPS == 2) {
        return (int)((wd[j >> 1] >> (16 * (j & 1))) & 0xffffu);
    } else {
        int c[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int b = 3 * j + q;
            c[q] = (int)((wd[b >> 2] >> (8 * (b & 3))) & 0xffu);
        }
        return (77 * c[0] + 150 * c[1] + 29 * c[2] + 128) >> 8;
    }
}

// v[j] = sample c0 + j of the row at `row` for j < cnt (cnt <= 16), 0 above; `row` points at the window's first sample
template <int BPS>
__device__ __forceinline__ void route_load16(const uint8_t* row, long long c0, int cnt, int (&v)[16]) {
    const uint8_t* p = row + c0 * BPS;
    if (cnt == 16 && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        uint32_t wd[4 * BPS];
#pragma unroll
        for (int q = 0; q < BPS; ++q) {
            const uint4 t = reinterpret_cast<const uint4*>(p)[q];
            wd[4 * q] = t.x, wd[4 * q + 1] = t.y, wd[4 * q + 2] = t.z, wd[4 * q + 3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = route_unpack<BPS>(wd, j);
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = j < cnt ? route_sample<BPS>(p, j) : 0;
    }
}

template <int BPS>                                    // bytes per sample: 1, 2 (16-bit planes) or 3 (interleaved RGB)
__global__ void __launch_bounds__(ROUTE_THREADS) window_activity_kernel(
    const uint8_t* __restrict__ src, long long H, long long W, const long long* __restrict__ origins, long long h, long long w,
    long long* __restrict__ partial) {
    __shared__ long long red[ROUTE_THREADS];
    const long long n = blockIdx.y, s = blockIdx.x, S = gridDim.x;
    const WindowOrigin o0 = window_origin(origins, n, H, W, h, w);
    const long long y0 = o0.y0, x0 = o0.x0;
    long long lo, hi;
    slab_rows(h, s, S, lo, hi);
    const long long K = ((w + 15) >> 4) + 1;           // the head and the chunks behind it
    const long long items = (hi - lo) * K;
    long long acc = 0;
    for (long long e = threadIdx.x; e < items; e += ROUTE_THREADS) {
        const long long r = lo + e / K, k = e % K;
        const uint8_t* row = src + ((y0 + r) * W + x0) * BPS;               // the window's first sample of row r
        const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15);
        const int gap = (16 - mis) & 15;                                    // bytes up to the next 16-byte boundary
        const long long head = BPS == 1 ? gap : BPS == 2 ? gap >> 1 : (gap * 11) & 15;   // 3 * 11 = 1 (mod 16)
        const long long c0 = k == 0 ? 0 : head + (k - 1) * 16;
        long long c1 = k == 0 ? head : c0 + 16;
        c1 = c1 < w ? c1 : w;
        if (c0 >= c1) continue;
        const int cnt = (int)(c1 - c0);
        int a[16], b[16];
        route_load16<BPS>(row, c0, cnt, a);
        int sum = 0;
#pragma unroll
        for (int j = 0; j + 1 < 16; ++j) sum += j + 1 < cnt ? abs(a[j + 1] - a[j]) : 0;
        if (c1 < w) {                                                       // the term that leaves the chunk to the right
            int last = a[0];
#pragma unroll
            for (int j = 1; j < 16; ++j) last = j < cnt ? a[j] : last;
            sum += abs(route_sample<BPS>(row, c1) - last);
        }
        if (r + 1 < h) {                                                    // the vertical terms whose upper row is r
            route_load16<BPS>(row + W * BPS, c0, cnt, b);
#pragma unroll
            for (int j = 0; j < 16; ++j) sum += j < cnt ? abs(b[j] - a[j]) : 0;
        }
        acc += sum;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int o = ROUTE_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[n * S + s] = red[0];
}

// out_origins [2][rows][2] (rows = ceil(n / B) * B), out_table [2][n][6], out_index [2][n], count [2]; include/ofasr.h
__global__ void __launch_bounds__(ROUTE_THREADS) window_route_kernel(
    const long long* __restrict__ partial, long long S, long long limit, const int* __restrict__ changed, long long CS,
    const long long* __restrict__ origins, const long long* __restrict__ table, long long n, long long B,
    long long* __restrict__ out_origins, long long* __restrict__ out_table, long long* __restrict__ out_index,
    long long* __restrict__ count) {
    const auto cls_of = [&](long long i) {              // 0: hard, 1: easy, -1: unchanged, in neither list
        int f = 1;
        if (changed) {
            f = 0;
            for (long long s = 0; s < CS; ++s) f |= changed[i * CS + s];
        }
        int cls = -1;
        if (f) {
            long long A = 0;
            for (long long s = 0; s < S; ++s) A += partial[i * S + s];
            cls = A <= limit ? 1 : 0;
        }
        return cls;
    };
    window_compact_by_class<2>(cls_of, origins, table, n, B, out_origins, out_table, out_index, count);
}

template <int BPS>
static int route_window_activity(const char* name, const void* src, int64_t H, int64_t W, const int64_t* origins, int64_t n,
                                 int64_t h, int64_t w, int64_t* partial, void* stream) {
    OFASR_REQUIRE(src && origins && partial, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && h > 0 && w > 0 && H > 0 && W > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    TILE_REQUIRE_FRAME_CAP(H, W);
    TILE_REQUIRE_WINDOWS(n, h, w, H, W, "frame", "too many windows");
    const int64_t S = window_slabs(h, w, ROUTE_SLAB_SAMPLES);
    prof_note((double)n * (double)(h * w) * BPS, 0.0);
    OFASR_LAUNCH(window_activity_kernel<BPS>, dim3((unsigned)S, (unsigned)n), dim3(ROUTE_THREADS), 0, as_stream(stream),
                 (const uint8_t*)src, (long long)H, (long long)W, (const long long*)origins, (long long)h, (long long)w,
                 (long long*)partial);
    return check_launch(name);
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int64_t ofasr_window_activity_slabs(int64_t h, int64_t w) { return window_slabs(h, w, ROUTE_SLAB_SAMPLES); }

OFASR_EXPORT int ofasr_window_activity_rgb8(const void* img, int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h,
                                            int64_t w, int64_t* partial, void* stream) {
    return route_window_activity<3>("ofasr_window_activity_rgb8", img, H, W, origins, n, h, w, partial, stream);
}

OFASR_EXPORT int ofasr_window_activity_plane(const void* plane, int64_t H, int64_t W, int depth, const int64_t* origins,
                                             int64_t n, int64_t h, int64_t w, int64_t* partial, void* stream) {
    const char* name = "ofasr_window_activity_plane";
    OFASR_REQUIRE(depth == 8 || depth == 10, OFASR_ERR_INVALID_ARG, "%s: depth %d is not supported (8 or 10)", name, depth);
    if (depth == 8) return route_window_activity<1>(name, plane, H, W, origins, n, h, w, partial, stream);
    OFASR_REQUIRE((reinterpret_cast<uintptr_t>(plane) & 1) == 0, OFASR_ERR_INVALID_ARG,
                  "%s: a 16-bit plane pointer is not 2-byte aligned", name);
    return route_window_activity<2>(name, plane, H, W, origins, n, h, w, partial, stream);
}

OFASR_EXPORT int ofasr_window_route(const int64_t* partial, int64_t slabs, int64_t limit, const int32_t* changed,
                                    int64_t changed_slabs, const int64_t* origins, const int64_t* table, int64_t n,
                                    int64_t batch, int64_t* out_origins, int64_t* out_table, int64_t* out_index, int64_t* count,
                                    void* stream) {
    const char* name = "ofasr_window_route";
    OFASR_REQUIRE(partial && origins && table && out_origins && out_table && out_index && count, OFASR_ERR_INVALID_ARG,
                  "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && batch > 0 && slabs > 0 && (!changed || changed_slabs > 0), OFASR_ERR_INVALID_ARG,
                  "%s: non-positive size", name);
    OFASR_REQUIRE(n <= 65535 && batch <= 65535, OFASR_ERR_UNSUPPORTED, "%s: too many windows", name);
    OFASR_REQUIRE(slabs <= WINDOW_MAX_SLABS && (!changed || changed_slabs <= WINDOW_MAX_SLABS), OFASR_ERR_INVALID_ARG,
                  "%s: more than %d slabs", name, WINDOW_MAX_SLABS);
    prof_note((double)n * (8.0 * (double)slabs + (changed ? 4.0 * (double)changed_slabs : 0.0) + 136.0), 0.0);
    OFASR_LAUNCH(window_route_kernel, dim3(1), dim3(ROUTE_THREADS), 0, as_stream(stream), (const long long*)partial,
                 (long long)slabs, (long long)limit, (const int*)changed, (long long)(changed ? changed_slabs : 0),
                 (const long long*)origins, (const long long*)table, (long long)n, (long long)batch, (long long*)out_origins,
                 (long long*)out_table, (long long*)out_index, (long long*)count);
    return check_launch(name);
}
