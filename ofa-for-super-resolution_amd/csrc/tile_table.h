// tile_table.h -- what the kernels of tiled inference share about their device tables, each rule stated once:
//   clampll / clampi      the one clamp;
//   window_origin         row n of an origin table [n][2], clamped so that the h x w window lies inside the H x W frame;
//   scatter_row / scatter_dest   row n of a scatter table [n][6], clamped so that the extent lies inside the source window
//                         and the destination (scatter_dest: the destination half alone);
//   window_slabs / slab_rows     how many row slabs a window is cut into and which rows a slab owns;
//   window_compact_by_class      the ordered compaction of plan rows by class in one workgroup;
//   pack4 / unpack4 / quant / grid_blocks   the 4-element accesses of a tile row (vec4: ofasr_common.h), the quantisation
//                         of network output, the grid size of a grid-stride kernel;
//   host side: the checks of a window table's entry point (TILE_REQUIRE_*; the dtype check and dispatch_float: launch.h).
// The clamps are __host__ __device__: tests/host/tile_table_check.hip runs them on the CPU over extreme rows and asserts
// the post-conditions that make every later access legal.  Everything is __forceinline__ and changes no access width.
#pragma once
#include "ofasr_common.h"

namespace ofasr {

__host__ __device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the same narrowed to int: for indices whose bounds fit one
__host__ __device__ __forceinline__ int clampi(long long v, long long lo, long long hi) { return (int)clampll(v, lo, hi); }

// ---- origin tables [n][2]: (y0, x0) ------------------------------------------------------------------------------------
struct WindowOrigin { long long y0, x0; };

// 0 <= y0 <= H - h and 0 <= x0 <= W - w whatever the table holds (the entry points require h <= H, w <= W)
__host__ __device__ __forceinline__ WindowOrigin window_origin(const long long* __restrict__ origins, long long n, long long H,
                                                               long long W, long long h, long long w) {
    return WindowOrigin{clampll(origins[2 * n], 0, H - h), clampll(origins[2 * n + 1], 0, W - w)};
}

// ---- scatter tables [n][6]: (sy, sx, dy, dx, eh, ew) -------------------------------------------------------------------
struct ScatterRow { long long sy, sx, dy, dx, eh, ew; };

// SRC: the first two columns are an offset into the sh x sw source window and bound the extent; without it they are
// passed through unclamped (the resize scatter keeps a full-size origin there) and sh, sw are not read.
// After it: 0 <= dy, dy + eh <= OH, 0 <= eh <= max_eh (x alike), with SRC also 0 <= sy, sy + eh <= sh (x alike); with
// `even`, dy, dx, eh, ew have their low bit cleared last (whole 2 x 2 blocks of a 4:2:0 frame: no chroma sample is
// half-owned), which keeps every inequality.  No step can overflow: every difference is of two values in [0, 2^63).
template <bool SRC>
__host__ __device__ __forceinline__ ScatterRow scatter_clamp(const long long* __restrict__ table, long long n, long long sh,
                                                             long long sw, long long OH, long long OW, long long max_eh,
                                                             long long max_ew, bool even) {
    const long long* t = table + 6 * n;
    long long sy = t[0], sx = t[1], dy = t[2], dx = t[3], eh = t[4], ew = t[5];
    if (SRC) {
        sy = clampll(sy, 0, sh);
        sx = clampll(sx, 0, sw);
    }
    dy = clampll(dy, 0, OH);
    dx = clampll(dx, 0, OW);
    eh = eh < 0 ? 0 : eh;
    ew = ew < 0 ? 0 : ew;
    eh = eh > max_eh ? max_eh : eh;
    ew = ew > max_ew ? max_ew : ew;
    if (SRC) eh = eh > sh - sy ? sh - sy : eh;
    eh = eh > OH - dy ? OH - dy : eh;
    if (SRC) ew = ew > sw - sx ? sw - sx : ew;
    ew = ew > OW - dx ? OW - dx : ew;
    if (even) dy &= ~1LL, dx &= ~1LL, eh &= ~1LL, ew &= ~1LL;
    return ScatterRow{sy, sx, dy, dx, eh, ew};
}
__host__ __device__ __forceinline__ ScatterRow scatter_row(const long long* __restrict__ table, long long n, long long sh,
                                                           long long sw, long long OH, long long OW, long long max_eh,
                                                           long long max_ew, bool even = false) {
    return scatter_clamp<true>(table, n, sh, sw, OH, OW, max_eh, max_ew, even);
}
__host__ __device__ __forceinline__ ScatterRow scatter_dest(const long long* __restrict__ table, long long n, long long OH,
                                                            long long OW, long long max_eh, long long max_ew, bool even) {
    return scatter_clamp<false>(table, n, 0, 0, OH, OW, max_eh, max_ew, even);
}

// ---- row slabs of a window ---------------------------------------------------------------------------------------------
constexpr int WINDOW_THREADS = 256;                   // the workgroup of the per-slab kernels and of the compaction
constexpr int WINDOW_MAX_SLABS = 64;

// slabs of an h x w window at about per_slab samples (bytes) a workgroup: 1 .. min(h, WINDOW_MAX_SLABS); 0 for no window
inline int64_t window_slabs(int64_t h, int64_t w, int64_t per_slab) {
    if (h <= 0 || w <= 0) return 0;
    int64_t s = h <= (1LL << 40) / w ? cdiv(h * w, per_slab) : WINDOW_MAX_SLABS;
    s = s < WINDOW_MAX_SLABS ? s : WINDOW_MAX_SLABS;
    s = s < h ? s : h;
    return s < 1 ? 1 : s;
}

// rows [lo, hi) of an nrows-tall rectangle that slab s of S owns
__host__ __device__ __forceinline__ void slab_rows(long long nrows, long long s, long long S, long long& lo, long long& hi) {
    const long long per = (nrows + S - 1) / S;
    lo = s * per < nrows ? s * per : nrows;
    hi = lo + per < nrows ? lo + per : nrows;
}

// ---- 4 elements of a tile row, quantisation, grid size -------------------------------------------------------------------
template <typename T> __device__ __forceinline__ typename vec4<T>::type pack4(const float* v);
template <> __device__ __forceinline__ float4 pack4<float>(const float* v) { return make_float4(v[0], v[1], v[2], v[3]); }
template <> __device__ __forceinline__ uint2 pack4<bf16_t>(const float* v) {
    return make_uint2(pack2<bf16_t>(v[0], v[1]), pack2<bf16_t>(v[2], v[3]));
}
template <> __device__ __forceinline__ uint2 pack4<f16_t>(const float* v) {
    return make_uint2(pack2<f16_t>(v[0], v[1]), pack2<f16_t>(v[2], v[3]));
}
template <typename T> __device__ __forceinline__ void unpack4(typename vec4<T>::type p, float* v);
template <> __device__ __forceinline__ void unpack4<float>(float4 p, float* v) { v[0] = p.x, v[1] = p.y, v[2] = p.z, v[3] = p.w; }
template <> __device__ __forceinline__ void unpack4<bf16_t>(uint2 p, float* v) {
    unpack2<bf16_t>(p.x, v[0], v[1]);
    unpack2<bf16_t>(p.y, v[2], v[3]);
}
template <> __device__ __forceinline__ void unpack4<f16_t>(uint2 p, float* v) {
    unpack2<f16_t>(p.x, v[0], v[1]);
    unpack2<f16_t>(p.y, v[2], v[3]);
}

// network output to a sample of 0 .. MAXV (255 or 1023): clamp, * MAXV in fp32, round half to even
template <int MAXV> __device__ __forceinline__ int quant(float v) {
    const float f = fminf(fmaxf(v, 0.0f), 1.0f);
    return (int)rintf(__fmul_rn(f, (float)MAXV));
}

// blocks of 256 lanes for `work` items of a grid-stride loop: 1 .. 4096
inline unsigned grid_blocks(long long work) {
    const long long b = cdiv(work, 256);
    return (unsigned)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

// ---- ordered compaction of plan rows by class ------------------------------------------------------------------------------
// ONE workgroup of WINDOW_THREADS.  cls_of(i) is the class of plan row i < n, 0 .. NC - 1, or -1 for a row that goes into
// no list.  Per round of 256 rows and per class: ballot + popcount inside the wave, the four wave totals through LDS; the
// rows of class c go out in plan order into out_origins [NC][rows][2] (rows = ceil(n / B) * B), out_table [NC][n][6] and
// out_index [NC][n], their number into count [NC]; each class's last batch is filled up by repeating its last window's
// origin (an empty class: nothing to fill).  Rows past those are not written.  Every position is < n: no store leaves
// its table.
template <int NC, typename Classify>
__device__ __forceinline__ void window_compact_by_class(Classify cls_of, const long long* __restrict__ origins,
                                                        const long long* __restrict__ table, long long n, long long B,
                                                        long long* __restrict__ out_origins, long long* __restrict__ out_table,
                                                        long long* __restrict__ out_index, long long* __restrict__ count) {
    __shared__ long long wave_total[NC][WINDOW_THREADS / 64];
    __shared__ long long last[NC];                      // plan index of the class's last window so far
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    const long long rows = (n + B - 1) / B * B;
    if ((int)threadIdx.x < NC) last[threadIdx.x] = 0;
    long long m[NC] = {};                               // windows of each class before this round (the same in every thread)
    for (long long i0 = 0; i0 < n; i0 += WINDOW_THREADS) {
        const long long i = i0 + threadIdx.x;
        const int cls = i < n ? cls_of(i) : -1;
        unsigned long long mask[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            mask[c] = __ballot(cls == c);
            if (lane == 0) wave_total[c][wave] = __popcll(mask[c]);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            long long before = m[c], tot = 0;
#pragma unroll
            for (int q = 0; q < WINDOW_THREADS / 64; ++q) {
                before += q < wave ? wave_total[c][q] : 0;
                tot += wave_total[c][q];
            }
            if (cls == c) {
                const long long pos = before + __popcll(mask[c] & ((1ull << lane) - 1ull));   // < n: positions are distinct
                long long* oo = out_origins + (c * rows + pos) * 2;
                oo[0] = origins[2 * i];
                oo[1] = origins[2 * i + 1];
                long long* ot = out_table + (c * n + pos) * 6;
#pragma unroll
                for (int q = 0; q < 6; ++q) ot[q] = table[6 * i + q];
                out_index[c * n + pos] = i;
                if (pos == m[c] + tot - 1) last[c] = i;  // one thread per class and round at most
            }
            m[c] += tot;
        }
        __syncthreads();                                 // wave_total is rewritten by the next round
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const long long padded = (m[c] + B - 1) / B * B; // <= rows
        const long long li = last[c];
        for (long long j = m[c] + threadIdx.x; j < padded; j += WINDOW_THREADS) {
            out_origins[(c * rows + j) * 2] = origins[2 * li];
            out_origins[(c * rows + j) * 2 + 1] = origins[2 * li + 1];
        }
    }
    if ((int)threadIdx.x < NC) {
        long long mine = m[0];
#pragma unroll
        for (int c = 1; c < NC; ++c) mine = (int)threadIdx.x == c ? m[c] : mine;
        count[threadIdx.x] = mine;
    }
}

}  // namespace ofasr

// ---- host side ---------------------------------------------------------------------------------------------------------
// The checks of an entry point that takes a window table; `name` is the entry point's.  The sizes are positive already.
#define TILE_REQUIRE_FRAME_CAP(H, W)                                                                                   \
    OFASR_REQUIRE((H) <= (1LL << 40) / (W), OFASR_ERR_UNSUPPORTED, "%s: too large a frame", name)
// at most 65535 rows (grid.y) and an H x W frame of at most 2^40 pixels; `msg` is the entry point's own wording
#define TILE_REQUIRE_COUNT(n, H, W, msg)                                                                                \
    OFASR_REQUIRE((n) <= 65535 && (H) <= (1LL << 40) / (W), OFASR_ERR_UNSUPPORTED, "%s: " msg, name)
// h x w windows inside the H x W frame (`what`: "image" or "frame"), then TILE_REQUIRE_COUNT
#define TILE_REQUIRE_WINDOWS(n, h, w, H, W, what, msg)                                                                  \
    OFASR_REQUIRE((h) <= (H) && (w) <= (W), OFASR_ERR_INVALID_ARG, "%s: window %lldx%lld larger than the " what " %lldx%lld", \
                  name, (long long)(h), (long long)(w), (long long)(H), (long long)(W));                                \
    TILE_REQUIRE_COUNT(n, H, W, msg)
