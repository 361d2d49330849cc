// resize_scatter.hip -- the scatter of tiled inference with a Pillow-exact resize fused in (ofasr_tile_resize_scatter_u8 /
// _yuv420 / _yuv420p16): the output of a batch of windows goes straight to an image or frame of a TARGET size between the
// input's and the network's own, with no full-size frame and no intermediate image in HBM.  Host definition: resize.py
// (Pillow's precompute_coeffs / normalize_coeffs_8bpc / horizontal pass -> clip -> vertical pass -> clip, at 8 bits, and
// the same arithmetic with 1023 and 20 coefficient bits at 10); upscale.py argues why a window's target rectangle reads
// only pixels of that window that equal the whole-image forward's.
//
// The coefficient tables are computed on the HOST (double, libm's sin) and uploaded once per plan: int32 rows
// (xmin, count, k[0 .. ksize)) per target row (vtab) and per target column (htab), the layout of rs_coeff_kernel
// (resample.hip); xmin is a FULL-SIZE source coordinate, the window's origin in that frame is in its table row.
//
// One workgroup (256 threads) owns an RS_TY x RS_TX = 16 x 64 tile of a window's target rectangle:
//   1. horizontal pass into LDS.  The tile's rows need the source rows [ylo, ylo + span), span <= RS_ROWS = 96 (16 target
//      rows at a 4 : 1 reduction advance 64 source rows, plus the 25 taps of lanczos there).  A lane owns one (source row,
//      target column) at a time, consecutive lanes consecutive columns; per tap it reads the three planes of the network
//      output (fp32 / bf16 / f16), quantises on load as the existing scatters do (clamp, * P in fp32, rint; P = 255 or
//      1023) and accumulates in 32 bits; (acc + 2^(bits-1)) >> bits, clipped, is Pillow's intermediate image and is what
//      the LDS holds, as 8-bit samples for 8-bit sinks and 16-bit samples for the 10-bit sink.
//   2. vertical pass from LDS, then the sink: HWC uint8 RGB (a lane owns a pixel), or planar YUV 4:2:0 (a lane owns a
//      2 x 4 pixel block at an even position and encodes and stores it with yuv_block.h's yuv_encode_block /
//      yuv_store_block, the code the full-size scatter uses).
// LDS: 3 * 96 * 64 samples = 18 KiB (8-bit) / 36 KiB (16-bit).  No scratch.
//
// Addressing is 64-bit.  Every access stays inside its tensor whatever the device tables hold: the table row's target
// rectangle is clamped by scatter_dest (tile_table.h: the destination half of ofasr_tile_scatter_u8's rule), xmin /
// count to the table's width, every source index into the window and every LDS row into the tile's span.  A wrong table
// gives wrong values, never a fault.  All loads sit inside the branch that bounds them.  The accumulators are unsigned,
// so a wild coefficient wraps instead of overflowing; with tables of resize.py they stay inside int32 as Pillow's do.
#include "yuv_block.h"

namespace ofasr {

constexpr int RS_TY = 16, RS_TX = 64, RS_ROWS = 96, RS_TAPS = 25;

struct RszSinkRgb { uint8_t* img; };
template <typename P> struct RszSinkYuv { P* y; P* u; P* v; YuvEnc E; };

// sums of the vertical pass for target row `r` of the tile, column `col`: the three channels
template <typename P, int BITS>
__device__ __forceinline__ void rsz_vertical(const P* mid, const int* __restrict__ vrow, int kh, long long ybase, int span, int col,
                                             int (&rgb)[3]) {
    const int cnt = clampi(vrow[1], 0, kh);
    const long long y0 = (long long)vrow[0] - ybase;       // first tap's row inside the tile's span
    uint32_t acc[3] = {1u << (BITS - 1), 1u << (BITS - 1), 1u << (BITS - 1)};
    for (int k = 0; k < cnt; ++k) {
        const int yl = clampi(y0 + k, 0, span - 1);
        const uint32_t w = (uint32_t)vrow[2 + k];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += (uint32_t)mid[(c * RS_ROWS + yl) * RS_TX + col] * w;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = yuv_clampv<P>((int)acc[c] >> BITS);
}

// table[6 n ..]: oy, ox (the window's origin in full-size source pixels), dy, dx, eh, ew (its target rectangle).
// grid: (x: ceil(max_eh / 16) * ceil(max_ew / 64) tiles, y: window)
template <typename T, typename P, bool YUV, typename Sink>
__global__ void __launch_bounds__(256) tile_resize_scatter_kernel(const T* __restrict__ src, long long sh_, long long sw,
                                                                  const long long* __restrict__ table,
                                                                  const int* __restrict__ vtab, int kh,
                                                                  const int* __restrict__ htab, int kw, Sink sink,
                                                                  long long TH, long long TW, long long max_eh,
                                                                  long long max_ew) {
    constexpr int BITS = 32 - (sizeof(P) == 1 ? 8 : 10) - 2;
    __shared__ P mid[3 * RS_ROWS * RS_TX];
    const long long n = blockIdx.y;
    const ScatterRow t = scatter_dest(table, n, TH, TW, max_eh, max_ew, YUV);   // YUV: whole 2 x 2 blocks only
    const long long oy = t.sy, ox = t.sx, dy = t.dy, dx = t.dx, eh = t.eh, ew = t.ew;
    const long long tiles_x = (max_ew + RS_TX - 1) / RS_TX;
    const long long ty = (long long)blockIdx.x / tiles_x, tx = (long long)blockIdx.x - ty * tiles_x;
    const long long r0 = ty * RS_TY, c0 = tx * RS_TX;
    if (r0 >= eh || c0 >= ew) return;                          // the same for the whole workgroup: no barrier is skipped
    const int nr = (int)(eh - r0 < RS_TY ? eh - r0 : RS_TY), nc = (int)(ew - c0 < RS_TX ? ew - c0 : RS_TX);
    const int vs = 2 + kh, hs = 2 + kw;
    const int* vt = vtab + (dy + r0) * vs;                     // rows dy + r0 .. dy + r0 + nr - 1 < TH
    const int* ht = htab + (dx + c0) * hs;
    // the source rows of the tile, window-local: from the first row's first tap to the last row's last
    const int ylo = clampi((long long)vt[0] - oy, 0, sh_ - 1);
    const int* vl = vt + (long long)(nr - 1) * vs;
    const long long yhi = (long long)vl[0] + clampi(vl[1], 0, kh) - oy;
    int span = clampi(yhi - ylo, 1, RS_ROWS);
    span = span > sh_ - ylo ? (int)(sh_ - ylo) : span;
    const long long plane = sh_ * sw;
    const T* sn = src + n * 3 * plane + (long long)ylo * sw;

    // 1. horizontal pass: mid[c][row][col] for row < span, col < nc
    for (int e = threadIdx.x; e < span * RS_TX; e += 256) {
        const int row = e / RS_TX, col = e % RS_TX;
        if (col < nc) {
            const int* h = ht + (long long)col * hs;
            const int cnt = clampi(h[1], 0, kw);
            const long long x0 = (long long)h[0] - ox;
            const T* s = sn + (long long)row * sw;
            uint32_t acc[3] = {1u << (BITS - 1), 1u << (BITS - 1), 1u << (BITS - 1)};
            for (int k = 0; k < cnt; ++k) {
                const int xl = clampi(x0 + k, 0, sw - 1);
                const uint32_t w = (uint32_t)h[2 + k];
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += (uint32_t)quant<yuv_px<P>::maxv>(to_float(s[c * plane + xl])) * w;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) mid[(c * RS_ROWS + row) * RS_TX + col] = (P)yuv_clampv<P>((int)acc[c] >> BITS);
        }
    }
    __syncthreads();

    // 2. vertical pass and the sink
    const long long ybase = oy + ylo;
    if constexpr (!YUV) {
        for (int e = threadIdx.x; e < nr * RS_TX; e += 256) {
            const int r = e / RS_TX, col = e % RS_TX;
            if (col < nc) {
                int rgb[3];
                rsz_vertical<P, BITS>(mid, vt + (long long)r * vs, kh, ybase, span, col, rgb);
                uint8_t* d = sink.img + ((dy + r0 + r) * TW + dx + c0 + col) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) d[c] = (uint8_t)rgb[c];
            }
        }
    } else {
        constexpr int BX = RS_TX / 4;
        for (int e = threadIdx.x; e < (nr >> 1) * BX; e += 256) {     // nr, nc are even
            const int br = e / BX, b0 = (e % BX) * 4;
            if (b0 < nc) {
                const int valid = b0 + 4 <= nc ? 4 : 2;
                int rgb[2][4][3];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (k < valid) {
                            rsz_vertical<P, BITS>(mid, vt + (long long)(2 * br + r) * vs, kh, ybase, span, b0 + k, rgb[r][k]);
                        } else {
                            rgb[r][k][0] = rgb[r][k][1] = rgb[r][k][2] = 0;
                        }
                    }
                int Y[2][4], U[2], V[2];
                yuv_encode_block<P>(rgb, sink.E, Y, U, V);
                yuv_store_block(sink.y, sink.u, sink.v, TW, dy + r0 + 2 * br, dx + c0 + b0, valid, Y, U, V);
            }
        }
    }
}

template <typename T, typename P, bool YUV, typename Sink>
static void rsz_launch(const void* src, int64_t n, int64_t sh, int64_t sw, const int64_t* table, const int32_t* vtab, int kh,
                       const int32_t* htab, int kw, Sink sink, int64_t TH, int64_t TW, int64_t max_eh, int64_t max_ew,
                       hipStream_t st) {
    const dim3 grid((unsigned)(cdiv(max_eh, RS_TY) * cdiv(max_ew, RS_TX)), (unsigned)n);
    prof_note((double)n * (double)(max_eh * max_ew) * ((YUV ? 1.5 : 3.0) * sizeof(P)) + (double)n * (double)(sh * sw) * 3.0 * sizeof(T),
              0.0);
    OFASR_LAUNCH((tile_resize_scatter_kernel<T, P, YUV, Sink>), grid, dim3(256), 0, st, (const T*)src, (long long)sh,
                 (long long)sw, (const long long*)table, (const int*)vtab, kh, (const int*)htab, kw, sink, (long long)TH,
                 (long long)TW, (long long)max_eh, (long long)max_ew);
}

template <typename P, bool YUV, typename Sink>
static int rsz_dispatch(const char* name, const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                        const int32_t* vtab, int kh, const int32_t* htab, int kw, Sink sink, int64_t TH, int64_t TW,
                        int64_t max_eh, int64_t max_ew, void* stream) {
    OFASR_REQUIRE(src && table && vtab && htab, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && sh > 0 && sw > 0 && TH > 0 && TW > 0 && max_eh > 0 && max_ew > 0, OFASR_ERR_INVALID_ARG,
                  "%s: non-positive size", name);
    OFASR_REQUIRE_DTYPE(dtype);
    OFASR_REQUIRE(kh >= 1 && kw >= 1, OFASR_ERR_INVALID_ARG, "%s: a coefficient table without taps", name);
    OFASR_REQUIRE(kh <= RS_TAPS && kw <= RS_TAPS, OFASR_ERR_UNSUPPORTED,
                  "%s: %d x %d taps; at most %d per axis (lanczos at a 4 : 1 reduction)", name, kh, kw, RS_TAPS);
    OFASR_REQUIRE(max_eh <= TH && max_ew <= TW, OFASR_ERR_INVALID_ARG, "%s: extent bound larger than the target", name);
    OFASR_REQUIRE(n <= 65535 && TH <= (1LL << 40) / TW && sh <= (1LL << 30) && sw <= (1LL << 30) && sh <= (1LL << 40) / sw &&
                      cdiv(max_eh, RS_TY) * cdiv(max_ew, RS_TX) <= 0x7fffffffLL,
                  OFASR_ERR_UNSUPPORTED, "%s: too many windows or too large an image", name);
    hipStream_t st = as_stream(stream);
    dispatch_float(dtype, [&](auto t) {
        rsz_launch<typename decltype(t)::type, P, YUV>(src, n, sh, sw, table, vtab, kh, htab, kw, sink, TH, TW, max_eh, max_ew, st);
    });
    return check_launch(name);
}

template <typename P>
static int rsz_yuv(const char* name, const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                   const int32_t* vtab, int kh, const int32_t* htab, int kw, const int32_t* coeffs, void* y, void* u, void* v,
                   int64_t TH, int64_t TW, int64_t max_eh, int64_t max_ew, void* stream) {
    OFASR_REQUIRE(coeffs && y && u && v, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(TH >= 2 && TW >= 2, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(TH % 2 == 0 && TW % 2 == 0, OFASR_ERR_INVALID_ARG, "%s: a 4:2:0 frame needs even sides, got %lldx%lld", name,
                  (long long)TH, (long long)TW);
    OFASR_REQUIRE(yuv_coeffs_ok(coeffs, 10), OFASR_ERR_INVALID_ARG, "%s: coefficient outside the 14-bit tables' range", name);
    const RszSinkYuv<P> sink{(P*)y, (P*)u, (P*)v, yuv_enc(coeffs)};
    return rsz_dispatch<P, true>(name, src, n, sh, sw, dtype, table, vtab, kh, htab, kw, sink, TH, TW, max_eh, max_ew, stream);
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int ofasr_tile_resize_scatter_u8(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype,
                                              const int64_t* table, const int32_t* vtab, int kh, const int32_t* htab, int kw,
                                              void* img, int64_t TH, int64_t TW, int64_t max_eh, int64_t max_ew, void* stream) {
    const char* name = "ofasr_tile_resize_scatter_u8";
    OFASR_REQUIRE(img, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    const RszSinkRgb sink{(uint8_t*)img};
    return rsz_dispatch<uint8_t, false>(name, src, n, sh, sw, dtype, table, vtab, kh, htab, kw, sink, TH, TW, max_eh, max_ew,
                                        stream);
}

OFASR_EXPORT int ofasr_tile_resize_scatter_yuv420(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype,
                                                  const int64_t* table, const int32_t* vtab, int kh, const int32_t* htab,
                                                  int kw, const int32_t* coeffs, void* y, void* u, void* v, int64_t TH,
                                                  int64_t TW, int64_t max_eh, int64_t max_ew, void* stream) {
    return rsz_yuv<uint8_t>("ofasr_tile_resize_scatter_yuv420", src, n, sh, sw, dtype, table, vtab, kh, htab, kw, coeffs, y, u, v,
                            TH, TW, max_eh, max_ew, stream);
}

OFASR_EXPORT int ofasr_tile_resize_scatter_yuv420p16(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype,
                                                     const int64_t* table, const int32_t* vtab, int kh, const int32_t* htab,
                                                     int kw, int depth, const int32_t* coeffs, void* y, void* u, void* v,
                                                     int64_t TH, int64_t TW, int64_t max_eh, int64_t max_ew, void* stream) {
    const char* name = "ofasr_tile_resize_scatter_yuv420p16";
    YUV_REQUIRE_P16(depth, y, u, v);
    return rsz_yuv<uint16_t>(name, src, n, sh, sw, dtype, table, vtab, kh, htab, kw, coeffs, y, u, v, TH, TW, max_eh, max_ew,
                             stream);
}
