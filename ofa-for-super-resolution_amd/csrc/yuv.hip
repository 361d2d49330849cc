// yuv.hip -- planar 8-bit YUV 4:2:0 frames: the whole-frame colour conversions (ofasr_yuv420_to_rgb_u8 /
// ofasr_rgb_to_yuv420_u8) and the tile moves of tiled inference with the conversion fused in
// (ofasr_tile_gather_yuv420 / ofasr_tile_scatter_yuv420).  The host statement is video.py (yuv420_to_rgb_host /
// rgb_to_yuv420_host); everything is integer arithmetic on 14-bit coefficients, so host and device agree bit for bit:
//   decode: chroma to full resolution by the centre-sited 9-3-3-1 filter, edge replication at the FRAME edge:
//             c = (9 C[cy0, cx0] + 3 C[cy0, nx] + 3 C[ny, cx0] + C[ny, nx] + 8) >> 4,   cy0 = y >> 1, cx0 = x >> 1,
//             ny = cy0 - 1 for even y, cy0 + 1 for odd y (nx alike from x), both clamped into the plane;
//           R = clamp((cy y' + rv v + 2^13) >> 14), G = clamp((cy y' + gu u + gv v + 2^13) >> 14),
//           B = clamp((cy y' + bu u + 2^13) >> 14)   with y' = Y - yo, u = c_U - 128, v = c_V - 128
//   encode: Y = clamp(((yr R + yg G + yb B + 2^13) >> 14) + yo) per pixel;
//           U = clamp(((sum over the 2x2 block of (ur R + ug G + ub B) + 2^15) >> 16) + 128), V alike
// The tile moves are the ones of tile_io.hip with these in front / behind:
//   gather:  out[n, c, r, x] = (T)(RGB_c(y0_n + r, x0_n + x) / 255.0f), RGB the decode at frame coordinates
//   scatter: the 2x2 blocks of quant<255>(src) (clamp, * 255 in fp32, rintf) encoded into the three planes
// so no RGB frame exists on either side of the network.  Addressing is 64-bit throughout.  Every access stays inside its
// tensor whatever the device tables hold: origins, offsets and extents are clamped in the kernels by window_origin and
// scatter_row with its `even` rule (tile_table.h).
//
// Access widths.  A lane owns a 2-row x 4-column pixel block whose corner is even in both frame coordinates, i.e. two
// whole chroma samples per plane: a decode fetches the 3 x 4 chroma neighbourhood of the block once per plane (byte loads
// at clamped indices) and the two luma rows as dwords; an encode writes two luma dwords and one 16-bit chroma pair per
// plane.  The wide accesses are taken only where the address is aligned for them and the block is whole; blocks cut by
// the frame's or an extent's edge and unaligned rows go byte by byte (element by element on the tile side).  A window
// with an odd origin is gathered as the even-aligned superset of the window, the pixels outside it masked.
//
// 16-bit planes (ofasr_tile_gather_yuv420p16 / ofasr_tile_scatter_yuv420p16, depth 10).  The same kernels on the sample
// type uint16_t (yuv_px<P>): a sample s is read as min(s, 1023), 512 takes the place of 128 and 1023 that of 255, in the
// clamps, in the gather's division and in the scatter's quantisation; the caller's tables are the ones of depth 10.  The
// widths double in bytes and stay the same in samples: a luma row of a block is one 8-byte access, a chroma pair one
// 32-bit store, under the same conditions (address aligned for it, block whole), samples one by one elsewhere.  Every
// stored word is <= 1023.  The 8-bit instantiations are what they were before the sample type became a parameter.
#include "yuv_block.h"

namespace ofasr {

// ---- whole frame ---------------------------------------------------------------------------------------------------
// grid: lanes over (H / 2) * ceil(W / 4) blocks in a grid-stride loop
__global__ void __launch_bounds__(256) yuv420_to_rgb_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ up,
                                                            const uint8_t* __restrict__ vp, long long H, long long W, YuvDec D,
                                                            uint8_t* __restrict__ rgb_out) {
    const long long G = (W + 3) >> 2;
    const long long total = (H >> 1) * G;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long br = e / G;
        const long long by = br * 2, bx = (e - br * G) * 4;
        int rgb[2][4][3];
        yuv_decode_block(yp, up, vp, H, W, by, bx, D, rgb);
        const int valid = bx + 4 <= W ? 4 : 2;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint8_t* d = rgb_out + ((by + r) * W + bx) * 3;
            if ((reinterpret_cast<uintptr_t>(d) & 3) == 0 && valid == 4) {
                uint32_t b[12];
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) b[3 * k + c] = (uint32_t)rgb[r][k][c];
                uint32_t* d4 = reinterpret_cast<uint32_t*>(d);
#pragma unroll
                for (int q = 0; q < 3; ++q) d4[q] = b[4 * q] | b[4 * q + 1] << 8 | b[4 * q + 2] << 16 | b[4 * q + 3] << 24;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < valid) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) d[3 * k + c] = (uint8_t)rgb[r][k][c];
                    }
            }
        }
    }
}

__global__ void __launch_bounds__(256) rgb_to_yuv420_kernel(const uint8_t* __restrict__ rgb_in, long long H, long long W,
                                                            YuvEnc E, uint8_t* __restrict__ yp, uint8_t* __restrict__ up,
                                                            uint8_t* __restrict__ vp) {
    const long long G = (W + 3) >> 2;
    const long long total = (H >> 1) * G;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long br = e / G;
        const long long by = br * 2, bx = (e - br * G) * 4;
        const int valid = bx + 4 <= W ? 4 : 2;
        int rgb[2][4][3];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint8_t* s = rgb_in + ((by + r) * W + bx) * 3;
            if ((reinterpret_cast<uintptr_t>(s) & 3) == 0 && valid == 4) {
                const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
                const uint32_t w[3] = {s4[0], s4[1], s4[2]};
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int i = 3 * k + c;
                        rgb[r][k][c] = (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
                    }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) rgb[r][k][c] = k < valid ? (int)s[3 * k + c] : 0;
            }
        }
        int Y[2][4], U[2], V[2];
        yuv_encode_block<uint8_t>(rgb, E, Y, U, V);
        yuv_store_block(yp, up, vp, W, by, bx, valid, Y, U, V);
    }
}

// ---- tiles ---------------------------------------------------------------------------------------------------------
// grid: (x: lanes over (h / 2 + 1) * (w / 4 + 1) blocks of the even-aligned superset of the window, y: window).
// vec_ok: w % 4 == 0 and `out` aligned for 4-element stores (then a window with an even x0 stores whole rows of a block)
template <typename T, typename P>
__global__ void __launch_bounds__(256) tile_gather_yuv420_kernel(const P* __restrict__ yp, const P* __restrict__ up,
                                                                 const P* __restrict__ vp, long long H, long long W,
                                                                 YuvDec D, const long long* __restrict__ origins, long long h,
                                                                 long long w, T* __restrict__ out, int vec_ok) {
    const long long n = blockIdx.y;
    const WindowOrigin o0 = window_origin(origins, n, H, W, h, w);
    const long long y0 = o0.y0, x0 = o0.x0;
    const long long ey0 = y0 & ~1LL, ex0 = x0 & ~1LL;
    const long long G = (w >> 2) + 1;                 // ceil((w + 1) / 4) <= w / 4 + 1 columns of blocks
    const long long R = (h >> 1) + 1;
    const long long plane = h * w;
    T* on = out + n * 3 * plane;
    const bool vec = vec_ok && x0 == ex0;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < R * G; e += (long long)gridDim.x * blockDim.x) {
        const long long br = e / G;
        const long long by = ey0 + br * 2, bx = ex0 + (e - br * G) * 4;
        if (by >= y0 + h || bx >= x0 + w) continue;
        int rgb[2][4][3];
        yuv_decode_block(yp, up, vp, H, W, by, bx, D, rgb);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long long wr = by + r - y0;           // window row
            if (wr < 0 || wr >= h) continue;
            const long long wx = bx - x0;               // window column of the block's first pixel (-1 for an odd x0)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = __fdiv_rn((float)rgb[r][k][c], (float)yuv_px<P>::maxv);
                T* dst = on + c * plane + wr * w + wx;
                if (vec) {                              // x0 even and w % 4 == 0: wx % 4 == 0 and the block is whole
                    *reinterpret_cast<typename vec4<T>::type*>(dst) = pack4<T>(v);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (wx + k >= 0 && wx + k < w) dst[k] = from_float<T>(v[k]);
                }
            }
        }
    }
}

// table[6 n ..]: sy, sx, dy, dx, eh, ew (dy, dx, eh, ew made even after the clamps).
// grid: (x: lanes over ceil(max_eh / 2) * ceil(max_ew / 4) blocks, y: window)
template <typename T, typename P>
__global__ void __launch_bounds__(256) tile_scatter_yuv420_kernel(const T* __restrict__ src, long long sh_, long long sw,
                                                                  const long long* __restrict__ table, YuvEnc E,
                                                                  P* __restrict__ yp, P* __restrict__ up, P* __restrict__ vp,
                                                                  long long OH, long long OW, long long max_eh,
                                                                  long long max_ew) {
    const long long n = blockIdx.y;
    const ScatterRow t = scatter_row(table, n, sh_, sw, OH, OW, max_eh, max_ew, true);   // even: whole 2 x 2 blocks only
    const long long sy = t.sy, sx = t.sx, dy = t.dy, dx = t.dx, eh = t.eh, ew = t.ew;
    const long long G = (max_ew + 3) >> 2;
    const long long plane = sh_ * sw;
    const T* sn = src + n * 3 * plane;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < (eh >> 1) * G; e += (long long)gridDim.x * blockDim.x) {
        const long long br = e / G;
        const long long r0 = br * 2, c0 = (e - br * G) * 4;   // the block inside the extent
        if (c0 >= ew) continue;
        const int valid = c0 + 4 <= ew ? 4 : 2;
        int rgb[2][4][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const T* s = sn + c * plane + (sy + r0 + r) * sw + sx + c0;
                float v[4];
                if (valid == 4 && (reinterpret_cast<uintptr_t>(s) & (4 * sizeof(T) - 1)) == 0) {
                    unpack4<T>(*reinterpret_cast<const typename vec4<T>::type*>(s), v);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = k < valid ? to_float(s[k]) : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) rgb[r][k][c] = quant<yuv_px<P>::maxv>(v[k]);
            }
        int Y[2][4], U[2], V[2];
        yuv_encode_block<P>(rgb, E, Y, U, V);
        yuv_store_block(yp, up, vp, OW, dy + r0, dx + c0, valid, Y, U, V);
    }
}

template <typename T, typename P>
static void yuv_gather(const void* y, const void* u, const void* v, int64_t H, int64_t W, YuvDec D, const int64_t* origins,
                       int64_t n, int64_t h, int64_t w, void* out, hipStream_t st) {
    const size_t al = sizeof(T) == 4 ? 16 : 8;
    const int vec = w % 4 == 0 && reinterpret_cast<uintptr_t>(out) % al == 0;
    const dim3 grid(grid_blocks((h / 2 + 1) * (w / 4 + 1)), (unsigned)n);
    prof_note((double)n * (double)(h * w) * (1.5 * sizeof(P) + 3.0 * sizeof(T)), 0.0);
    OFASR_LAUNCH((tile_gather_yuv420_kernel<T, P>), grid, dim3(256), 0, st, (const P*)y, (const P*)u, (const P*)v,
                 (long long)H, (long long)W, D, (const long long*)origins, (long long)h, (long long)w, (T*)out, vec);
}

template <typename T, typename P>
static void yuv_scatter(const void* src, int64_t n, int64_t sh, int64_t sw, const int64_t* table, YuvEnc E, void* y, void* u,
                        void* v, int64_t OH, int64_t OW, int64_t max_eh, int64_t max_ew, hipStream_t st) {
    const dim3 grid(grid_blocks(cdiv(max_eh, 2) * cdiv(max_ew, 4)), (unsigned)n);
    prof_note((double)n * (double)(max_eh * max_ew) * (1.5 * sizeof(P) + 3.0 * sizeof(T)), 0.0);
    OFASR_LAUNCH((tile_scatter_yuv420_kernel<T, P>), grid, dim3(256), 0, st, (const T*)src, (long long)sh, (long long)sw,
                 (const long long*)table, E, (P*)y, (P*)u, (P*)v, (long long)OH, (long long)OW, (long long)max_eh,
                 (long long)max_ew);
}

}  // namespace ofasr

using namespace ofasr;

// the checks the tile moves share, whatever the sample type
template <typename P>
static int yuv_tile_gather(const char* name, const void* y, const void* u, const void* v, int64_t H, int64_t W,
                           const int32_t* coeffs, const int64_t* origins, int64_t n, int64_t h, int64_t w, void* out, int dtype,
                           void* stream) {
    OFASR_REQUIRE(y && u && v && coeffs && origins && out, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && h > 0 && w > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    YUV_REQUIRE_FRAME(H, W);
    OFASR_REQUIRE_DTYPE(dtype);
    TILE_REQUIRE_WINDOWS(n, h, w, H, W, "frame", "too many windows");
    OFASR_REQUIRE(yuv_coeffs_ok(coeffs, 6), OFASR_ERR_INVALID_ARG, "%s: coefficient outside the 14-bit tables' range", name);
    hipStream_t st = as_stream(stream);
    const YuvDec D = yuv_dec(coeffs);
    dispatch_float(dtype, [&](auto t) { yuv_gather<typename decltype(t)::type, P>(y, u, v, H, W, D, origins, n, h, w, out, st); });
    return check_launch(name);
}

template <typename P>
static int yuv_tile_scatter(const char* name, const void* src, int64_t n, int64_t sh, int64_t sw, int dtype,
                            const int64_t* table, const int32_t* coeffs, void* y, void* u, void* v, int64_t OH, int64_t OW,
                            int64_t max_eh, int64_t max_ew, void* stream) {
    OFASR_REQUIRE(src && table && coeffs && y && u && v, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && sh > 0 && sw > 0 && max_eh > 0 && max_ew > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    YUV_REQUIRE_FRAME(OH, OW);
    OFASR_REQUIRE_DTYPE(dtype);
    OFASR_REQUIRE(max_eh <= sh && max_ew <= sw, OFASR_ERR_INVALID_ARG, "%s: extent bound larger than the source window",
                  name);
    TILE_REQUIRE_COUNT(n, OH, OW, "too many windows");
    OFASR_REQUIRE(yuv_coeffs_ok(coeffs, 10), OFASR_ERR_INVALID_ARG, "%s: coefficient outside the 14-bit tables' range", name);
    hipStream_t st = as_stream(stream);
    const YuvEnc E = yuv_enc(coeffs);
    dispatch_float(dtype, [&](auto t) {
        yuv_scatter<typename decltype(t)::type, P>(src, n, sh, sw, table, E, y, u, v, OH, OW, max_eh, max_ew, st);
    });
    return check_launch(name);
}

OFASR_EXPORT int ofasr_yuv420_to_rgb_u8(const void* y, const void* u, const void* v, int64_t H, int64_t W,
                                        const int32_t* coeffs, void* rgb_hwc, void* stream) {
    const char* name = "ofasr_yuv420_to_rgb_u8";
    OFASR_REQUIRE(y && u && v && coeffs && rgb_hwc, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    YUV_REQUIRE_FRAME(H, W);
    OFASR_REQUIRE(yuv_coeffs_ok(coeffs, 6), OFASR_ERR_INVALID_ARG, "%s: coefficient outside the 14-bit tables' range", name);
    prof_note((double)(H * W) * 4.5, 0.0);
    OFASR_LAUNCH(yuv420_to_rgb_kernel, dim3(grid_blocks((H / 2) * cdiv(W, 4))), dim3(256), 0, as_stream(stream),
                 (const uint8_t*)y, (const uint8_t*)u, (const uint8_t*)v, (long long)H, (long long)W, yuv_dec(coeffs),
                 (uint8_t*)rgb_hwc);
    return check_launch(name);
}

OFASR_EXPORT int ofasr_rgb_to_yuv420_u8(const void* rgb_hwc, int64_t H, int64_t W, const int32_t* coeffs, void* y, void* u,
                                        void* v, void* stream) {
    const char* name = "ofasr_rgb_to_yuv420_u8";
    OFASR_REQUIRE(y && u && v && coeffs && rgb_hwc, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    YUV_REQUIRE_FRAME(H, W);
    OFASR_REQUIRE(yuv_coeffs_ok(coeffs, 10), OFASR_ERR_INVALID_ARG, "%s: coefficient outside the 14-bit tables' range", name);
    prof_note((double)(H * W) * 4.5, 0.0);
    OFASR_LAUNCH(rgb_to_yuv420_kernel, dim3(grid_blocks((H / 2) * cdiv(W, 4))), dim3(256), 0, as_stream(stream),
                 (const uint8_t*)rgb_hwc, (long long)H, (long long)W, yuv_enc(coeffs), (uint8_t*)y, (uint8_t*)u, (uint8_t*)v);
    return check_launch(name);
}

OFASR_EXPORT int ofasr_tile_gather_yuv420(const void* y, const void* u, const void* v, int64_t H, int64_t W,
                                          const int32_t* coeffs, const int64_t* origins, int64_t n, int64_t h, int64_t w,
                                          void* out, int dtype, void* stream) {
    return yuv_tile_gather<uint8_t>("ofasr_tile_gather_yuv420", y, u, v, H, W, coeffs, origins, n, h, w, out, dtype, stream);
}

OFASR_EXPORT int ofasr_tile_scatter_yuv420(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                                           const int32_t* coeffs, void* y, void* u, void* v, int64_t OH, int64_t OW,
                                           int64_t max_eh, int64_t max_ew, void* stream) {
    return yuv_tile_scatter<uint8_t>("ofasr_tile_scatter_yuv420", src, n, sh, sw, dtype, table, coeffs, y, u, v, OH, OW, max_eh,
                                     max_ew, stream);
}

OFASR_EXPORT int ofasr_tile_gather_yuv420p16(const void* y, const void* u, const void* v, int64_t H, int64_t W, int depth,
                                             const int32_t* coeffs, const int64_t* origins, int64_t n, int64_t h, int64_t w,
                                             void* out, int dtype, void* stream) {
    const char* name = "ofasr_tile_gather_yuv420p16";
    YUV_REQUIRE_P16(depth, y, u, v);
    return yuv_tile_gather<uint16_t>(name, y, u, v, H, W, coeffs, origins, n, h, w, out, dtype, stream);
}

OFASR_EXPORT int ofasr_tile_scatter_yuv420p16(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype,
                                              const int64_t* table, int depth, const int32_t* coeffs, void* y, void* u, void* v,
                                              int64_t OH, int64_t OW, int64_t max_eh, int64_t max_ew, void* stream) {
    const char* name = "ofasr_tile_scatter_yuv420p16";
    YUV_REQUIRE_P16(depth, y, u, v);
    return yuv_tile_scatter<uint16_t>(name, src, n, sh, sw, dtype, table, coeffs, y, u, v, OH, OW, max_eh, max_ew, stream);
}
