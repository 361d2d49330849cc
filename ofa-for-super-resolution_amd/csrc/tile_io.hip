// tile_io.hip -- the 8-bit image <-> tile batch moves of tiled inference (ofasr_tile_gather_u8 / ofasr_tile_scatter_u8).
//
// upscale.py cuts an HWC uint8 RGB image into equally shaped windows, runs the static SR network on the batch of windows
// and writes the core of each window's output back into an HWC uint8 image.  Both moves are one launch per batch:
//   gather:  out[n, c, r, x] = (T)(img[y0_n + r, x0_n + x, c] / 255.0f)    (fp32 division: torchvision's ToTensor,
//            div2k_setxx.to_tensor, bit for bit; then one RNE cast to the 16-bit types)
//   scatter: img[dy_n + r, dx_n + x, c] = rint(min(max(src[n, c, sy_n + r, sx_n + x], 0), 1) * 255)    (the steps of
//            utils.tensor2img_np / psnr_y_device: clamp, * 255 in fp32, round half to even)
// Addressing is 64-bit throughout (a 4x output of an 8K input is > 2^31 bytes).  Every access stays inside its tensor
// whatever the device tables hold: origins and table rows are clamped into range in the kernel (window_origin /
// scatter_row, tile_table.h), and the uint8 side's aligned dword loads fall back to byte loads for the (at most two)
// words that straddle the ends of the image.
//
// Access widths.  gather: a lane owns 4 consecutive pixels of one window row: 12 bytes of HWC input read as 4 aligned
// dwords (funnel-shifted into place with v_alignbyte), 3 row-contiguous 4-element planar stores (16 B for fp32, 8 B for
// 16-bit; element stores when the window width or the output pointer is not aligned for them).  scatter: a lane owns
// the 4 pixels of an aligned 4-pixel group of the destination image (12 bytes = 3 aligned dwords, stored as one
// dwordx3) -- groups cut by the edge of a core are written byte by byte, since their other bytes belong to a neighbour
// core; the planar source reads are consecutive across the lanes of a wave.
#include "tile_table.h"

namespace ofasr {

struct alignas(4) tio_u32x3 { uint32_t a, b, c; };

// the aligned dword at absolute address q of the byte range [b, e); bytes outside it read as 0
__device__ __forceinline__ uint32_t tio_word(uintptr_t q, uintptr_t b, uintptr_t e) {
    if (q >= b && q + 4 <= e) return *reinterpret_cast<const uint32_t*>(q);
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (q + i >= b && q + i < e) v |= (uint32_t)(*reinterpret_cast<const uint8_t*>(q + i)) << (8 * i);
    return v;
}

// grid: (x: lanes over h * ceil(w / 4) in a grid-stride loop, y: window)
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) tile_gather_u8_kernel(const uint8_t* __restrict__ img, long long H, long long W,
                                                             const long long* __restrict__ origins, long long h,
                                                             long long w, T* __restrict__ out) {
    const long long n = blockIdx.y;
    const WindowOrigin o0 = window_origin(origins, n, H, W, h, w);
    const long long y0 = o0.y0, x0 = o0.x0;
    const uintptr_t ib = reinterpret_cast<uintptr_t>(img), ie = ib + (uintptr_t)(H * W * 3);
    const long long gw = (w + 3) >> 2;
    const long long plane = h * w;
    T* on = out + n * 3 * plane;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < h * gw; e += (long long)gridDim.x * blockDim.x) {
        const long long r = e / gw;
        const long long x = (e - r * gw) * 4;
        const uintptr_t a = ib + (uintptr_t)(((y0 + r) * W + x0 + x) * 3);
        const uintptr_t q = a & ~(uintptr_t)3;
        const int sh = (int)(a & 3);
        const uint32_t w0 = tio_word(q, ib, ie), w1 = tio_word(q + 4, ib, ie), w2 = tio_word(q + 8, ib, ie),
                       w3 = tio_word(q + 12, ib, ie);
        // the 12 bytes of pixels x .. x+3 (RGB RGB RGB RGB), in order
        const uint32_t b[3] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                               __builtin_amdgcn_alignbyte(w3, w2, sh)};
        const long long o = r * w + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 3 * j + c;
                v[j] = __fdiv_rn((float)((b[k >> 2] >> (8 * (k & 3))) & 0xffu), 255.0f);
            }
            T* dst = on + c * plane + o;
            if (VEC) {
                *reinterpret_cast<typename vec4<T>::type*>(dst) = pack4<T>(v);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < w) dst[j] = from_float<T>(v[j]);
            }
        }
    }
}

// table[6 n ..]: sy, sx, dy, dx, eh, ew.  grid: (x: lanes over max_eh * (max_ew / 4 + 2) groups, y: window)
template <typename T, bool WIDE>
__global__ void __launch_bounds__(256) tile_scatter_u8_kernel(const T* __restrict__ src, long long sh_, long long sw,
                                                              const long long* __restrict__ table, uint8_t* __restrict__ img,
                                                              long long OH, long long OW, long long max_eh,
                                                              long long max_ew) {
    const long long n = blockIdx.y;
    const ScatterRow t = scatter_row(table, n, sh_, sw, OH, OW, max_eh, max_ew);
    const long long sy = t.sy, sx = t.sx, dy = t.dy, dx = t.dx, eh = t.eh, ew = t.ew;
    const long long G = (max_ew >> 2) + 2;
    const long long plane = sh_ * sw;
    const T* sn = src + n * 3 * plane;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < eh * G; e += (long long)gridDim.x * blockDim.x) {
        const long long r = e / G;
        const long long F = (dy + r) * OW + dx;          // flat index of the row's first destination pixel
        const long long p0 = ((F >> 2) + (e - r * G)) << 2;
        if (p0 >= F + ew) continue;
        const T* s = sn + (sy + r) * sw + sx - F;        // s[p]: the source value of destination pixel p, plane 0
        uint32_t q[4][3];
        bool in[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long p = p0 + j;
            in[j] = p >= F && p < F + ew;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[j][c] = in[j] ? (uint32_t)quant<255>(to_float(s[c * plane + p])) : 0u;
        }
        uint8_t* d = img + p0 * 3;
        if (WIDE && in[0] && in[3]) {
            tio_u32x3 v;
            v.a = q[0][0] | q[0][1] << 8 | q[0][2] << 16 | q[1][0] << 24;
            v.b = q[1][1] | q[1][2] << 8 | q[2][0] << 16 | q[2][1] << 24;
            v.c = q[2][2] | q[3][0] << 8 | q[3][1] << 16 | q[3][2] << 24;
            *reinterpret_cast<tio_u32x3*>(d) = v;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (in[j]) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[3 * j + c] = (uint8_t)q[j][c];
                }
        }
    }
}

template <typename T>
static void tio_gather(const void* img, int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h, int64_t w,
                       void* out, hipStream_t st) {
    const size_t al = sizeof(T) == 4 ? 16 : 8;
    const bool vec = w % 4 == 0 && reinterpret_cast<uintptr_t>(out) % al == 0;
    const dim3 grid(grid_blocks(h * cdiv(w, 4)), (unsigned)n);
    prof_note((double)n * (double)(h * w) * (3.0 + 3.0 * sizeof(T)), 0.0);
    dispatch_bool(vec, [&](auto VEC) {
        OFASR_LAUNCH((tile_gather_u8_kernel<T, VEC>), grid, dim3(256), 0, st, (const uint8_t*)img, (long long)H, (long long)W,
                     (const long long*)origins, (long long)h, (long long)w, (T*)out);
    });
}

template <typename T>
static void tio_scatter(const void* src, int64_t n, int64_t sh, int64_t sw, const int64_t* table, void* img, int64_t OH,
                        int64_t OW, int64_t max_eh, int64_t max_ew, hipStream_t st) {
    const bool wide = reinterpret_cast<uintptr_t>(img) % 4 == 0;
    const dim3 grid(grid_blocks(max_eh * ((max_ew >> 2) + 2)), (unsigned)n);
    prof_note((double)n * (double)(max_eh * max_ew) * (3.0 + 3.0 * sizeof(T)), 0.0);
    dispatch_bool(wide, [&](auto WIDE) {
        OFASR_LAUNCH((tile_scatter_u8_kernel<T, WIDE>), grid, dim3(256), 0, st, (const T*)src, (long long)sh, (long long)sw,
                     (const long long*)table, (uint8_t*)img, (long long)OH, (long long)OW, (long long)max_eh, (long long)max_ew);
    });
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int ofasr_tile_gather_u8(const void* img, int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h,
                                      int64_t w, void* out, int dtype, void* stream) {
    const char* name = "ofasr_tile_gather_u8";
    OFASR_REQUIRE(img && origins && out, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(H > 0 && W > 0 && n > 0 && h > 0 && w > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE_DTYPE(dtype);
    TILE_REQUIRE_WINDOWS(n, h, w, H, W, "image", "too many windows or too large an image");
    hipStream_t st = as_stream(stream);
    dispatch_float(dtype, [&](auto t) { tio_gather<typename decltype(t)::type>(img, H, W, origins, n, h, w, out, st); });
    return check_launch(name);
}

OFASR_EXPORT int ofasr_tile_scatter_u8(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                                       void* img, int64_t OH, int64_t OW, int64_t max_eh, int64_t max_ew, void* stream) {
    const char* name = "ofasr_tile_scatter_u8";
    OFASR_REQUIRE(src && table && img, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n > 0 && sh > 0 && sw > 0 && OH > 0 && OW > 0 && max_eh > 0 && max_ew > 0, OFASR_ERR_INVALID_ARG,
                  "%s: non-positive size", name);
    OFASR_REQUIRE_DTYPE(dtype);
    OFASR_REQUIRE(max_eh <= sh && max_ew <= sw, OFASR_ERR_INVALID_ARG, "%s: extent bound larger than the source window",
                  name);
    TILE_REQUIRE_COUNT(n, OH, OW, "too many windows or too large an image");
    hipStream_t st = as_stream(stream);
    dispatch_float(dtype, [&](auto t) {
        tio_scatter<typename decltype(t)::type>(src, n, sh, sw, table, img, OH, OW, max_eh, max_ew, st);
    });
    return check_launch(name);
}
