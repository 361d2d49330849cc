// mode_io.hip -- alpha and greyscale around the RGB image path (ofasr_mode_unpack_u8 / ofasr_mode_pack_u8): an L, LA or RGBA
// image is split into the 3-byte RGB image that gather, routing and window_activity read plus its alpha plane, and the
// RGB output of the network is joined with the alpha plane, resampled to the output's size, into an image of the input's
// mode.  Host definition: modes.py (split_host, alpha_host = resize.resize_host of the SOURCE alpha, luma_host = Pillow's
// convert("L"), join_host).  Integers only; both kernels are bit-exact against it.
//
// unpack: one pass, a lane owns four consecutive pixels.  Where the three pointers are 4-byte aligned it loads C dwords and
// stores three dwords of RGB and one of alpha; elsewhere, and for the last pixels of the image, bytes.
//
// pack: one workgroup (256 threads) owns an MP_TY x MP_TX = 16 x 64 tile of the target, the tile and the two passes of
// tile_resize_scatter_kernel (resize_scatter.hip) on one plane:
//   1. horizontal pass of the alpha source rows the tile needs into LDS.  The kernel only enlarges (at most MP_TAPS = 7 taps
//      per axis: lanczos enlarging), so the tile's 16 target rows read at most MP_ROWS = 24 source rows (modes.alpha_tables
//      asserts both).  (acc + 2^21) >> 22, clipped, is Pillow's 8-bit intermediate image and is what the LDS holds.
//      Consecutive lanes own consecutive columns of one row: their byte stores fall into 16 consecutive LDS dwords, four
//      lanes to a dword, 16 banks, no conflict.
//   2. vertical pass from LDS: a wave owns one target row at a time (its table row is wave-uniform), a lane one pixel; the
//      lane reads its three RGB bytes, forms the luma for L / LA, and leaves the pixel's C bytes in an LDS image of the
//      tile's output.
//   3. the store: every target row of the tile is a contiguous run of nc * C bytes; the workgroup walks the ALIGNED dwords
//      that cover it, consecutive lanes consecutive dwords.  A dword that lies inside the run is one 4-byte store (RGBA at
//      an aligned `out`: one pixel), the at most two ragged dwords of a run go out as bytes: no store covers a byte outside
//      the run, whatever the alignment of `out` and the parity of TW.
// C = 1 has no alpha: steps 1 and the vertical sums are compiled out, the tables are not read.
// LDS: 1.5 KiB (intermediate) + 16 * 64 * C bytes (output tile) <= 5.5 KiB.  No scratch.
//
// Addressing is 64-bit.  Every access stays inside its tensor whatever the device tables hold, by resize_scatter's rule:
// counts are clamped to kh / kw, every source index into the alpha plane, every LDS row into the tile's span, and loads
// sit inside the branch that bounds them.  A wrong table gives wrong values, never a fault.  The accumulators are
// unsigned, so a wild coefficient wraps instead of overflowing.
#include "tile_table.h"

namespace ofasr {

constexpr int MP_TY = 16, MP_TX = 64, MP_ROWS = 24, MP_TAPS = 7, MP_BITS = 22;
constexpr int MP_SLOTS = MP_TX + 1;      // aligned dwords that can cover one row of a tile: (3 + 64 * 4 + 3) / 4

__device__ __forceinline__ uint32_t mp_clip8(uint32_t acc) {
    const int v = (int)acc >> MP_BITS;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
// Pillow's convert("L") of an RGB pixel (ImagingConvert rgb2l: L24 >> 16)
__device__ __forceinline__ uint32_t mp_luma(uint32_t r, uint32_t g, uint32_t b) {
    return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
}

// grid: ceil(HW / 1024) blocks of 256 lanes, four pixels a lane
template <int C>
__global__ void __launch_bounds__(256) mode_unpack_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ rgb,
                                                          uint8_t* __restrict__ alpha, long long HW, int vec) {
    const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p0 >= HW) return;
    if (vec && p0 + 4 <= HW) {
        uint32_t w[C];
#pragma unroll
        for (int i = 0; i < C; ++i) w[i] = reinterpret_cast<const uint32_t*>(img + p0 * C)[i];
        uint32_t o[3] = {0u, 0u, 0u}, a = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int b = C == 4 ? i * 4 + c : i * C;                   // L / LA: R = G = B = L
                const uint32_t v = (w[b >> 2] >> (8 * (b & 3))) & 0xffu;
                o[(i * 3 + c) >> 2] |= v << (8 * ((i * 3 + c) & 3));
            }
            if (C != 1) {
                const int b = i * C + C - 1;
                a |= ((w[b >> 2] >> (8 * (b & 3))) & 0xffu) << (8 * i);
            }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) reinterpret_cast<uint32_t*>(rgb + p0 * 3)[i] = o[i];
        if (C != 1) *reinterpret_cast<uint32_t*>(alpha + p0) = a;
    } else {
        const int n = (int)(HW - p0 < 4 ? HW - p0 : 4);
        for (int i = 0; i < n; ++i) {
            const uint8_t* s = img + (p0 + i) * C;
            uint8_t* d = rgb + (p0 + i) * 3;
            d[0] = s[0];
            d[1] = C == 4 ? s[1] : s[0];
            d[2] = C == 4 ? s[2] : s[0];
            if (C != 1) alpha[p0 + i] = s[C - 1];
        }
    }
}

// grid: ceil(TH / 16) * ceil(TW / 64) tiles
template <int C>
__global__ void __launch_bounds__(256) mode_pack_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ alpha,
                                                        const int* __restrict__ vtab, int kh, const int* __restrict__ htab, int kw,
                                                        uint8_t* __restrict__ out, long long H, long long W, long long TH,
                                                        long long TW) {
    __shared__ uint8_t mid[C == 1 ? 4 : MP_ROWS * MP_TX];
    __shared__ __attribute__((aligned(4))) uint8_t stage[MP_TY * MP_TX * C];
    const long long tiles_x = (TW + MP_TX - 1) / MP_TX;
    const long long ty = (long long)blockIdx.x / tiles_x, tx = (long long)blockIdx.x - ty * tiles_x;
    const long long r0 = ty * MP_TY, c0 = tx * MP_TX;
    if (r0 >= TH || c0 >= TW) return;                          // the same for the whole workgroup: no barrier is skipped
    const int nr = (int)(TH - r0 < MP_TY ? TH - r0 : MP_TY), nc = (int)(TW - c0 < MP_TX ? TW - c0 : MP_TX);
    const int vs = 2 + kh, hs = 2 + kw;
    const int* vt = nullptr;
    int ylo = 0, span = 1;
    // 256 = 4 * MP_TX: a lane keeps its column through every loop below and a wave its row, which is wave-uniform
    const int col = threadIdx.x % MP_TX, wrow = __builtin_amdgcn_readfirstlane(threadIdx.x / MP_TX);
    constexpr int WAVES = 256 / MP_TX;

    // 1. horizontal pass of the alpha plane: mid[row][col] for row < span, col < nc
    if constexpr (C != 1) {
        vt = vtab + r0 * vs;                                   // rows r0 .. r0 + nr - 1 < TH
        const int* ht = htab + c0 * hs;
        // the source rows of the tile: from the first row's first tap to the last row's last
        ylo = clampi((long long)vt[0], 0, H - 1);
        const int* vl = vt + (long long)(nr - 1) * vs;
        const long long yhi = (long long)vl[0] + clampi(vl[1], 0, kh);
        span = clampi(yhi - ylo, 1, MP_ROWS);
        span = span > H - ylo ? (int)(H - ylo) : span;
        const uint8_t* sn = alpha + (long long)ylo * W;
        if (col < nc) {
            // the column's taps once, in registers, for every source row of the tile
            const int* h = ht + (long long)col * hs;
            const int cnt = clampi(h[1], 0, kw);
            const long long x0 = (long long)h[0];
            uint32_t kc[MP_TAPS];
            int xl[MP_TAPS];
#pragma unroll
            for (int k = 0; k < MP_TAPS; ++k) {
                kc[k] = 0u;
                if (k < cnt) kc[k] = (uint32_t)h[2 + k];
                xl[k] = clampi(x0 + k, 0, W - 1);
            }
            for (int row = wrow; row < span; row += WAVES) {
                const uint8_t* s = sn + (long long)row * W;
                uint32_t acc = 1u << (MP_BITS - 1);
#pragma unroll
                for (int k = 0; k < MP_TAPS; ++k)
                    if (k < cnt) acc += (uint32_t)s[xl[k]] * kc[k];
                mid[row * MP_TX + col] = (uint8_t)mp_clip8(acc);
            }
        }
        __syncthreads();
    }

    // 2. vertical pass, the pixel's RGB, the luma: the tile's output bytes into LDS
    for (int r = wrow; r < nr; r += WAVES) {
        if (col < nc) {
            uint32_t a = 0u;
            if constexpr (C != 1) {
                const int* vrow = vt + (long long)r * vs;
                const int cnt = clampi(vrow[1], 0, kh);
                const long long y0 = (long long)vrow[0] - ylo;   // first tap's row inside the tile's span
                uint32_t acc = 1u << (MP_BITS - 1);
                for (int k = 0; k < cnt; ++k) {
                    const int yl = clampi(y0 + k, 0, span - 1);
                    acc += (uint32_t)mid[yl * MP_TX + col] * (uint32_t)vrow[2 + k];
                }
                a = mp_clip8(acc);
            }
            const uint8_t* p = rgb + ((r0 + r) * TW + c0 + col) * 3;
            const uint32_t R = p[0], G = p[1], B = p[2];
            if constexpr (C == 4) {
                reinterpret_cast<uint32_t*>(stage)[r * MP_TX + col] = R | (G << 8) | (B << 16) | (a << 24);
            } else if constexpr (C == 2) {
                reinterpret_cast<uint16_t*>(stage)[r * MP_TX + col] = (uint16_t)(mp_luma(R, G, B) | (a << 8));
            } else {
                stage[r * MP_TX + col] = (uint8_t)mp_luma(R, G, B);
            }
        }
    }
    __syncthreads();

    // 3. the store: per target row the aligned dwords that cover its run of nc * C bytes
    const int run = nc * C;
    for (int e = threadIdx.x; e < nr * MP_SLOTS; e += 256) {
        const int r = e / MP_SLOTS, j = e % MP_SLOTS;
        uint8_t* d = out + ((r0 + r) * TW + c0) * C;
        const int mis = (int)(reinterpret_cast<uintptr_t>(d) & 3);
        const int b0 = j * 4 - mis;                            // the dword's first byte, relative to the run
        if (b0 < run) {
            const uint8_t* s = stage + r * MP_TX * C;
            if (b0 >= 0 && b0 + 4 <= run) {
                uint32_t w;
                if (mis == 0) w = *reinterpret_cast<const uint32_t*>(s + b0);
                else w = (uint32_t)s[b0] | ((uint32_t)s[b0 + 1] << 8) | ((uint32_t)s[b0 + 2] << 16) | ((uint32_t)s[b0 + 3] << 24);
                *reinterpret_cast<uint32_t*>(d + b0) = w;
            } else {
                for (int k = 0; k < 4; ++k) {
                    const int b = b0 + k;
                    if (b >= 0 && b < run) d[b] = s[b];
                }
            }
        }
    }
}

template <int C>
static void unpack_launch(const void* img, void* rgb, void* alpha, int64_t HW, hipStream_t st) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(alpha);
    prof_note((double)HW * (C + 3 + (C != 1)), 0.0);
    OFASR_LAUNCH((mode_unpack_kernel<C>), dim3((unsigned)cdiv(HW, 1024)), dim3(256), 0, st, (const uint8_t*)img, (uint8_t*)rgb,
                 (uint8_t*)alpha, (long long)HW, (int)((bits & 3) == 0));
}

template <int C>
static void pack_launch(const void* rgb, const void* alpha, const int32_t* vtab, int kh, const int32_t* htab, int kw, void* out,
                        int64_t H, int64_t W, int64_t TH, int64_t TW, hipStream_t st) {
    prof_note((double)(TH * TW) * (3 + C) + (C != 1 ? (double)(H * W) : 0.0), 0.0);
    OFASR_LAUNCH((mode_pack_kernel<C>), dim3((unsigned)(cdiv(TH, MP_TY) * cdiv(TW, MP_TX))), dim3(256), 0, st, (const uint8_t*)rgb,
                 (const uint8_t*)alpha, (const int*)vtab, kh, (const int*)htab, kw, (uint8_t*)out, (long long)H, (long long)W,
                 (long long)TH, (long long)TW);
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int ofasr_mode_unpack_u8(const void* img, int C, void* rgb, void* alpha, int64_t H, int64_t W, void* stream) {
    const char* name = "ofasr_mode_unpack_u8";
    OFASR_REQUIRE(C == 1 || C == 2 || C == 4, OFASR_ERR_INVALID_ARG, "%s: %d channels; 1 (L), 2 (LA) or 4 (RGBA)", name, C);
    OFASR_REQUIRE(img && rgb && (alpha || C == 1), OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(!(alpha && C == 1), OFASR_ERR_INVALID_ARG, "%s: an L image has no alpha plane to write", name);
    OFASR_REQUIRE(H > 0 && W > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(H <= (1LL << 40) / W, OFASR_ERR_UNSUPPORTED, "%s: too large an image", name);
    hipStream_t st = as_stream(stream);
    if (C == 1) unpack_launch<1>(img, rgb, alpha, H * W, st);
    else if (C == 2) unpack_launch<2>(img, rgb, alpha, H * W, st);
    else unpack_launch<4>(img, rgb, alpha, H * W, st);
    return check_launch(name);
}

OFASR_EXPORT int ofasr_mode_pack_u8(const void* rgb, const void* alpha_src, const int32_t* vtab, int kh, const int32_t* htab, int kw,
                                    void* out, int C, int64_t H, int64_t W, int64_t TH, int64_t TW, void* stream) {
    const char* name = "ofasr_mode_pack_u8";
    OFASR_REQUIRE(C == 1 || C == 2 || C == 4, OFASR_ERR_INVALID_ARG, "%s: %d channels; 1 (L), 2 (LA) or 4 (RGBA)", name, C);
    OFASR_REQUIRE(rgb && out && (C == 1 || (alpha_src && vtab && htab)), OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(H > 0 && W > 0 && TH > 0 && TW > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    if (C != 1) {
        OFASR_REQUIRE(kh >= 1 && kw >= 1 && kh <= MP_TAPS && kw <= MP_TAPS, OFASR_ERR_UNSUPPORTED,
                      "%s: %d x %d taps; 1 to %d per axis (this kernel enlarges only: lanczos enlarging has %d)", name, kh, kw,
                      MP_TAPS, MP_TAPS);
        OFASR_REQUIRE(TH >= H && TW >= W, OFASR_ERR_UNSUPPORTED, "%s: a %lldx%lld target of a %lldx%lld alpha plane; this kernel enlarges only",
                      name, (long long)TW, (long long)TH, (long long)W, (long long)H);
    }
    OFASR_REQUIRE(TH <= (1LL << 40) / TW && H <= (1LL << 40) / W && cdiv(TH, MP_TY) * cdiv(TW, MP_TX) <= 0x7fffffffLL,
                  OFASR_ERR_UNSUPPORTED, "%s: too large an image", name);
    hipStream_t st = as_stream(stream);
    if (C == 1) pack_launch<1>(rgb, nullptr, nullptr, 1, nullptr, 1, out, H, W, TH, TW, st);
    else if (C == 2) pack_launch<2>(rgb, alpha_src, vtab, kh, htab, kw, out, H, W, TH, TW, st);
    else pack_launch<4>(rgb, alpha_src, vtab, kh, htab, kw, out, H, W, TH, TW, st);
    return check_launch(name);
}
