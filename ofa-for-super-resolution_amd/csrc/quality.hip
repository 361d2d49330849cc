// quality.hip -- Y-channel SSE and SSIM of two image batches where they already are, on the GPU (ofasr_quality_y).
//
// Definition (utils.y_exact / utils.ssim_y are the host statement):
//   quantise: a float operand -> uint8 RGB as utils.tensor2img_np / tile_io.hip do (clamp to [0, 1], * 255 in fp32,
//             round half to even); a uint8 operand is taken as it is
//   luma:     Y = round_half_even((65481 R + 128553 G + 24966 B) / 255000 + 16), in integer arithmetic (exact)
//   shave:    that many pixels dropped from every side of both images first
//   sse:      sum (Ya - Yb)^2 over the shaved image, int64, exact
//   ssim:     Wang et al. 2004 on the Y images: 11x11 Gaussian window (sigma 1.5, normalised, separable), "valid"
//             positions only ((h - 10) x (w - 10)), C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, fp64 throughout, mean of
//             the map
//
// Tile scheme.  One workgroup of 256 lanes per (32 x 32 tile of the SSIM map, image).  It reads the 42 x 42 pixels under
// the tile of both operands once, quantises, forms both lumas and keeps them as one 16-bit word per pixel in LDS
// (3.6 KB).  The squared error of the pixels a tile OWNS (its 32 x 32 block; the last tile of a row / column also owns
// the 10 trailing pixels) is taken in that same pass.  Horizontal 11-tap pass: the four quantities G*a, G*b, G*(a^2+b^2),
// G*(ab) of the 42 rows x 32 columns go to LDS as fp64 (43 KB; the products are formed on the fly from the small
// integers, sigma1^2 + sigma2^2 is all the formula needs of the two variances).  Vertical pass: a lane owns 4 vertically
// adjacent positions of one column and walks the 14 rows under them once.  The formula, then a fixed-order reduction:
// shuffles inside a wave, the 4 wave totals added by lane 0, one (sse, ssim_sum) partial per tile in the workspace.
// A second kernel (one workgroup per image) adds the partials in a fixed order and divides.  No atomics anywhere: two
// runs give identical bits.
//
// ofasr_quality_mse is the evaluation loop's LOSS beside the metric: the mean of the fp32 squares of the fp32 differences
// of the raw values (what nn.MSELoss computes per image), accumulated in fp64 in a fixed order, so that a scoring pass
// needs no ATen kernel at all.
//
// Every global read is bounds-checked against the shaved image, offsets are 64-bit.
#include "quality_math.h"   // q_quant, q_luma
#include <math.h>

#pragma clang fp contract(off)   // the formula's groupings are meant as written (identical operands give exactly 1)

namespace ofasr {

constexpr int QT = 32;            // tile side, SSIM positions
constexpr int QW = 11;            // window
constexpr int QH = QT + QW - 1;   // 42: pixels under a tile, per side
constexpr int QP = QH + 2;        // row pitch of the luma image in LDS

struct QGauss { double g[QW]; };

struct QOperand {
    const void* p;
    int fmt;                      // OFASR_F32 / OFASR_F16 / OFASR_BF16: planar NCHW; OFASR_U8_HWC: interleaved, one image
};

// luma of pixel (y, x) of image n of an operand ([N, 3, H, W] planar or [H, W, 3] interleaved)
__device__ __forceinline__ uint32_t q_pixel(const QOperand& o, long long n, long long H, long long W, long long y,
                                            long long x) {
    uint32_t c[3];
    if (o.fmt == OFASR_U8_HWC) {
        const uint8_t* s = reinterpret_cast<const uint8_t*>(o.p) + (y * W + x) * 3;
        c[0] = s[0], c[1] = s[1], c[2] = s[2];
    } else {
        const long long plane = H * W, at = n * 3 * plane + y * W + x;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v;
            if (o.fmt == OFASR_F32) v = reinterpret_cast<const float*>(o.p)[at + k * plane];
            else if (o.fmt == OFASR_BF16) v = to_float(reinterpret_cast<const bf16_t*>(o.p)[at + k * plane]);
            else v = to_float(reinterpret_cast<const f16_t*>(o.p)[at + k * plane]);
            c[k] = q_quant(v);
        }
    }
    return q_luma(c[0], c[1], c[2]);
}

struct alignas(16) QPartial {
    long long sse;
    double ssim;
};

// grid: (tiles_x, tiles_y, N).  h, w: the shaved image.
__global__ void __launch_bounds__(256) quality_y_tile_kernel(QOperand A, QOperand B, long long H, long long W, long long shave,
                                                             long long h, long long w, QGauss G, QPartial* __restrict__ part) {
    __shared__ uint16_t ybuf[QH * QP];
    __shared__ double hbuf[4][QH * QT];
    __shared__ double red_s[4];
    __shared__ unsigned long long red_e[4];
    const int t = (int)threadIdx.x;
    const long long n = blockIdx.z;
    const long long y0 = (long long)blockIdx.y * QT, x0 = (long long)blockIdx.x * QT;
    const bool last_y = blockIdx.y + 1 == gridDim.y, last_x = blockIdx.x + 1 == gridDim.x;

    // ---- load, quantise, luma; squared error of the owned pixels
    unsigned long long sse = 0;
    for (int i = t; i < QH * QH; i += 256) {
        const int r = i / QH, c = i - r * QH;
        const long long y = y0 + r, x = x0 + c;
        uint32_t ya = 0, yb = 0;
        if (y < h && x < w) {
            ya = q_pixel(A, n, H, W, y + shave, x + shave);
            yb = q_pixel(B, n, H, W, y + shave, x + shave);
            if ((r < QT || last_y) && (c < QT || last_x)) {
                const int d = (int)ya - (int)yb;
                sse += (unsigned)(d * d);
            }
        }
        ybuf[r * QP + c] = (uint16_t)(ya | (yb << 8));
    }
    __syncthreads();

    // ---- horizontal pass: rows 0..41, columns 0..31
    for (int i = t; i < QH * QT; i += 256) {
        const int r = i >> 5, c = i & 31;
        double sa = 0.0, sb = 0.0, sq = 0.0, sx = 0.0;
#pragma unroll
        for (int k = 0; k < QW; ++k) {
            const uint32_t v = ybuf[r * QP + c + k];
            const int a = (int)(v & 0xffu), b = (int)(v >> 8);
            sa = fma(G.g[k], (double)a, sa);
            sb = fma(G.g[k], (double)b, sb);
            sq = fma(G.g[k], (double)(a * a + b * b), sq);
            sx = fma(G.g[k], (double)(a * b), sx);
        }
        hbuf[0][i] = sa;
        hbuf[1][i] = sb;
        hbuf[2][i] = sq;
        hbuf[3][i] = sx;
    }
    __syncthreads();

    // ---- vertical pass: lane = (column, group of 4 rows)
    const int c = t & 31, r0 = (t >> 5) * 4;
    double acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[j][q] = 0.0;
#pragma unroll
    for (int r = 0; r < 4 + QW - 1; ++r) {
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = hbuf[q][(r0 + r) * QT + c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = r - j;
            if (k >= 0 && k < QW) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[j][q] = fma(G.g[k], v[q], acc[j][q]);
            }
        }
    }
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double ssim = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (y0 + r0 + j < h - (QW - 1) && x0 + c < w - (QW - 1)) {
            const double m1 = acc[j][0], m2 = acc[j][1];
            const double m12 = m1 * m2, mm = m1 * m1 + m2 * m2;
            const double s12 = acc[j][3] - m12;
            const double num = (2.0 * m12 + C1) * (2.0 * s12 + C2);
            const double den = (mm + C1) * ((acc[j][2] - mm) + C2);
            ssim += num / den;
        }
    }

    // ---- fixed-order reduction
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ssim += __shfl_xor(ssim, o, 64);
        sse += __shfl_xor(sse, o, 64);
    }
    if ((t & 63) == 0) {
        red_s[t >> 6] = ssim;
        red_e[t >> 6] = sse;
    }
    __syncthreads();
    if (t == 0) {
        QPartial p;
        p.ssim = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        p.sse = (long long)(red_e[0] + red_e[1] + red_e[2] + red_e[3]);
        part[(n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = p;
    }
}

// grid: (N).  Lane t adds partials t, t + 256, ... in order; the 256 lane totals are then added pairwise in a fixed tree.
__global__ void __launch_bounds__(256) quality_y_finish_kernel(const QPartial* __restrict__ part, long long tiles,
                                                               double positions, long long* __restrict__ sse,
                                                               double* __restrict__ ssim) {
    __shared__ double rs[256];
    __shared__ long long re[256];
    const int t = (int)threadIdx.x;
    const QPartial* p = part + (long long)blockIdx.x * tiles;
    double s = 0.0;
    long long e = 0;
    for (long long i = t; i < tiles; i += 256) {
        s += p[i].ssim;
        e += p[i].sse;
    }
    rs[t] = s;
    re[t] = e;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            rs[t] += rs[t + o];
            re[t] += re[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        sse[blockIdx.x] = re[0];
        ssim[blockIdx.x] = rs[0] / positions;
    }
}

// ---- mean squared error of the raw (unquantised) values: the evaluation loop's loss beside the metric.
// grid: (P <= 256, N).  Block p of image n adds the fp32 squares of the fp32 differences of elements p*256+t, (p+P)*256+t, ...
// in fp64; lanes, then waves, are folded in a fixed order into partial[n * P + p].
template <typename TA, typename TB>
__global__ void __launch_bounds__(256) quality_mse_part_kernel(const TA* __restrict__ a, const TB* __restrict__ b,
                                                               long long elems, double* __restrict__ part) {
    __shared__ double red[4];
    const int t = (int)threadIdx.x;
    const long long base = (long long)blockIdx.y * elems;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + t; i < elems; i += (long long)gridDim.x * 256) {
        const float d = __fsub_rn(to_float(a[base + i]), to_float(b[base + i]));
        s += (double)__fmul_rn(d, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// grid: (N); mse[n] = (sum of the P partials, pairwise in a fixed tree) / elems
__global__ void __launch_bounds__(256) quality_mse_finish_kernel(const double* __restrict__ part, int P, double elems,
                                                                 double* __restrict__ mse) {
    __shared__ double rs[256];
    const int t = (int)threadIdx.x;
    rs[t] = t < P ? part[(long long)blockIdx.x * P + t] : 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) rs[t] += rs[t + o];
        __syncthreads();
    }
    if (t == 0) mse[blockIdx.x] = rs[0] / elems;
}

static int q_mse_parts(int64_t elems) {
    const int64_t p = cdiv(elems, 256 * 16);
    return (int)(p < 1 ? 1 : (p > 256 ? 256 : p));
}

template <typename TA, typename TB>
static void q_mse_launch(const void* a, const void* b, int64_t N, int64_t elems, double* mse, double* part, hipStream_t st) {
    const int P = q_mse_parts(elems);
    OFASR_LAUNCH((quality_mse_part_kernel<TA, TB>), dim3((unsigned)P, (unsigned)N), dim3(256), 0, st, (const TA*)a,
                 (const TB*)b, (long long)elems, part);
    OFASR_LAUNCH(quality_mse_finish_kernel, dim3((unsigned)N), dim3(256), 0, st, (const double*)part, P, (double)elems, mse);
}
template <typename TA>
static void q_mse_b(const void* a, const void* b, int fmt_b, int64_t N, int64_t elems, double* mse, double* part,
                    hipStream_t st) {
    dispatch_float(fmt_b, [&](auto tb) { q_mse_launch<TA, typename decltype(tb)::type>(a, b, N, elems, mse, part, st); });
}

static bool q_fmt_ok(int f) { return is_float_dtype(f) || f == OFASR_U8_HWC; }
static double q_fmt_bytes(int f) { return f == OFASR_U8_HWC ? 1.0 : (double)elem_bytes(f); }

// 0 unless the shape is one ofasr_quality_y accepts
static int64_t q_tiles(int64_t N, int64_t H, int64_t W, int64_t shave, int64_t* ty, int64_t* tx) {
    if (N <= 0 || H <= 0 || W <= 0 || shave < 0 || shave > (1LL << 30)) return 0;
    const int64_t h = H - 2 * shave, w = W - 2 * shave;
    if (h < QW || w < QW) return 0;
    *ty = cdiv(h - (QW - 1), QT);
    *tx = cdiv(w - (QW - 1), QT);
    return *ty * *tx;
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT size_t ofasr_quality_y_workspace(int64_t N, int64_t H, int64_t W, int64_t shave) {
    int64_t ty = 0, tx = 0;
    const int64_t tiles = q_tiles(N, H, W, shave, &ty, &tx);
    return tiles > 0 ? (size_t)(tiles * N) * sizeof(QPartial) : 0;
}

OFASR_EXPORT int ofasr_quality_y(const void* a, int fmt_a, const void* b, int fmt_b, int64_t N, int64_t H, int64_t W,
                                 int64_t shave, int64_t* sse, double* ssim, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    const char* name = "ofasr_quality_y";
    OFASR_REQUIRE(a && b && sse && ssim, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(q_fmt_ok(fmt_a) && q_fmt_ok(fmt_b), OFASR_ERR_INVALID_ARG, "%s: unknown format %d / %d", name, fmt_a,
                  fmt_b);
    OFASR_REQUIRE(N > 0 && H > 0 && W > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(shave >= 0, OFASR_ERR_INVALID_ARG, "%s: negative shave %lld", name, (long long)shave);
    OFASR_REQUIRE(shave <= (1LL << 30) && H - 2 * shave >= QW && W - 2 * shave >= QW, OFASR_ERR_INVALID_ARG,
                  "%s: a %lldx%lld image shaved by %lld has a side below the %d-pixel SSIM window", name, (long long)H,
                  (long long)W, (long long)shave, QW);
    OFASR_REQUIRE((fmt_a != OFASR_U8_HWC && fmt_b != OFASR_U8_HWC) || N == 1, OFASR_ERR_INVALID_ARG,
                  "%s: an interleaved uint8 operand is one image (N = %lld)", name, (long long)N);
    int64_t ty = 0, tx = 0;
    const int64_t tiles = q_tiles(N, H, W, shave, &ty, &tx);
    OFASR_REQUIRE(N <= 65535 && ty <= 65535 && H <= (1LL << 40) / W, OFASR_ERR_UNSUPPORTED,
                  "%s: too many images or too large an image", name);
    const size_t need = (size_t)(tiles * N) * sizeof(QPartial);
    OFASR_REQUIRE(workspace && workspace_bytes >= need && aligned16(workspace),
                  OFASR_ERR_WORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", name, need,
                  workspace_bytes);
    QGauss G;
    double sum = 0.0;
    for (int k = 0; k < QW; ++k) sum += (G.g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5)));
    for (int k = 0; k < QW; ++k) G.g[k] /= sum;
    const long long h = H - 2 * shave, w = W - 2 * shave;
    hipStream_t st = as_stream(stream);
    prof_note((double)N * (double)H * (double)W * 3.0 * (q_fmt_bytes(fmt_a) + q_fmt_bytes(fmt_b)), 0.0);
    OFASR_LAUNCH(quality_y_tile_kernel, dim3((unsigned)tx, (unsigned)ty, (unsigned)N), dim3(256), 0, st, QOperand{a, fmt_a},
                 QOperand{b, fmt_b}, (long long)H, (long long)W, (long long)shave, h, w, G, (QPartial*)workspace);
    OFASR_LAUNCH(quality_y_finish_kernel, dim3((unsigned)N), dim3(256), 0, st, (const QPartial*)workspace, (long long)tiles,
                 (double)(h - (QW - 1)) * (double)(w - (QW - 1)), (long long*)sse, (double*)ssim);
    return check_launch(name);
}

OFASR_EXPORT size_t ofasr_quality_mse_workspace(int64_t N, int64_t elems) {
    if (N <= 0 || elems <= 0) return 0;
    return (size_t)N * (size_t)q_mse_parts(elems) * sizeof(double);
}

OFASR_EXPORT int ofasr_quality_mse(const void* a, int fmt_a, const void* b, int fmt_b, int64_t N, int64_t elems, double* mse,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "ofasr_quality_mse";
    OFASR_REQUIRE(a && b && mse, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(q_fmt_ok(fmt_a) && q_fmt_ok(fmt_b) && fmt_a != OFASR_U8_HWC && fmt_b != OFASR_U8_HWC, OFASR_ERR_INVALID_ARG,
                  "%s: operands are f32 / f16 / bf16 (formats %d / %d)", name, fmt_a, fmt_b);
    OFASR_REQUIRE(N > 0 && elems > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(N <= 65535 && elems <= (1LL << 40), OFASR_ERR_UNSUPPORTED, "%s: too many or too large images", name);
    const size_t need = ofasr_quality_mse_workspace(N, elems);
    OFASR_REQUIRE(workspace && workspace_bytes >= need && reinterpret_cast<uintptr_t>(workspace) % 8 == 0,
                  OFASR_ERR_WORKSPACE, "%s: workspace of %zu bytes (8-byte aligned) needed, %zu given", name, need,
                  workspace_bytes);
    hipStream_t st = as_stream(stream);
    const double eb = q_fmt_bytes(fmt_a) + q_fmt_bytes(fmt_b);
    prof_note((double)N * (double)elems * eb, 0.0);
    dispatch_float(fmt_a, [&](auto ta) { q_mse_b<typename decltype(ta)::type>(a, b, fmt_b, N, elems, mse, (double*)workspace, st); });
    return check_launch(name);
}
