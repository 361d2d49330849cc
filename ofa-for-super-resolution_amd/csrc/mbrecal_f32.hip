// mbrecal_f32.hip -- BatchNorm re-calibration of the MB block at fp32 (ofasr_mbconv_recal_f32_*), and the statistics fold
// of the static convs' re-calibration (ofasr_bn_recal_accumulate).
//
// Re-calibration is train-mode BatchNorm forward with no backward: every BN of
//     out = x + BN3(W2 . relu6(BN2(dw_k(relu6(BN1(W1 . x))))))
// normalises with the mean and biased variance of the current batch, and those are added, weighted by the batch size,
// into caller-owned fp64 accumulators.  Running statistics and num_batches_tracked are neither read nor written.  The
// block keeps the structure of mbfused_f32.hip (one workgroup = one 16 x 16 output tile of one image, x straight from
// global memory into the fp32 MFMA fragments through buffer loads bounded by the image, the mid tensor in LDS only) and
// recomputes instead of storing y1 / y2:
//   S1  y1 = W1 . x over the tile's in-image pixels (no halo)                  -> per-workgroup (mean, M2) of y1
//   F1  fixed-order Chan merge of the partials -> batch mean1 / var1, accumulators, BN1 folded into the expand operands
//   S2  expand (BN1 folded), ReLU6 on the halo window, raw depthwise          -> per-workgroup (mean, M2) of y2
//   F2  the same for BN2, folded into the taps and the depthwise bias
//   S3  the whole block with BN1 / BN2 folded, project raw                    -> y3 (64 ch) + per-workgroup (mean, M2)
//   F3  the same for BN3 -> scale3 / shift3;  apply: out = y3 . scale3 + shift3 (+ x)  (ofasr_bn_act_fwd)
// Per-workgroup statistics are (mean, sum of squared deviations) of fp32 values taken in two passes over registers, so
// they do not cancel; the merge runs in fp64 in a fixed order (no float atomics: two runs are bit-identical).
// Everything is queued on the caller's stream, with no host round trip.  Roofline numbers: DESIGN.md section 3.1b.
#include "ofasr_common.h"

namespace ofasr {

typedef __attribute__((ext_vector_type(16))) float r32x16;
typedef __attribute__((ext_vector_type(2))) float r32x2;

constexpr int MR_THREADS = 512;
constexpr int MR_MC = 32;          // mid channels per chunk
constexpr int MR_A2P = 288;        // pixel pitch of the a2 planes (as mbfused_f32.hip)
constexpr int MR_TILE = 16;        // output tile 16 x 16
constexpr int MR_MERGE_THREADS = 256;

template <int K> struct MrGeom {
    static constexpr int P = K / 2;
    static constexpr int WC = MR_TILE + 2 * P;
    static constexpr int NPIX = WC * WC;
    static constexpr int NBLK = (NPIX + 31) / 32;
    static constexpr int NBW = (NBLK + 7) / 8;
    static constexpr int A1P = NBLK * 32 + 4;
    static constexpr int TAPROW = (K * K + 1 + 3) / 4 * 4;
};

__device__ __forceinline__ int mr_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ r32x16 mr_mma(float a, float b, r32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t mr_rsrc(const float* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, bytes, 0x00020000);
}
__device__ __forceinline__ float mr_load(__amdgpu_buffer_rsrc_t r, int off_bytes) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, off_bytes, 0, 0));
}

__device__ __forceinline__ float mr_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Chan et al. merge of (n, mean, M2) triples; an empty side leaves the other unchanged
template <typename T> __device__ __forceinline__ void mr_chan(T& n, T& m, T& m2, T nb, T mb, T m2b) {
    if (nb <= T(0)) return;
    if (n <= T(0)) {
        n = nb; m = mb; m2 = m2b;
        return;
    }
    const T t = n + nb, d = mb - m;
    m += d * (nb / t);
    m2 += m2b + d * d * (n * nb / t);
    n = t;
}

// ---- operand images: BN i folded when fold[i], identity otherwise -----------------------------------------------
struct MrFold {
    const float* w1; long long ldw1;
    const float* w2; long long ldw2;
    const float* f;                      // active depthwise filter [mid][K][K]
    const float* gamma[3]; const float* beta[3]; const float* mean[3]; const float* var[3];
    float eps[3];
    int fold[3];
    int mid, K;
};

__global__ void __launch_bounds__(256) mr_fold_kernel(MrFold p, float* __restrict__ w1f, float* __restrict__ b1,
                                                      float* __restrict__ taps, float* __restrict__ w2f,
                                                      float* __restrict__ b3) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int nth = gridDim.x * blockDim.x;
    const int mid = p.mid, K = p.K, TAPROW = (K * K + 1 + 3) / 4 * 4;
    auto scale = [&](int i, int c) { return p.fold[i] ? p.gamma[i][c] / sqrtf(p.var[i][c] + p.eps[i]) : 1.f; };
    auto shift = [&](int i, int c) { return p.fold[i] ? p.beta[i][c] - p.mean[i][c] * scale(i, c) : 0.f; };
    // fragment order of mbfused_f32.hip's mg_fold_kernel
    for (int e = tid; e < mid * 64; e += nth) {
        const int l = e & 63, s = (e >> 6) & 31, ci = e >> 11;
        const int c = 32 * ci + (l & 31), k = 2 * s + (l >> 5);
        w1f[e] = p.w1[(long long)c * p.ldw1 + k] * scale(0, c);
    }
    for (int e = tid; e < 64 * mid; e += nth) {
        const int l = e & 63, s = (e >> 6) & 15, ob = (e >> 10) & 1, ci = e >> 11;
        const int o = 32 * ob + (l & 31), c = 32 * ci + 2 * s + (l >> 5);
        w2f[e] = p.w2[(long long)o * p.ldw2 + c] * scale(2, o);
    }
    for (int c = tid; c < mid; c += nth) {
        b1[c] = shift(0, c);
        float* row = taps + (long long)c * TAPROW;
        const float s2 = scale(1, c);
        for (int t = 0; t < K * K; ++t) row[t] = p.f[(long long)c * K * K + t] * s2;
        row[K * K] = shift(1, c);
        for (int t = K * K + 1; t < TAPROW; ++t) row[t] = 0.f;
    }
    for (int o = tid; o < 64; o += nth) b3[o] = shift(2, o);
}

// ---- the finalize shared by the MB block's F passes and ofasr_bn_recal_accumulate --------------------------------
// acc[c] += weight * mean, acc[C + c] += weight * var (one writer per channel); optional float outputs
struct MrOut {
    double* acc;
    double weight;
    float* mean;
    float* var;
    float* invstd;
    float* scale;
    float* shift;
    const float* gamma;
    const float* beta;
    double eps;
};

__device__ __forceinline__ void mr_finalize(const MrOut& o, int C, int c, double mean, double var) {
    if (var < 0.0) var = 0.0;
    o.acc[c] += o.weight * mean;
    o.acc[C + c] += o.weight * var;
    if (o.mean) o.mean[c] = (float)mean;
    if (o.var) o.var[c] = (float)var;
    const double invstd = 1.0 / sqrt(var + o.eps);
    if (o.invstd) o.invstd[c] = (float)invstd;
    if (o.scale) {
        const double g = o.gamma ? (double)o.gamma[c] : 1.0, b = o.beta ? (double)o.beta[c] : 0.0;
        o.scale[c] = (float)(g * invstd);
        o.shift[c] = (float)(b - mean * g * invstd);
    }
}

// F pass: one workgroup per channel; thread t merges the tiles t, t + 256, ... in order, then a fixed LDS tree.
// A tile's count is its in-image pixel count, recomputed from the geometry.
__global__ void __launch_bounds__(MR_MERGE_THREADS) mr_merge_kernel(const float2* __restrict__ part, int P, int C,
                                                                    int H, int W, int tiles_x, int tiles_y, MrOut o) {
    __shared__ double sn[MR_MERGE_THREADS], sm[MR_MERGE_THREADS], s2[MR_MERGE_THREADS];
    const int c = blockIdx.x, t = threadIdx.x;
    double n = 0.0, m = 0.0, m2 = 0.0;
    for (int p = t; p < P; p += MR_MERGE_THREADS) {
        const int tile = p % (tiles_x * tiles_y);
        const int tx = tile % tiles_x, ty = tile / tiles_x;
        const int rows = min(MR_TILE, H - ty * MR_TILE), cols = min(MR_TILE, W - tx * MR_TILE);
        const float2 v = part[(long long)p * C + c];
        mr_chan(n, m, m2, (double)(rows * cols), (double)v.x, (double)v.y);
    }
    sn[t] = n; sm[t] = m; s2[t] = m2;
    __syncthreads();
    for (int w = MR_MERGE_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            double a = sn[t], b = sm[t], q = s2[t];
            mr_chan(a, b, q, sn[t + w], sm[t + w], s2[t + w]);
            sn[t] = a; sm[t] = b; s2[t] = q;
        }
        __syncthreads();
    }
    if (t == 0) mr_finalize(o, C, c, sm[0], sn[0] > 0.0 ? s2[0] / sn[0] : 0.0);
}

// ---- the statistics passes -----------------------------------------------------------------------------------------
// PASS 1: S1, PASS 2: S2, PASS 3: S3 (module comment).  part: [blocks][C] float2 (tile mean, tile M2) with C = mid for
// S1 / S2 and 64 for S3; y3: [N][64][H][W] (S3 only).
template <int K, int PASS>
__global__ void __launch_bounds__(MR_THREADS) mb_recal_f32_kernel(const float* __restrict__ x, float* __restrict__ y3,
                                                                  float2* __restrict__ part,
                                                                  const float* __restrict__ w1f,
                                                                  const float* __restrict__ b1,
                                                                  const float* __restrict__ taps,
                                                                  const float* __restrict__ w2f, int mid, int H, int W,
                                                                  int tiles_x, int tiles_y) {
    using G = MrGeom<K>;
    // S1 computes the tile's own 16 x 16 pixels: 8 blocks of 32, one per wave
    constexpr int P = PASS == 1 ? 0 : G::P;
    constexpr int WC = PASS == 1 ? MR_TILE : G::WC;
    constexpr int NPIX = WC * WC;
    constexpr int NBLK = (NPIX + 31) / 32;
    constexpr int NBW = (NBLK + 7) / 8;
    constexpr int A1P = NBLK * 32 + 4;
    constexpr int TAPROW = G::TAPROW;
    constexpr int A1N = PASS == 1 ? 4 : MR_MC * A1P;
    constexpr int A2N = PASS == 3 ? MR_MC * MR_A2P : 4;
    __shared__ __attribute__((aligned(16))) float A1[A1N];
    __shared__ __attribute__((aligned(16))) float A2[A2N];
    __shared__ float2 red[2][8][64];     // per-wave (mean, M2), double-buffered by chunk
    __shared__ float wn[8];              // per-wave in-image pixel counts (S1, S3)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    const int blk = blockIdx.x;
    int b = blk;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    const int n = b / tiles_y;
    const int h0 = ty * MR_TILE, w0 = tx * MR_TILE;
    const int plane = H * W;                        // 64 * plane * 4 < 2^31 (mr_supported)
    const int img_bytes = 64 * plane * 4;
    const float* xn = x + (long long)n * 64 * plane;
    const __amdgpu_buffer_rsrc_t xr = mr_rsrc(xn, img_bytes);

    float xf[NBW][32];
    uint32_t mk[NBW];
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        const int pb = wave + 8 * j;
        const int px = 32 * pb + r32;
        const int hh = px / WC, ww = px - hh * WC;
        const int gh = h0 - P + hh, gw = w0 - P + ww;
        const bool ok = pb < NBLK && px < NPIX && gh >= 0 && gh < H && gw >= 0 && gw < W;
        const int pof = ok ? (gh * W + gw) * 4 : img_bytes;
#pragma unroll
        for (int s = 0; s < 32; ++s) {
            const int c = 2 * s + h;
            xf[j][s] = mr_load(xr, ok ? pof + c * plane * 4 : img_bytes);
        }
        uint32_t m = 0u;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int q = 32 * pb + mr_acc_row(reg, h);
            const int qh = q / WC, qw = q - qh * WC;
            const int qgh = h0 - P + qh, qgw = w0 - P + qw;
            if (q < NPIX && qgh >= 0 && qgh < H && qgw >= 0 && qgw < W) m |= 1u << reg;
        }
        mk[j] = m;
    }
    const int tile_rows = min(MR_TILE, H - h0), tile_cols = min(MR_TILE, W - w0);
    const float tile_n = (float)(tile_rows * tile_cols);
    if (PASS != 2 && lane == 0) {
        // S1: the wave's block of 32 tile pixels; S3: the same pixels of the project's output
        const int r0 = 2 * wave;
        wn[wave] = (float)((min(r0 + 2, tile_rows) - min(r0, tile_rows)) * tile_cols);
    }

    const int nchunk = mid / MR_MC;
    float w1c[32];
    float b1c = 0.f;
    auto load_w1 = [&](int ci) {
#pragma unroll
        for (int s = 0; s < 32; ++s) w1c[s] = w1f[(ci * 32 + s) * 64 + lane];
        b1c = b1[ci * MR_MC + r32];
    };

    // (mean, M2) of the 16 masked accumulator values of this lane and its partner lane ^ 32 (same column)
    auto col_stats = [&](const r32x16& acc, uint32_t m, float cnt, float& mean, float& m2) {
        float s = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) s += (m >> reg) & 1u ? acc[reg] : 0.f;
        s += __shfl_xor(s, 32, 64);
        mean = cnt > 0.f ? s / cnt : 0.f;
        float q = 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float d = acc[reg] - mean;
            q += (m >> reg) & 1u ? d * d : 0.f;
        }
        m2 = q + __shfl_xor(q, 32, 64);
    };
    // merge the 8 waves' (mean, M2) of `nc` channels in wave order -> part[blk][c0 + t]
    auto wave_merge = [&](int buf, int nc, int C, int c0) {
        if (tid < nc) {
            float cn = 0.f, cm = 0.f, cq = 0.f;
#pragma unroll
            for (int w = 0; w < 8; ++w) mr_chan(cn, cm, cq, wn[w], red[buf][w][tid].x, red[buf][w][tid].y);
            part[(long long)blk * C + c0 + tid] = make_float2(cm, cq);
        }
    };

    if constexpr (PASS == 1) {
        __syncthreads();   // wn
        const float cnt = wn[wave];
        load_w1(0);
        for (int i = 0; i < nchunk; ++i) {
            r32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int s = 0; s < 32; ++s) acc = mr_mma(xf[0][s], w1c[s], acc);
            if (i + 1 < nchunk) load_w1(i + 1);
            float mean, m2;
            col_stats(acc, mk[0], cnt, mean, m2);
            if (h == 0) red[i & 1][wave][r32] = make_float2(mean, m2);
            __syncthreads();
            wave_merge(i & 1, MR_MC, mid, i * MR_MC);
        }
        return;
    }

    auto expand = [&]() {
#pragma unroll
        for (int j = 0; j < NBW; ++j) {
            const int pb = wave + 8 * j;
            if (pb < NBLK) {   // wave-uniform
                r32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = b1c;
#pragma unroll
                for (int s = 0; s < 32; ++s) acc = mr_mma(xf[j][s], w1c[s], acc);
                float* pl = A1 + r32 * A1P + 32 * pb + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float v[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int reg = 4 * g + i;
                        const float a = __builtin_amdgcn_fmed3f(acc[reg], 0.f, 6.f);
                        v[i] = (mk[j] >> reg) & 1u ? a : 0.f;
                    }
                    *reinterpret_cast<float4*>(pl + 8 * g) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        }
    };

    const int q4 = lane & 3, row = lane >> 2;    // depthwise: outputs (row, 4 q4 .. 4 q4 + 3)
    // the depthwise of one channel: 4 outputs per lane, the whole tile per wave
    auto dw_channel = [&](int cglob, int cc, r32x2& o01, r32x2& o23) {
        const float* tp = taps + (long long)cglob * TAPROW;
        float t[K * K + 1];
#pragma unroll
        for (int q = 0; q <= K * K; ++q) t[q] = tp[q];
        o01 = r32x2{t[K * K], t[K * K]};
        o23 = o01;
        const float* pl = A1 + cc * A1P + row * WC + 4 * q4;
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            float r[K + 3];
#pragma unroll
            for (int m = 0; m < (K + 3) / 2; ++m) {
                const float2 v = *reinterpret_cast<const float2*>(pl + ky * WC + 2 * m);
                r[2 * m] = v.x;
                r[2 * m + 1] = v.y;
            }
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const r32x2 tt = {t[ky * K + kx], t[ky * K + kx]};
                o01 = __builtin_elementwise_fma(r32x2{r[kx], r[kx + 1]}, tt, o01);
                o23 = __builtin_elementwise_fma(r32x2{r[kx + 2], r[kx + 3]}, tt, o23);
            }
        }
    };

    if constexpr (PASS == 2) {
        const bool rin = row < tile_rows;
        bool cin[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cin[i] = rin && 4 * q4 + i < tile_cols;
        load_w1(0);
        for (int i = 0; i < nchunk; ++i) {
            expand();
            __syncthreads();
            if (i + 1 < nchunk) load_w1(i + 1);
            constexpr int NCH = MR_MC / 8;
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const int cc = wave * NCH + k;     // wave-uniform
                r32x2 o01, o23;
                dw_channel(i * MR_MC + cc, cc, o01, o23);
                const float v[4] = {o01.x, o01.y, o23.x, o23.y};
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) s += cin[e] ? v[e] : 0.f;
                const float mean = mr_wave_sum(s) / tile_n;
                float q = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) q += cin[e] ? (v[e] - mean) * (v[e] - mean) : 0.f;
                const float m2 = mr_wave_sum(q);
                if (lane == 0) part[(long long)blk * mid + i * MR_MC + cc] = make_float2(mean, m2);
            }
            __syncthreads();
        }
        return;
    }

    // PASS 3: the whole block (BN1, BN2 folded), project raw
    r32x16 oacc[2];
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[ob][i] = 0.f;
    float w2c[2][16];
    auto load_w2 = [&](int ci) {
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int s = 0; s < 16; ++s) w2c[ob][s] = w2f[((ci * 2 + ob) * 16 + s) * 64 + lane];
    };
    auto depthwise = [&](int ci) {
        constexpr int NCH = MR_MC / 8;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int cc = wave * NCH + i;
            r32x2 o01, o23;
            dw_channel(ci * MR_MC + cc, cc, o01, o23);
            *reinterpret_cast<float4*>(A2 + cc * MR_A2P + 4 * lane) =
                make_float4(__builtin_amdgcn_fmed3f(o01.x, 0.f, 6.f), __builtin_amdgcn_fmed3f(o01.y, 0.f, 6.f),
                            __builtin_amdgcn_fmed3f(o23.x, 0.f, 6.f), __builtin_amdgcn_fmed3f(o23.y, 0.f, 6.f));
        }
    };
    auto project = [&]() {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float a = A2[(2 * s + h) * MR_A2P + 32 * wave + r32];
#pragma unroll
            for (int ob = 0; ob < 2; ++ob) oacc[ob] = mr_mma(a, w2c[ob][s], oacc[ob]);
        }
    };
    load_w1(0);
    for (int i = 0; i < nchunk; ++i) {
        if (i > 0) project();
        expand();
        __syncthreads();
        if (i + 1 < nchunk) load_w1(i + 1);
        load_w2(i);
        depthwise(i);
        __syncthreads();
    }
    project();

    // epilogue: y3 stored raw; lane (o = 32 ob + r32, h), register group g: tile pixels 32 wave + 8 g + 4 h + 0..3
    float* yn = y3 + (long long)n * 64 * plane;
    const bool vec = (W & 3) == 0;
    uint32_t om = 0u;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p0 = 32 * wave + 8 * g + 4 * h;
            if (h0 + p0 / MR_TILE < H && w0 + p0 % MR_TILE + i < W) om |= 1u << (4 * g + i);
        }
    const float cnt = wn[wave];    // written before the chunk loop's barriers
#pragma unroll
    for (int ob = 0; ob < 2; ++ob) {
        const int o = 32 * ob + r32;
        float mean, m2;
        col_stats(oacc[ob], om, cnt, mean, m2);
        if (h == 0) red[0][wave][o] = make_float2(mean, m2);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int p0 = 32 * wave + 8 * g + 4 * h;
            const int gh = h0 + p0 / MR_TILE, gw = w0 + p0 % MR_TILE;
            if (gh < H) {
                float* dst = yn + (long long)o * plane + gh * W + gw;
                if (vec && gw + 4 <= W) {
                    *reinterpret_cast<float4*>(dst) = make_float4(oacc[ob][4 * g], oacc[ob][4 * g + 1],
                                                                  oacc[ob][4 * g + 2], oacc[ob][4 * g + 3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (gw + i < W) dst[i] = oacc[ob][4 * g + i];
                }
            }
        }
    }
    __syncthreads();
    wave_merge(0, 64, 64, 0);
}

struct MrWs {
    size_t f, w1f, b1, taps, w2f, b3, stats, bn3, part, y3, total;
};
static MrWs mr_ws(const ofasr_mbconv_desc* d) {
    const size_t mid = (size_t)d->mid;
    const int K = d->K;
    const size_t blocks = (size_t)d->N * cdiv(d->H, MR_TILE) * cdiv(d->W, MR_TILE);
    MrWs s;
    size_t o = 0;
    s.f = o;     o += align_up(mid * K * K * sizeof(float), 256);
    s.w1f = o;   o += align_up(mid * 64 * sizeof(float), 256);
    s.b1 = o;    o += align_up(mid * sizeof(float), 256);
    s.taps = o;  o += align_up(mid * ((K * K + 1 + 3) / 4 * 4) * sizeof(float), 256);
    s.w2f = o;   o += align_up(64 * mid * sizeof(float), 256);
    s.b3 = o;    o += align_up(64 * sizeof(float), 256);
    s.stats = o; o += align_up(2 * 2 * mid * sizeof(float), 256);       // mean | var of BN1, then of BN2
    s.bn3 = o;   o += align_up(4 * 64 * sizeof(float), 256);            // mean | invstd | scale | shift of BN3
    s.part = o;  o += align_up(blocks * (mid > 64 ? mid : 64) * sizeof(float2), 256);   // S3 writes 64 channels
    s.y3 = o;    o += align_up((size_t)d->N * 64 * d->H * d->W * sizeof(float), 256);
    s.total = o;
    return s;
}

static bool mr_supported(const ofasr_mbconv_desc* d) {
    return d && d->dtype == OFASR_F32 && d->Cin == 64 && d->Cout == 64 && d->mid > 0 && d->mid % MR_MC == 0 &&
           (d->K == 3 || d->K == 5 || d->K == 7) && d->N > 0 && d->H > 0 && d->W > 0 &&
           64 * 4 * d->H * d->W <= INT32_MAX && d->N * cdiv(d->H, MR_TILE) * cdiv(d->W, MR_TILE) <= INT32_MAX;
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int ofasr_mbconv_recal_f32_supported(const ofasr_mbconv_desc* d) { return mr_supported(d) ? 1 : 0; }

OFASR_EXPORT size_t ofasr_mbconv_recal_f32_workspace(const ofasr_mbconv_desc* d) {
    return mr_supported(d) ? mr_ws(d).total : 0;
}

OFASR_EXPORT int ofasr_mbconv_recal_f32(const ofasr_mbconv_desc* d, const void* x, void* out, double* acc1,
                                        double* acc2, double* acc3, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    const char* name = "ofasr_mbconv_recal_f32";
    OFASR_REQUIRE(d != nullptr, OFASR_ERR_INVALID_ARG, "%s: null descriptor", name);
    OFASR_REQUIRE(mr_supported(d), OFASR_ERR_UNSUPPORTED,
                  "%s: needs fp32 activations, 64 -> mid (multiple of 32) -> 64 channels, K in {3,5,7}", name);
    OFASR_REQUIRE(x && out && acc1 && acc2 && acc3, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(d->w1 && d->w2 && d->wdw_max, OFASR_ERR_INVALID_ARG, "%s: null weight", name);
    for (int i = 0; i < 3; ++i)
        OFASR_REQUIRE(d->gamma[i] && d->beta[i], OFASR_ERR_INVALID_ARG, "%s: null BN affine tensor %d", name, i);
    OFASR_REQUIRE(d->chain_len >= 1 && d->chain_len <= 4 && d->ks[d->chain_len - 1] == d->K, OFASR_ERR_INVALID_ARG,
                  "%s: bad kernel chain", name);
    OFASR_REQUIRE(d->ldw1 >= 64 && d->ldw2 >= d->mid && d->Cmid_max >= d->mid, OFASR_ERR_INVALID_ARG,
                  "%s: weight shapes smaller than the block", name);
    const MrWs s = mr_ws(d);
    OFASR_REQUIRE_WORKSPACE(workspace, workspace_bytes, s.total);
    char* ws = (char*)workspace;
    float* f = reinterpret_cast<float*>(ws + s.f);
    float* w1f = reinterpret_cast<float*>(ws + s.w1f);
    float* b1 = reinterpret_cast<float*>(ws + s.b1);
    float* taps = reinterpret_cast<float*>(ws + s.taps);
    float* w2f = reinterpret_cast<float*>(ws + s.w2f);
    float* b3 = reinterpret_cast<float*>(ws + s.b3);
    float* st = reinterpret_cast<float*>(ws + s.stats);
    float* bn3 = reinterpret_cast<float*>(ws + s.bn3);
    float2* part = reinterpret_cast<float2*>(ws + s.part);
    float* y3 = reinterpret_cast<float*>(ws + s.y3);
    const int mid = (int)d->mid, H = (int)d->H, W = (int)d->W;
    const int tiles_x = (int)cdiv(d->W, MR_TILE), tiles_y = (int)cdiv(d->H, MR_TILE);
    const int blocks = (int)(d->N * (long long)tiles_x * tiles_y);
    hipStream_t strm = as_stream(stream);

    int rc = ofasr_ktransform_fwd(d->wdw_max, d->ks, d->chain_len - 1, d->mats, d->transform, f, d->mid, stream);
    if (rc) return rc;
    MrFold p;
    p.w1 = d->w1; p.ldw1 = d->ldw1; p.w2 = d->w2; p.ldw2 = d->ldw2; p.f = f;
    for (int i = 0; i < 3; ++i) {
        p.gamma[i] = d->gamma[i]; p.beta[i] = d->beta[i];
        p.mean[i] = nullptr; p.var[i] = nullptr;
        p.eps[i] = (float)d->bn_eps[i];
        p.fold[i] = 0;
    }
    p.mean[0] = st; p.var[0] = st + mid;
    p.mean[1] = st + 2 * mid; p.var[1] = st + 3 * mid;
    p.mid = mid; p.K = d->K;
    auto fold = [&](int upto) {
        for (int i = 0; i < 3; ++i) p.fold[i] = i < upto ? 1 : 0;
        OFASR_LAUNCH(mr_fold_kernel, dim3(96), dim3(256), 0, strm, p, w1f, b1, taps, w2f, b3);
    };
    auto merge = [&](int C, double* acc, float* mean, float* var, float* invstd, float* scale, float* shift, int bn) {
        MrOut o{acc, (double)d->N, mean, var, invstd, scale, shift, d->gamma[bn], d->beta[bn], d->bn_eps[bn]};
        OFASR_LAUNCH(mr_merge_kernel, dim3((unsigned)C), dim3(MR_MERGE_THREADS), 0, strm, (const float2*)part, blocks,
                     C, H, W, tiles_x, tiles_y, o);
    };
    const double px = (double)d->N * H * W;
    dispatch_int<7, 5, 3>(d->K, [&](auto KK) {
        const double win = (double)MrGeom<KK>::NBLK * 32.0 / 256.0;
        fold(0);
        prof_note(4.0 * px * 64, 2.0 * px * 64 * mid);
        OFASR_LAUNCH((mb_recal_f32_kernel<KK, 1>), dim3((unsigned)blocks), dim3(MR_THREADS), 0, strm, (const float*)x, y3, part,
                     w1f, b1, taps, w2f, mid, H, W, tiles_x, tiles_y);
        merge(mid, acc1, st, st + mid, nullptr, nullptr, nullptr, 0);
        fold(1);
        prof_note(4.0 * px * 64, 2.0 * px * (win * 64.0 * mid + (double)KK * KK * mid));
        OFASR_LAUNCH((mb_recal_f32_kernel<KK, 2>), dim3((unsigned)blocks), dim3(MR_THREADS), 0, strm, (const float*)x, y3, part,
                     w1f, b1, taps, w2f, mid, H, W, tiles_x, tiles_y);
        merge(mid, acc2, st + 2 * mid, st + 3 * mid, nullptr, nullptr, nullptr, 1);
        fold(2);
        prof_note(8.0 * px * 64, 2.0 * px * (win * 64.0 * mid + (double)KK * KK * mid + 64.0 * mid));
        OFASR_LAUNCH((mb_recal_f32_kernel<KK, 3>), dim3((unsigned)blocks), dim3(MR_THREADS), 0, strm, (const float*)x, y3, part,
                     w1f, b1, taps, w2f, mid, H, W, tiles_x, tiles_y);
    });
    rc = check_launch(name);
    if (rc) return rc;
    merge(64, acc3, bn3, nullptr, bn3 + 64, bn3 + 128, bn3 + 192, 2);
    rc = check_launch(name);
    if (rc) return rc;
    return ofasr_bn_act_fwd(y3, d->residual ? x : nullptr, out, bn3 + 128, bn3 + 192, bn3, d->N, 64, (int64_t)H * W, 0,
                            OFASR_F32, stream);
}

namespace ofasr {
// ofasr_bn_recal_accumulate: the bn_stats partials ([P][C] fp64 (sum, sum of squares), bnact.hip) -> batch mean and biased
// variance as bn_finalize forms them, into the accumulators and stats = mean | invstd | scale | shift
__global__ void __launch_bounds__(64) mr_accumulate_kernel(const double* __restrict__ partial, int P, int C, double M,
                                                           MrOut o) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, ss = 0.0;
    for (int p = 0; p < P; ++p) {
        s += partial[((long long)p * C + c) * 2];
        ss += partial[((long long)p * C + c) * 2 + 1];
    }
    const double mean = s / M;
    mr_finalize(o, C, c, mean, ss / M - mean * mean);
}
}  // namespace ofasr

OFASR_EXPORT int ofasr_bn_recal_accumulate(const void* partial, int64_t n_partials, int64_t C, double count,
                                           double weight, const float* gamma, const float* beta, double eps,
                                           double* acc, float* stats, void* stream) {
    const char* name = "ofasr_bn_recal_accumulate";
    OFASR_REQUIRE(partial && acc && stats, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n_partials > 0 && C > 0 && C <= INT32_MAX && n_partials <= INT32_MAX && count > 0.0,
                  OFASR_ERR_INVALID_ARG, "%s: bad sizes", name);
    MrOut o{acc, weight, stats, nullptr, stats + C, stats + 2 * C, stats + 3 * C, gamma, beta, eps};
    OFASR_LAUNCH(mr_accumulate_kernel, dim3((unsigned)cdiv(C, 64)), dim3(64), 0, as_stream(stream),
                 (const double*)partial, (int)n_partials, (int)C, count, o);
    return check_launch(name);
}
