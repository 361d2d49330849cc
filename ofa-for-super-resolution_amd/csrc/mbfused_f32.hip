// mbfused_f32.hip -- the WHOLE MB block as ONE kernel for eval-mode BatchNorm at fp32 (ofasr_mbconv_infer_f32_*):
//     out = x + BN3(W2 . relu6(BN2(dw_k(relu6(BN1(W1 . x))))))
// the fp32 counterpart of mbfused.hip (same descriptor, same BN folding), at the reference's precision: expand and project
// on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation), the depthwise on the vector pipe in fp32, no 16-bit
// operand anywhere.  The mid tensor never reaches HBM: the block reads x once (+ the shortcut re-read, an L2 hit) and writes
// out once.
//
// One workgroup (8 waves) = one 16x16 output tile of one image, all channels.  At fp32 the 16-bit kernel's LDS-staged x
// window (64 x 22 x 22 fp32 = 124 KB at k = 7) does not fit beside the mid planes, so x goes straight from global memory into
// the MFMA A fragments, which stay in registers for the whole block:
//   prologue  wave w owns window pixel blocks pb = w, w + 8 (32 window pixels each, the window is (16+2P) x (16+2P)):
//             lane l holds x[ch 2s + l/32][pixel 32 pb + l%32] for s = 0..31 -- 64 VGPRs.  Loads are buffer loads on a
//             resource that spans exactly this image's 64 planes; pixels outside the image or the window get an offset past
//             the resource's end, which the hardware answers with 0 without touching memory
//   per chunk of 32 mid channels (mid/32 chunks), two barriers:
//     [P(i-1) E(i)]  P: out[32 px x 64] += a2^T . W2f^T (accumulators resident, 16 k-steps x 2 column blocks)
//                    E: a1[32 px x 32 ch] = X^T . W1f^T + b1 per pixel block (32 k-steps), ReLU6, positions outside the
//                       image forced to 0 (the depthwise pads the ACTIVATED tensor) -> A1 planes [32][A1P]
//     [D(i)]         depthwise k x k from the planes, v_pk_fma_f32 on pairs of outputs: a lane owns 4 adjacent outputs of
//                    one row, 4 channels per wave; taps wave-uniform (scalar loads); + b2, ReLU6 -> A2 [32][A2P]
//   epilogue  + b3 (+ x), stored straight from the accumulators (4 adjacent pixels per lane and register group).
//
// LDS: A1 32 x (32 NBLK + 4) floats (66.0 / 53.8 / 45.6 KB at k = 7 / 5 / 3) + A2 32 x 288 floats (36 KB): <= 102 KB, one
// workgroup per CU.  Bounds at N=16, 64x64, mid 384, k = 7: matrix work 2 x (512/256 x 64 x 384 + 384 x 64) x 65536
// = 9.7 GFLOP (the window of 484 pixels is computed in 16 blocks of 32) -> 62 us at the 157 TF fp32 matrix peak; HBM
// 16.8 MB in + 16.8 MB out (+ the shortcut) -> 7-10 us.  The kernel is matrix-bound; DESIGN.md has the measured numbers.
#include "ofasr_common.h"

namespace ofasr {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int MG_THREADS = 512;
constexpr int MG_MC = 32;          // mid channels per chunk
constexpr int MG_A2P = 288;        // pixel pitch of the a2 planes: the two k-rows of a fragment read sit 32 banks apart
constexpr int MG_TILE = 16;        // output tile 16 x 16

template <int K> struct MgGeom {
    static constexpr int P = K / 2;
    static constexpr int WC = MG_TILE + 2 * P;          // window columns = rows
    static constexpr int NPIX = WC * WC;                // 324 / 400 / 484
    static constexpr int NBLK = (NPIX + 31) / 32;       // 11 / 13 / 16
    static constexpr int NBW = (NBLK + 7) / 8;          // pixel blocks per wave: 2
    static constexpr int A1P = NBLK * 32 + 4;
    static constexpr int TAPROW = (K * K + 1 + 3) / 4 * 4;   // K*K folded taps + the BN2 bias, padded
};

__device__ __forceinline__ int mg_acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__device__ __forceinline__ f32x16 mg_mma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// buffer resource over [base, base + bytes): loads at offsets >= bytes return 0 and access nothing
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mg_rsrc(const float* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, bytes, 0x00020000);
}
__device__ __forceinline__ float mg_load(__amdgpu_buffer_rsrc_t r, int off_bytes) {
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, off_bytes, 0, 0));
}

// ---- BN folding: the fp32 operand images -------------------------------------------------------------------
struct MgFold {
    const float* w1; long long ldw1;
    const float* w2; long long ldw2;
    const float* f;                      // active depthwise filter [mid][K][K] (ofasr_ktransform_fwd)
    const float* gamma[3]; const float* beta[3]; const float* mean[3]; const float* var[3];
    float eps[3];
    int mid, K;
};

__global__ void __launch_bounds__(256) mg_fold_kernel(MgFold p, float* __restrict__ w1f, float* __restrict__ b1,
                                                      float* __restrict__ taps, float* __restrict__ w2f,
                                                      float* __restrict__ b3) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    const int nth = gridDim.x * blockDim.x;
    const int mid = p.mid, K = p.K, TAPROW = (K * K + 1 + 3) / 4 * 4;
    auto scale = [&](int i, int c) { return p.gamma[i][c] / sqrtf(p.var[i][c] + p.eps[i]); };
    // fragment order: the value lane l needs for (chunk, k-step) sits at [(chunk, step)][l] (one coalesced 256-byte load)
    //   w1f[(ci*32 + s)*64 + l] = s1[c] W1[c][2 s + l/32],                      c = 32 ci + l%32
    //   w2f[((ci*2 + ob)*16 + s)*64 + l] = s3[o] W2[o][32 ci + 2 s + l/32],     o = 32 ob + l%32
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
        b1[c] = p.beta[0][c] - p.mean[0][c] * scale(0, c);
        float* row = taps + (long long)c * TAPROW;
        const float s2 = scale(1, c);
        for (int t = 0; t < K * K; ++t) row[t] = p.f[(long long)c * K * K + t] * s2;
        row[K * K] = p.beta[1][c] - p.mean[1][c] * s2;
        for (int t = K * K + 1; t < TAPROW; ++t) row[t] = 0.f;
    }
    for (int o = tid; o < 64; o += nth) b3[o] = p.beta[2][o] - p.mean[2][o] * scale(2, o);
}

// ---- the fused block ---------------------------------------------------------------------------------------
template <int K>
__global__ void __launch_bounds__(MG_THREADS) mb_fused_f32_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                  const float* __restrict__ w1f,
                                                                  const float* __restrict__ b1,
                                                                  const float* __restrict__ taps,
                                                                  const float* __restrict__ w2f,
                                                                  const float* __restrict__ b3, int mid, int H, int W,
                                                                  int tiles_x, int tiles_y, int residual) {
    using G = MgGeom<K>;
    constexpr int P = G::P, WC = G::WC, NPIX = G::NPIX, NBLK = G::NBLK, NBW = G::NBW, A1P = G::A1P;
    constexpr int TAPROW = G::TAPROW;
    __shared__ __attribute__((aligned(16))) float A1[MG_MC * A1P];
    __shared__ __attribute__((aligned(16))) float A2[MG_MC * MG_A2P];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r32 = lane & 31, h = lane >> 5;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    const int ty = b % tiles_y;
    const int n = b / tiles_y;
    const int h0 = ty * MG_TILE, w0 = tx * MG_TILE;
    const int plane = H * W;                        // 64 * plane * 4 < 2^31 (mg_supported)
    const int img_bytes = 64 * plane * 4;
    const float* xn = x + (long long)n * 64 * plane;
    const __amdgpu_buffer_rsrc_t xr = mg_rsrc(xn, img_bytes);

    // ---- prologue: X fragments of this wave's window pixel blocks; masks of the expand outputs
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
            xf[j][s] = mg_load(xr, ok ? pof + c * plane * 4 : img_bytes);
        }
        uint32_t m = 0u;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int q = 32 * pb + mg_acc_row(reg, h);
            const int qh = q / WC, qw = q - qh * WC;
            const int qgh = h0 - P + qh, qgw = w0 - P + qw;
            if (q < NPIX && qgh >= 0 && qgh < H && qgw >= 0 && qgw < W) m |= 1u << reg;
        }
        mk[j] = m;
    }

    f32x16 oacc[2];
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int i = 0; i < 16; ++i) oacc[ob][i] = 0.f;

    const int nchunk = mid / MG_MC;
    float w1c[32], w2c[2][16];
    float b1c = 0.f;
    auto load_w1 = [&](int ci) {
#pragma unroll
        for (int s = 0; s < 32; ++s) w1c[s] = w1f[(ci * 32 + s) * 64 + lane];
        b1c = b1[ci * MG_MC + r32];
    };
    auto load_w2 = [&](int ci) {
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int s = 0; s < 16; ++s) w2c[ob][s] = w2f[((ci * 2 + ob) * 16 + s) * 64 + lane];
    };

    auto expand = [&]() {
#pragma unroll
        for (int j = 0; j < NBW; ++j) {
            const int pb = wave + 8 * j;
            if (pb < NBLK) {   // wave-uniform
                f32x16 acc;
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[i] = b1c;   // the folded BN1 shift rides in the accumulator
#pragma unroll
                for (int s = 0; s < 32; ++s) acc = mg_mma(xf[j][s], w1c[s], acc);
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
    auto depthwise = [&](int ci) {
        constexpr int NCH = MG_MC / 8;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int cc = wave * NCH + i;     // wave-uniform
            const float* tp = taps + (long long)(ci * MG_MC + cc) * TAPROW;
            float t[K * K + 1];
#pragma unroll
            for (int q = 0; q <= K * K; ++q) t[q] = tp[q];
            f32x2 o01 = {t[K * K], t[K * K]}, o23 = o01;
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
                    const f32x2 tt = {t[ky * K + kx], t[ky * K + kx]};
                    o01 = __builtin_elementwise_fma(f32x2{r[kx], r[kx + 1]}, tt, o01);
                    o23 = __builtin_elementwise_fma(f32x2{r[kx + 2], r[kx + 3]}, tt, o23);
                }
            }
            *reinterpret_cast<float4*>(A2 + cc * MG_A2P + 4 * lane) =
                make_float4(__builtin_amdgcn_fmed3f(o01.x, 0.f, 6.f), __builtin_amdgcn_fmed3f(o01.y, 0.f, 6.f),
                            __builtin_amdgcn_fmed3f(o23.x, 0.f, 6.f), __builtin_amdgcn_fmed3f(o23.y, 0.f, 6.f));
        }
    };

    auto project = [&]() {
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float a = A2[(2 * s + h) * MG_A2P + 32 * wave + r32];
#pragma unroll
            for (int ob = 0; ob < 2; ++ob) oacc[ob] = mg_mma(a, w2c[ob][s], oacc[ob]);
        }
    };

    // ---- chunk loop: [P(i-1) E(i)] barrier [D(i)] barrier; the operands of the next phase are requested a phase ahead
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

    // ---- epilogue: + b3 (+ x); lane (o = 32 ob + r32, h), register group g: tile pixels 32 wave + 8 g + 4 h + 0..3
    float* on = out + (long long)n * 64 * plane;
    const bool vec = (W & 3) == 0;
    // the shortcut values first, all requested together (no shortcut: every offset is past the resource's end -> 0)
    float xv[2][4][4];
#pragma unroll
    for (int ob = 0; ob < 2; ++ob)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p0 = 32 * wave + 8 * g + 4 * h;
                const int gh = h0 + p0 / MG_TILE, gw = w0 + p0 % MG_TILE + i;
                const bool in = residual && gh < H && gw < W;
                xv[ob][g][i] = mg_load(xr, in ? ((32 * ob + r32) * plane + gh * W + gw) * 4 : img_bytes);
            }
#pragma unroll
    for (int ob = 0; ob < 2; ++ob) {
        const int o = 32 * ob + r32;
        const float bias = b3[o];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int p0 = 32 * wave + 8 * g + 4 * h;
            const int gh = h0 + p0 / MG_TILE, gw = w0 + p0 % MG_TILE;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = oacc[ob][4 * g + i] + bias + xv[ob][g][i];
            if (gh < H) {
                float* dst = on + (long long)o * plane + gh * W + gw;
                if (vec && gw + 4 <= W) {
                    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (gw + i < W) dst[i] = v[i];
                }
            }
        }
    }
}

struct MgWs {
    size_t f, w1f, b1, taps, w2f, b3, total;
};
static MgWs mg_ws(const ofasr_mbconv_desc* d) {
    const size_t mid = (size_t)d->mid;
    const int K = d->K;
    MgWs s;
    size_t o = 0;
    s.f = o;    o += align_up(mid * K * K * sizeof(float), 256);
    s.w1f = o;  o += align_up(mid * 64 * sizeof(float), 256);
    s.b1 = o;   o += align_up(mid * sizeof(float), 256);
    s.taps = o; o += align_up(mid * ((K * K + 1 + 3) / 4 * 4) * sizeof(float), 256);
    s.w2f = o;  o += align_up(64 * mid * sizeof(float), 256);
    s.b3 = o;   o += align_up(64 * sizeof(float), 256);
    s.total = o;
    return s;
}

static bool mg_supported(const ofasr_mbconv_desc* d) {
    return d && d->dtype == OFASR_F32 && d->Cin == 64 && d->Cout == 64 && d->mid > 0 && d->mid % MG_MC == 0 &&
           (d->K == 3 || d->K == 5 || d->K == 7) && !d->bn_training[0] && !d->bn_training[1] && !d->bn_training[2] &&
           d->N > 0 && d->H > 0 && d->W > 0 && 64 * 4 * d->H * d->W <= INT32_MAX &&
           d->N * cdiv(d->H, MG_TILE) * cdiv(d->W, MG_TILE) <= INT32_MAX;
}

static int mg_check(const char* name, const ofasr_mbconv_desc* d) {
    OFASR_REQUIRE(d != nullptr, OFASR_ERR_INVALID_ARG, "%s: null descriptor", name);
    OFASR_REQUIRE(mg_supported(d), OFASR_ERR_UNSUPPORTED,
                  "%s: needs eval-mode BN, fp32 activations, 64 -> mid (multiple of 32) -> 64 channels, K in {3,5,7}", name);
    return OFASR_OK;
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int ofasr_mbconv_infer_f32_supported(const ofasr_mbconv_desc* d) { return mg_supported(d) ? 1 : 0; }

OFASR_EXPORT size_t ofasr_mbconv_infer_f32_operand_bytes(const ofasr_mbconv_desc* d) {
    return mg_supported(d) ? mg_ws(d).total : 0;
}

OFASR_EXPORT size_t ofasr_mbconv_infer_f32_scratch_bytes(const ofasr_mbconv_desc* d) {
    (void)d;
    return 0;
}

OFASR_EXPORT int ofasr_mbconv_infer_f32_prepare(const ofasr_mbconv_desc* d, void* operands, size_t operand_bytes,
                                                void* stream) {
    const char* name = "ofasr_mbconv_infer_f32_prepare";
    int rc = mg_check(name, d);
    if (rc) return rc;
    OFASR_REQUIRE(d->w1 && d->w2 && d->wdw_max, OFASR_ERR_INVALID_ARG, "%s: null weight", name);
    for (int i = 0; i < 3; ++i)
        OFASR_REQUIRE(d->gamma[i] && d->beta[i] && d->running_mean[i] && d->running_var[i], OFASR_ERR_INVALID_ARG,
                      "%s: null BN tensor %d", name, i);
    OFASR_REQUIRE(d->chain_len >= 1 && d->chain_len <= 4 && d->ks[d->chain_len - 1] == d->K, OFASR_ERR_INVALID_ARG,
                  "%s: bad kernel chain", name);
    OFASR_REQUIRE(d->ldw1 >= 64 && d->ldw2 >= d->mid && d->Cmid_max >= d->mid, OFASR_ERR_INVALID_ARG,
                  "%s: weight shapes smaller than the block", name);
    const MgWs s = mg_ws(d);
    OFASR_REQUIRE(operands && operand_bytes >= s.total, OFASR_ERR_WORKSPACE, "%s: operand buffer %zu B < required %zu B",
                  name, operand_bytes, s.total);
    char* ws = (char*)operands;
    rc = ofasr_ktransform_fwd(d->wdw_max, d->ks, d->chain_len - 1, d->mats, d->transform,
                              reinterpret_cast<float*>(ws + s.f), d->mid, stream);
    if (rc) return rc;
    MgFold p;
    p.w1 = d->w1; p.ldw1 = d->ldw1; p.w2 = d->w2; p.ldw2 = d->ldw2;
    p.f = reinterpret_cast<const float*>(ws + s.f);
    for (int i = 0; i < 3; ++i) {
        p.gamma[i] = d->gamma[i]; p.beta[i] = d->beta[i]; p.mean[i] = d->running_mean[i]; p.var[i] = d->running_var[i];
        p.eps[i] = (float)d->bn_eps[i];
    }
    p.mid = (int)d->mid; p.K = d->K;
    OFASR_LAUNCH(mg_fold_kernel, dim3(96), dim3(256), 0, as_stream(stream), p, reinterpret_cast<float*>(ws + s.w1f),
                 reinterpret_cast<float*>(ws + s.b1), reinterpret_cast<float*>(ws + s.taps),
                 reinterpret_cast<float*>(ws + s.w2f), reinterpret_cast<float*>(ws + s.b3));
    return check_launch(name);
}

OFASR_EXPORT int ofasr_mbconv_infer_f32_run(const ofasr_mbconv_desc* d, const void* x, void* out, const void* operands,
                                            size_t operand_bytes, void* scratch, size_t scratch_bytes, void* stream) {
    (void)scratch;
    (void)scratch_bytes;
    const char* name = "ofasr_mbconv_infer_f32_run";
    int rc = mg_check(name, d);
    if (rc) return rc;
    OFASR_REQUIRE(x && out, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    const MgWs s = mg_ws(d);
    OFASR_REQUIRE(operands && operand_bytes >= s.total, OFASR_ERR_WORKSPACE, "%s: operand buffer %zu B < required %zu B",
                  name, operand_bytes, s.total);
    const char* ws = (const char*)operands;
    const float* w1f = reinterpret_cast<const float*>(ws + s.w1f);
    const float* b1 = reinterpret_cast<const float*>(ws + s.b1);
    const float* taps = reinterpret_cast<const float*>(ws + s.taps);
    const float* w2f = reinterpret_cast<const float*>(ws + s.w2f);
    const float* b3 = reinterpret_cast<const float*>(ws + s.b3);
    const int tiles_x = (int)cdiv(d->W, MG_TILE), tiles_y = (int)cdiv(d->H, MG_TILE);
    const long long blocks = d->N * (long long)tiles_x * tiles_y;
    const double px = (double)d->N * (double)d->H * (double)d->W;
    prof_note(4.0 * px * 64 * (d->residual ? 3.0 : 2.0), 2.0 * px * (2.0 * 64 * d->mid + (double)d->K * d->K * d->mid));
    hipStream_t st = as_stream(stream);
    dispatch_int<7, 5, 3>(d->K, [&](auto KK) {
        OFASR_LAUNCH(mb_fused_f32_kernel<KK>, dim3((unsigned)blocks), dim3(MG_THREADS), 0, st, (const float*)x, (float*)out, w1f,
                     b1, taps, w2f, b3, (int)d->mid, (int)d->H, (int)d->W, tiles_x, tiles_y, d->residual);
    });
    return check_launch(name);
}
