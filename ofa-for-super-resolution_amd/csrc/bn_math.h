// bn_math.h -- the BatchNorm arithmetic of the training path, each rule stated once.  The depthwise and pointwise
// kernels never run BatchNorm as a pass of its own: they finalize their producer's statistics, apply BN + ReLU6 as they
// load an operand and form the BN backward from (da, y) as they read the gradient; bnact.hip holds the passes that
// remain.  All of them take their arithmetic from here:
//   bn_moments / bn_coef / bn_affine      fp64 finalize: mean, clamped biased variance, invstd, scale, shift;
//   bn_unbiased_var / bn_ema              the running-statistics update;
//   bn_bwd_coef / bn_bwd_means            the backward's per-channel coefficients (fused read / pass form);
//   bn_beta / bn_pre / relu6 / relu6_gate / bn_bwd_dy / bn_bwd_dx     the elementwise pieces;
//   bn_publish, bn_fold_finish, bn_fold_wave        the designated writer's stores and a consumer's whole finalize;
//   bn_fold_cp / bn_fold_pc2 / bn_fold_cp_wave, bwdxf_fold            the partial folds;
//   xf_apply8_core / xf_apply8 / bx_apply8          the fused reads of 8 packed 16-bit values;
//   InputXf, BwdXf, BwdStatOut, BnFold, StatOut     what a launch hands a kernel to do so.
// The scalar rules are __host__ __device__: tests/host/bn_math_check.hip walks them on the CPU over extreme inputs.
// Everything is __forceinline__; a fold fixes its summation order (the step is bit-reproducible because of it) and
// only groups the loads.  Included by ofasr_common.h after the 16-bit element types; include that header, not this one.
#pragma once
#include <math.h>

namespace ofasr {

// ---- scalar rules ------------------------------------------------------------------------------------------------------
// The ReLU6 window is STRICT in the backward (hardtanh_backward: the gradient passes where 0 < pre < 6) and the
// forward clamps to its closed ends.
constexpr float RELU6_MAX = 6.f;

// mean and BIASED variance from (sum, sum of squares) over M values; E[x^2] - mean^2 can round below zero: var >= 0
struct BnMoments { double mean, var; };
__host__ __device__ __forceinline__ BnMoments bn_moments(double s, double ss, double M) {
    const double mean = s / M;
    double var = ss / M - mean * mean;
    var = var < 0.0 ? 0.0 : var;
    return BnMoments{mean, var};
}

// gamma[c] / beta[c], or the identity value of an absent parameter
__host__ __device__ __forceinline__ double bn_affine(const float* p, int c, double absent) { return p ? (double)p[c] : absent; }

// invstd, scale = gamma * invstd, shift = beta - mean * scale (from the fp64 product, not the rounded scale); beta rides
// along as the fp32 the centred form uses
struct BnCoef {
    double invstd;
    float scale, shift, beta;
};
__host__ __device__ __forceinline__ BnCoef bn_coef(BnMoments m, double eps, double g, double b) {
    const double invstd = 1.0 / sqrt(m.var + eps);
    return BnCoef{invstd, (float)(g * invstd), (float)(b - m.mean * g * invstd), (float)b};
}

// running statistics: EMA of the mean and of the UNBIASED variance (M = 1 has none: the biased one stands in)
__host__ __device__ __forceinline__ double bn_unbiased_var(double var, double M) { return M > 1.0 ? var * M / (M - 1.0) : var; }
__host__ __device__ __forceinline__ float bn_ema(float running, double momentum, double value) {
    return (float)((1.0 - momentum) * (double)running + momentum * value);
}

// Backward, per channel, from s = sum dz and sx = sum dz * xhat (xhat = (y - mean) * invstd) over M values.
// TWO partial conventions feed it:
//   the reduction pass (bn_bwd_reduce_kernel, [P][C][2] doubles) carries  sum dz * xhat  itself;
//   a producer's epilogue (BwdStatOut, [C][P] float2; bn_bwd_coef_cp) carries  sum dz * (y - mean)  and the fold
//   multiplies by invstd afterwards (the producer need not know invstd).
// and TWO forms consume it, which round differently and both stay as they are:
//   fused read (BwdXf):  dy = -t * kbi + (scale * dz - ka),  t = y - mean,  ka = scale * s / M,  kbi = scale * invstd * sx / M
//   pass form (bnact):   dx = scale * (dz - a - t * invstd * b),  a = s / M,  b = sx / M
// Eval-mode BN has constant statistics: every coefficient is exactly 0.
__host__ __device__ __forceinline__ void bn_bwd_coef(double s, double sx, double sc, double invstd, double M, int training,
                                                     float& ka, float& kbi) {
    ka = training ? (float)(sc * (s / M)) : 0.f;
    kbi = training ? (float)(sc * invstd * (sx / M)) : 0.f;
}
__host__ __device__ __forceinline__ void bn_bwd_means(double s, double sx, double M, int training, float& a, float& b) {
    a = training ? (float)(s / M) : 0.f;
    b = training ? (float)(sx / M) : 0.f;
}

// centred form (v - mean) * scale + beta': v * scale + shift cancels when |mean| >> std.  beta' = shift + mean * scale
__host__ __device__ __forceinline__ float bn_beta(float mu, float sc, float shift) { return fmaf(mu, sc, shift); }
__host__ __device__ __forceinline__ float bn_pre(float v, float mu, float sc, float b) { return fmaf(v - mu, sc, b); }
__host__ __device__ __forceinline__ float relu6(float v) { return fminf(fmaxf(v, 0.f), RELU6_MAX); }
__host__ __device__ __forceinline__ float relu6_gate(float pre, float dz) { return (pre > 0.f && pre < RELU6_MAX) ? dz : 0.f; }
__host__ __device__ __forceinline__ float bn_bwd_dy(float t, float dz, float sc, float ka, float kbi) {
    return fmaf(-t, kbi, fmaf(sc, dz, -ka));
}
__host__ __device__ __forceinline__ float bn_bwd_dx(float t, float dz, float k1, float is, float a, float b) {
    return k1 * (dz - a - t * is * b);
}

// ---- what a launch hands a kernel --------------------------------------------------------------------------------------
// Optional BatchNorm + ReLU6 applied to an operand as a kernel reads it (the composite MB block never materialises
// the activated tensor): v -> relu6(bn_pre(v, mean[c], scale[c], bn_beta(..))).  Zero padding / out-of-range elements
// stay exactly zero.  All pointers null = plain read.
struct InputXf {
    const float* scale;
    const float* shift;
    const float* mean;
};

// BatchNorm(+ReLU6) BACKWARD applied to an operand as a kernel reads it: the gradient dy of the pre-BN tensor y is
// bn_bwd_dy(t, relu6_gate(bn_pre(y), da), ..) (the fused-read form above), formed from the incoming gradient da and y
// on the fly, so the "apply" pass of the BN backward -- read da, read y, write dy -- never runs and dy is a pass of its
// own no more.  The per-channel sums behind ka / kbi come from bn_bwd_reduce_coef.  The kernel that consumes dy on the
// input-gradient chain also stores it once (dy_out, may be null) for the weight-gradient kernel on the side stream:
// compared with the separate pass the chain moves one tensor less (no second read of da) and loses a launch, and the
// side stream reads what it read before.  y == nullptr: plain read.
struct BwdXf {
    const void* y;        // the pre-BN tensor, same shape and element type as the gradient operand
    const float* mean;
    const float* scale;   // gamma * invstd
    const float* shift;   // beta - mean * scale
    const float* ka;
    const float* kbi;
    void* dy_out;         // where the consumer leaves dy (same shape / element type), or nullptr
    // Optional: the consumer folds the reduction pass's partial slabs itself (no coefficient launch between the two).
    // fold_partial[(q * C + c) * 2 + {0, 1}] = (sum dz, sum dz * xhat) of part q < fold_P (bn_bwd_reduce_kernel's layout),
    // folded in fp64 in the order q = 0 .. fold_P-1 exactly as bn_bwd_coef_kernel does; ka / kbi above are then ignored.
    // ONE designated unit per channel also writes dgamma / dbeta and (coef_ka, coef_kbi) -- the latter for a later kernel
    // that takes finished coefficients (the side stream's weight gradient).
    const double* fold_partial;
    int fold_P, fold_C, fold_training;
    double fold_M;
    const float* fold_invstd;
    float* fold_dgamma;
    float* fold_dbeta;
    float* coef_ka;
    float* coef_kbi;
};
// The REDUCTION pass of the same backward folded into the kernel that produces da (the gradient of the activated
// tensor): the producer reads y at the positions it writes and leaves, per channel c and producer unit p (a pixel tile,
// a plane slab), partial[c * P + p] = (sum dz, sum dz * (y - mean)) with dz as above and da as stored; bn_bwd_coef_cp
// folds the P partials of a channel in fp64 in a fixed order into dgamma, dbeta, ka, kbi.  The chain loses the pass
// "read da, read y" and its launch; the producer reads y (one tensor) more.
struct BwdStatOut {
    const void* y;
    const float* mean;
    const float* scale;
    const float* shift;
    float2* partial;
    int P;
};
// A consumer kernel can fold the producer's epilogue partials itself (no finalize launch between the two): every
// block derives scale / mean / beta of the channels it reads from partial[c * P + 0..P) in fp64 in a fixed order, and
// one designated block also writes mean | invstd | scale | shift (kept for the backward) and the running statistics.
// cp == nullptr: not used (the InputXf pointers hold finalized values).
struct BnFold {
    const float2* cp;
    int P;
    double M, momentum, eps;
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    float* mean;
    float* invstd;
    float* scale;
    float* shift;
    int64_t* counters[3];   // num_batches_tracked of the block's BNs, bumped once by the designated writer (may be null)
};
// Optional BatchNorm statistics of the tensor a conv kernel writes: every producer unit p (a pixel tile, a plane slab)
// leaves its per-channel (sum, sum of squares) at partial[c * P + p] -- fp32 over <= a few thousand values -- and
// bn_finalize_cp folds the P partials of a channel in fp64 in a fixed order.  partial == nullptr: no statistics.
struct StatOut {
    float2* partial;
    int P;
};

#if defined(__HIPCC__)
// ---- device only: publish ----------------------------------------------------------------------------------------------
// The designated writer of channel c stores mean | invstd | scale | shift, moves the running statistics (`running`:
// batch statistics and buffers present) and, where `bump` (the caller's channel-0 writer), the up to three counters
// (entries may be null).  Dst: anything with mean, invstd, scale, shift, running_mean, running_var, momentum (BnFold, BnSource, BnStatsOut).
struct BnStatsOut {
    float* mean;
    float* invstd;
    float* scale;
    float* shift;
    float* running_mean;
    float* running_var;
    double momentum;
};
template <typename Dst>
__device__ __forceinline__ void bn_publish(const Dst& d, int c, BnMoments m, BnCoef k, double M, bool running, bool bump,
                                           int64_t* const (&counters)[3]) {
    d.mean[c] = (float)m.mean;
    d.invstd[c] = (float)k.invstd;
    d.scale[c] = k.scale;
    d.shift[c] = k.shift;
    if (running) {
        d.running_mean[c] = bn_ema(d.running_mean[c], d.momentum, m.mean);
        d.running_var[c] = bn_ema(d.running_var[c], d.momentum, bn_unbiased_var(m.var, M));
    }
    if (bump) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (counters[i]) *counters[i] += 1;
    }
}

// ---- device only: partial folds ----------------------------------------------------------------------------------------
// 8 requests per round with a clamped index (the loads of a round are in flight together; one load per iteration is P
// dependent L2 round trips), summed in order; a slot past the end adds 0.0, which leaves a sum that started at +0.0 as it is.
// in order over the float2 [C][P] layout; pc = partial + c * P
__device__ __forceinline__ void bn_fold_cp(const float2* pc, int P, double& s, double& ss) {
    s = 0.0, ss = 0.0;
    for (int q0 = 0; q0 < P; q0 += 8) {
        float2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = pc[q0 + j < P ? q0 + j : P - 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool live = q0 + j < P;
            s += live ? (double)v[j].x : 0.0;
            ss += live ? (double)v[j].y : 0.0;
        }
    }
}
// in order over the double [P][C][2] layout
__device__ __forceinline__ void bn_fold_pc2(const double* partial, int P, int C, int c, double& s, double& sx) {
    s = 0.0, sx = 0.0;
    for (int q0 = 0; q0 < P; q0 += 8) {
        double a[8], b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int q = q0 + j < P ? q0 + j : P - 1;
            a[j] = partial[((long long)q * C + c) * 2];
            b[j] = partial[((long long)q * C + c) * 2 + 1];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            s += q0 + j < P ? a[j] : 0.0;
            sx += q0 + j < P ? b[j] : 0.0;
        }
    }
}
// one wave per channel over the float2 [C][P] layout: lane l sums partials l, l + 64, .. in order, then a fixed
// butterfly; the result is valid in every lane
__device__ __forceinline__ void bn_fold_cp_wave(const float2* pc, int P, int lane, double& s, double& ss) {
    s = 0.0, ss = 0.0;
    for (int q0 = lane; q0 < P; q0 += 8 * 64) {
        float2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = pc[q0 + 64 * j < P ? q0 + 64 * j : P - 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool live = q0 + 64 * j < P;
            s += live ? (double)v[j].x : 0.0;
            ss += live ? (double)v[j].y : 0.0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        ss += __shfl_xor(ss, o, 64);
    }
}

// ---- device only: a consumer's finalize of its input BN (BnFold) ---------------------------------------------------------
// (scale, mean, beta) of channel c for the centred read from the folded sums; `writer` also publishes (training mode by
// construction: a BnFold carries batch partials)
__device__ __forceinline__ void bn_fold_finish(const BnFold& fold, int c, double s, double ss, bool writer, float& sc,
                                               float& mu, float& b) {
    const BnMoments m = bn_moments(s, ss, fold.M);
    const BnCoef k = bn_coef(m, fold.eps, bn_affine(fold.gamma, c, 1.0), bn_affine(fold.beta, c, 0.0));
    sc = k.scale;
    mu = (float)m.mean;
    b = k.beta;
    if (writer) bn_publish(fold, c, m, k, fold.M, fold.running_mean != nullptr, c == 0, fold.counters);
}
// the same by one wave from the partials themselves
__device__ __forceinline__ void bn_fold_wave(const BnFold& fold, int c, int lane, bool writer, float& sc, float& mu, float& b) {
    double s, ss;
    bn_fold_cp_wave(fold.cp + (long long)c * fold.P, fold.P, lane, s, ss);
    bn_fold_finish(fold, c, s, ss, writer, sc, mu, b);
}

// (ka, kbi) of channel c from the reduction pass's partial slabs; `writer`: this unit also publishes dgamma / dbeta / the
// coefficients
__device__ __forceinline__ void bwdxf_fold(const BwdXf& bx, int c, float sc, bool writer, float& ka, float& kbi) {
    double s, sx;
    bn_fold_pc2(bx.fold_partial, bx.fold_P, bx.fold_C, c, s, sx);
    bn_bwd_coef(s, sx, (double)sc, (double)bx.fold_invstd[c], bx.fold_M, bx.fold_training, ka, kbi);
    if (writer) {
        if (bx.fold_dgamma) bx.fold_dgamma[c] = (float)sx;
        if (bx.fold_dbeta) bx.fold_dbeta[c] = (float)s;
        if (bx.coef_ka) bx.coef_ka[c] = ka;
        if (bx.coef_kbi) bx.coef_kbi[c] = kbi;
    }
}

// ---- device only: fused reads of 8 packed 16-bit values ------------------------------------------------------------------
// BN + ReLU6 of 8 values of one channel (InputXf); b = bn_beta(mu, sc, shift)
template <typename T>
__device__ __forceinline__ uint4 xf_apply8_core(uint4 v, float sc, float mu, float b) {
    uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        T lo, hi;
        lo.v = (uint16_t)(w[i] & 0xffffu);
        hi.v = (uint16_t)(w[i] >> 16);
        w[i] = pack2<T>(relu6(bn_pre(to_float(lo), mu, sc, b)), relu6(bn_pre(to_float(hi), mu, sc, b)));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
template <typename T>
__device__ __forceinline__ uint4 xf_apply8(uint4 v, const InputXf& xf, int ch) {
    const float sc = xf.scale[ch], mu = xf.mean[ch];
    return xf_apply8_core<T>(v, sc, mu, bn_beta(mu, sc, xf.shift[ch]));
}
// BN(+ReLU6) backward of 8 gradient values `g` of one channel given the 8 pre-BN values `yv` (BwdXf); xb as b above
template <typename T>
__device__ __forceinline__ uint4 bx_apply8(uint4 g, uint4 yv, float mu, float sc, float xb, float ka, float kbi) {
    uint32_t w[4] = {g.x, g.y, g.z, g.w};
    const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        T lo, hi, ylo, yhi;
        lo.v = (uint16_t)(w[i] & 0xffffu);
        hi.v = (uint16_t)(w[i] >> 16);
        ylo.v = (uint16_t)(yw[i] & 0xffffu);
        yhi.v = (uint16_t)(yw[i] >> 16);
        const float y0 = to_float(ylo), y1 = to_float(yhi), t0 = y0 - mu, t1 = y1 - mu;
        const float z0 = relu6_gate(bn_pre(y0, mu, sc, xb), to_float(lo)), z1 = relu6_gate(bn_pre(y1, mu, sc, xb), to_float(hi));
        w[i] = pack2<T>(bn_bwd_dy(t0, z0, sc, ka, kbi), bn_bwd_dy(t1, z1, sc, ka, kbi));
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}
#endif

}  // namespace ofasr
