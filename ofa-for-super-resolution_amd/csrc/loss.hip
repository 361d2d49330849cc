// loss.hip -- the training loss of one batch, its gradient and the logged Y-PSNR (ofasr_sr_loss_fwd / ofasr_sr_loss_bwd),
// and the same with an SSIM term (ofasr_sr_loss_ssim_fwd / ofasr_sr_loss_ssim_bwd: the second half of this file).
//
// Definition (losses.py is the host statement; include/ofasr.h): o, t and optionally s are
// [N, 3, H, W] batches of f32 / f16 / bf16, each read as fp32; d = o - t, e = o - s; rho is x*x (mse), |x| (l1) or
// sqrt(x*x + eps2) (charbonnier), every step one fp32 operation with a correctly rounded sqrt and division;
// L = w_main * sum rho(d) / M + w_kd * sum rho(e) / M with fp64 sums in a fixed order; the gradient with respect to o is
// fl(fl(ga * rho'(d)) + fl(gb * rho'(e))) rounded into o's format; the metric is the exact int64 squared error of the two
// luma images (quality_math.h) and its PSNR over a pixel count the caller passes.
//
// Walk.  The unit is a chunk of 8 horizontally consecutive pixels of one image: a lane reads the chunk from each of the
// three colour planes of every operand, so that it holds the whole pixel for the luma and the 24 elements for the loss
// sums in one pass over the memory.  Chunks are dealt to the lanes grid-stride.  When every tensor of the call lies at a
// 16-byte aligned address and H * W % 8 == 0 -- every plane then starts on a 16-byte boundary and no chunk is partial --
// the VEC kernels read (the gradient: write) 16-byte requests; otherwise the other variant goes in 2-byte requests, each
// index clamped to the last element of its plane.  Inside a variant nothing branches on an operand's format: addresses
// are selected, the raw words are read, and the fp32 / bf16 / f16 readings are selected afterwards, so the requests of
// all operands and planes of a chunk are in flight together.  Lanes past the last chunk run the last chunk again: every
// lane issues every load from a valid address and the surplus is masked out of the sums afterwards (no load under a
// lane-dependent branch, DESIGN.md section 6 rule 3); the gradient's surplus stores repeat the owner's bytes at the
// owner's address, so they too stand under no branch.  64-bit offsets throughout.
//
// Forward: a workgroup folds its lanes (shuffles, then the 4 wave totals in order) into one partial in the workspace; a
// second launch of one workgroup adds the partials in index order and writes the result buffer.  No atomics: two runs
// give identical bits.  Backward: the same walk; g is read from device memory, so the caller needs neither a host read
// nor a multiply of its own.
#include "quality_math.h"   // q_quant, q_luma
#include <math.h>

#pragma clang fp contract(off)   // every fp32 step of the statement is its own rounding

namespace ofasr {

constexpr int LC = 8;             // pixels per chunk
constexpr int L_MAX_PARTS = 2048;

struct LOperand {
    const void* p;
    int fmt;                      // OFASR_F32 / OFASR_F16 / OFASR_BF16
};

struct alignas(16) LPartial {
    double sa, sb;
    long long sse;
    long long pad;
};

// The 8 elements at `at` .. `at + 7` of an operand, with no branch on its format: the requests are issued from selected
// addresses and the three readings of the raw words (fp32, bf16, f16) are selected afterwards, so that all operands' and
// planes' requests of a chunk stand in one block of code and are in flight together.  VEC: two 16-byte requests (a
// 16-bit operand repeats its one); else 2-byte requests, two per element (a 16-bit element repeats its one), every
// index clamped to `last`.
template <bool VEC>
__device__ __forceinline__ void l_load8(const LOperand& a, long long at, long long last, float (&v)[LC]) {
    const bool wide = a.fmt == OFASR_F32, bf = a.fmt == OFASR_BF16;
    uint32_t w32[LC], w16[LC];
    if (VEC) {
        const char* p = reinterpret_cast<const char*>(a.p) + at * (wide ? 4 : 2);
        const uint4 lo = *reinterpret_cast<const uint4*>(p);
        const uint4 hi = *reinterpret_cast<const uint4*>(p + (wide ? 16 : 0));
        const uint32_t l[LC] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int j = 0; j < LC; ++j) {
            w32[j] = l[j];
            w16[j] = (l[j >> 1] >> (16 * (j & 1))) & 0xffffu;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LC; ++j) {
            const long long i = at + j < last ? at + j : last;
            const uint16_t* q = reinterpret_cast<const uint16_t*>(a.p) + i * (wide ? 2 : 1);
            const uint32_t a0 = q[0], a1 = q[wide ? 1 : 0];
            w32[j] = a0 | (a1 << 16);
            w16[j] = a0;
        }
    }
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        const float fb = to_float(bf16_t{(uint16_t)w16[j]}), fh = to_float(f16_t{(uint16_t)w16[j]});
        v[j] = wide ? __uint_as_float(w32[j]) : (bf ? fb : fh);
    }
}

// The counterpart store, rounding to nearest even into the format, as branch-free: a 16-bit format stores its bytes
// twice at the same address.  Element by element, the slots past `last` hold the value of `last` (their loads were
// clamped the same way) and store it again.
template <bool VEC>
__device__ __forceinline__ void l_store8(void* p, int fmt, long long at, long long last, const float (&u)[LC]) {
    const bool wide = fmt == OFASR_F32, bf = fmt == OFASR_BF16;
    // The fp32 value is final before it is narrowed: left to itself the compiler folds the product in front of an f16
    // conversion into v_fma_mixlo_f16, which rounds the exact product ONCE into f16 -- not fl32 first, as the statement
    // has it (one word in 36864 differed, at an f16 subnormal).  An empty asm makes each value opaque.
    float v[LC];
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        v[j] = u[j];
        asm volatile("" : "+v"(v[j]));
    }
    if (VEC) {
        uint32_t h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t pb = pack2<bf16_t>(v[2 * j], v[2 * j + 1]), ph = pack2<f16_t>(v[2 * j], v[2 * j + 1]);
            h[j] = bf ? pb : ph;
        }
        char* q = reinterpret_cast<char*>(p) + at * (wide ? 4 : 2);
        uint4 lo, hi;
        lo.x = wide ? __float_as_uint(v[0]) : h[0], lo.y = wide ? __float_as_uint(v[1]) : h[1];
        lo.z = wide ? __float_as_uint(v[2]) : h[2], lo.w = wide ? __float_as_uint(v[3]) : h[3];
        hi.x = wide ? __float_as_uint(v[4]) : h[0], hi.y = wide ? __float_as_uint(v[5]) : h[1];
        hi.z = wide ? __float_as_uint(v[6]) : h[2], hi.w = wide ? __float_as_uint(v[7]) : h[3];
        *reinterpret_cast<uint4*>(q) = lo;
        *reinterpret_cast<uint4*>(q + (wide ? 16 : 0)) = hi;
    } else {
#pragma unroll
        for (int j = 0; j < LC; ++j) {
            const long long i = at + j < last ? at + j : last;
            const uint32_t w = __float_as_uint(v[j]);
            const uint32_t s = bf ? (uint32_t)from_float<bf16_t>(v[j]).v : (uint32_t)from_float<f16_t>(v[j]).v;
            uint16_t* q = reinterpret_cast<uint16_t*>(p) + i * (wide ? 2 : 1);
            q[0] = (uint16_t)(wide ? w & 0xffffu : s);
            q[wide ? 1 : 0] = (uint16_t)(wide ? w >> 16 : s);
        }
    }
}

// The statement's fp32 steps, spelled with operators HERE, under this file's contract(off): the header's __fmul_rn /
// __fadd_rn are plain operators compiled under the default contraction, and a product and a sum of theirs meet as one
// fused multiply-add once both are inlined.
__device__ __forceinline__ float l_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float l_add(float a, float b) { return a + b; }
__device__ __forceinline__ float l_sub(float a, float b) { return a - b; }
// correctly rounded, both: hipcc's default for the `/` operator and the sqrt builtin (the header's __fsqrt_rn is the
// hardware's approximate square root unless the rounded OCML entry points are asked for)
__device__ __forceinline__ float l_div(float a, float b) { return a / b; }
__device__ __forceinline__ float l_sqrt(float a) { return __builtin_sqrtf(a); }

template <int KIND> __device__ __forceinline__ float l_rho(float x, float eps2) {
    if (KIND == OFASR_LOSS_MSE) return l_mul(x, x);
    if (KIND == OFASR_LOSS_L1) return fabsf(x);
    return l_sqrt(l_add(l_mul(x, x), eps2));
}

template <int KIND> __device__ __forceinline__ float l_drho(float x, float eps2) {
    if (KIND == OFASR_LOSS_MSE) return l_add(x, x);
    if (KIND == OFASR_LOSS_L1) return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f);
    return l_div(x, l_sqrt(l_add(l_mul(x, x), eps2)));
}

// where chunk q lies: the element index of its first element in colour plane 0 and of the last element of that plane.
// cpi: chunks per image.  The caller has clamped q to the last chunk.
__device__ __forceinline__ void l_chunk(long long q, long long cpi, long long plane, long long& at, long long& last,
                                        long long& r0) {
    const long long n = q / cpi;
    r0 = (q - n * cpi) * LC;
    at = n * 3 * plane + r0;
    last = n * 3 * plane + plane - 1;
}

// grid: (P).  part[blockIdx.x] = this workgroup's (sum rho(d), sum rho(e), Y-SSE)
template <int KIND, bool HAS_S, bool VEC>
__global__ void __launch_bounds__(256) sr_loss_fwd_kernel(LOperand O, LOperand T, LOperand S, long long plane, long long cpi,
                                                          long long total, float eps2, LPartial* __restrict__ part) {
    __shared__ double red_a[4], red_b[4];
    __shared__ unsigned long long red_e[4];
    const int t = (int)threadIdx.x;
    double sa = 0.0, sb = 0.0;
    unsigned long long sse = 0;
    for (long long q0 = (long long)blockIdx.x * 256; q0 < total; q0 += (long long)gridDim.x * 256) {
        const bool live = q0 + t < total;
        const long long q = live ? q0 + t : total - 1;
        long long at, last, r0;
        l_chunk(q, cpi, plane, at, last, r0);
        uint32_t po[LC], pt[LC];   // the three quantised colours of a pixel, one byte each
#pragma unroll
        for (int j = 0; j < LC; ++j) po[j] = pt[j] = 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float o[LC], g[LC], s[LC];
            l_load8<VEC>(O, at + k * plane, last + k * plane, o);
            l_load8<VEC>(T, at + k * plane, last + k * plane, g);
            if (HAS_S) l_load8<VEC>(S, at + k * plane, last + k * plane, s);
#pragma unroll
            for (int j = 0; j < LC; ++j) {
                const bool ok = live && r0 + j < plane;
                const float ra = l_rho<KIND>(l_sub(o[j], g[j]), eps2);
                sa += ok ? (double)ra : 0.0;
                if (HAS_S) {
                    const float rb = l_rho<KIND>(l_sub(o[j], s[j]), eps2);
                    sb += ok ? (double)rb : 0.0;
                }
                po[j] |= q_quant(o[j]) << (8 * k);
                pt[j] |= q_quant(g[j]) << (8 * k);
            }
        }
#pragma unroll
        for (int j = 0; j < LC; ++j) {
            const int d = (int)q_luma(po[j] & 0xffu, (po[j] >> 8) & 0xffu, po[j] >> 16) -
                          (int)q_luma(pt[j] & 0xffu, (pt[j] >> 8) & 0xffu, pt[j] >> 16);
            sse += (live && r0 + j < plane) ? (unsigned)(d * d) : 0u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sa += __shfl_xor(sa, o, 64);
        sb += __shfl_xor(sb, o, 64);
        sse += __shfl_xor(sse, o, 64);
    }
    if ((t & 63) == 0) {
        red_a[t >> 6] = sa;
        red_b[t >> 6] = sb;
        red_e[t >> 6] = sse;
    }
    __syncthreads();
    if (t == 0) {
        LPartial p;
        p.sa = ((red_a[0] + red_a[1]) + red_a[2]) + red_a[3];
        p.sb = ((red_b[0] + red_b[1]) + red_b[2]) + red_b[3];
        p.sse = (long long)(red_e[0] + red_e[1] + red_e[2] + red_e[3]);
        p.pad = 0;
        part[blockIdx.x] = p;
    }
}

// grid: (1).  Lane t adds partials t, t + 256, ... in order; the 256 lane totals are then added pairwise in a fixed tree.
__global__ void __launch_bounds__(256) sr_loss_fold_kernel(const LPartial* __restrict__ part, int P, double M, double w_main,
                                                           double w_kd, double count, double* __restrict__ res) {
    __shared__ double ra[256], rb[256];
    __shared__ long long re[256];
    const int t = (int)threadIdx.x;
    double a = 0.0, b = 0.0;
    long long e = 0;
    for (int i = t; i < P; i += 256) {
        a += part[i].sa;
        b += part[i].sb;
        e += part[i].sse;
    }
    ra[t] = a;
    rb[t] = b;
    re[t] = e;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            ra[t] += ra[t + o];
            rb[t] += rb[t + o];
            re[t] += re[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double L = w_main * ra[0] / M + w_kd * rb[0] / M;
        const double mse = (double)re[0] / count;
        res[0] = ra[0];
        res[1] = rb[0];
        res[2] = L;
        reinterpret_cast<long long*>(res)[3] = re[0];
        res[4] = 20.0 * log10(255.0 / sqrt(mse));
        reinterpret_cast<unsigned long long*>(res)[5] = (unsigned long long)__float_as_uint((float)L);
    }
}

// grid: (P).  G: the gradient, in O's format.
template <int KIND, bool HAS_S, bool VEC>
__global__ void __launch_bounds__(256) sr_loss_bwd_kernel(LOperand O, LOperand T, LOperand S, const float* __restrict__ gin,
                                                          float ca, float cb, long long plane, long long cpi, long long total,
                                                          float eps2, void* __restrict__ G) {
    const int t = (int)threadIdx.x;
    const float g = *gin;
    const float ga = l_mul(ca, g), gb = l_mul(cb, g);
    for (long long q0 = (long long)blockIdx.x * 256; q0 < total; q0 += (long long)gridDim.x * 256) {
        const long long q = q0 + t < total ? q0 + t : total - 1;
        long long at, last, r0;
        l_chunk(q, cpi, plane, at, last, r0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float o[LC], h[LC], s[LC], v[LC];
            l_load8<VEC>(O, at + k * plane, last + k * plane, o);
            l_load8<VEC>(T, at + k * plane, last + k * plane, h);
            if (HAS_S) l_load8<VEC>(S, at + k * plane, last + k * plane, s);
#pragma unroll
            for (int j = 0; j < LC; ++j) {
                v[j] = l_mul(ga, l_drho<KIND>(l_sub(o[j], h[j]), eps2));
                if (HAS_S) v[j] = l_add(v[j], l_mul(gb, l_drho<KIND>(l_sub(o[j], s[j]), eps2)));
            }
            l_store8<VEC>(G, O.fmt, at + k * plane, last + k * plane, v);
        }
    }
}

static double l_fmt_bytes(int f) { return (double)elem_bytes(f); }
static bool l_kind_ok(int k) { return k == OFASR_LOSS_MSE || k == OFASR_LOSS_L1 || k == OFASR_LOSS_CHARBONNIER; }

static int l_parts(int64_t elems) {
    const int64_t p = cdiv(elems, 3 * LC * 256);
    return (int)(p < 1 ? 1 : (p > L_MAX_PARTS ? L_MAX_PARTS : p));
}

// 16-byte requests: every tensor of the call at a 16-byte aligned address, H * W % 8 == 0
static bool l_vec(int64_t plane, const void* a, const void* b, const void* c, const void* d) {
    return aligned16(a, b, c, d) && plane % LC == 0;
}

// what the two entry points check alike; 0 when the call may go on
static int l_check(const char* name, const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s, int64_t N,
                   int64_t H, int64_t W, int kind, double eps) {
    OFASR_REQUIRE(o && t, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(is_float_dtype(fmt_o) && is_float_dtype(fmt_t) && (!s || is_float_dtype(fmt_s)), OFASR_ERR_INVALID_ARG,
                  "%s: operands are f32 / f16 / bf16 (formats %d / %d / %d)", name, fmt_o, fmt_t, fmt_s);
    OFASR_REQUIRE(l_kind_ok(kind), OFASR_ERR_INVALID_ARG, "%s: unknown loss kind %d", name, kind);
    OFASR_REQUIRE(N > 0 && H > 0 && W > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(kind != OFASR_LOSS_CHARBONNIER || (eps > 0.0 && eps < INFINITY), OFASR_ERR_INVALID_ARG,
                  "%s: the Charbonnier eps must be positive and finite, got %g", name, eps);
    OFASR_REQUIRE(H <= (1LL << 40) / W && N <= (1LL << 40) / 3 / (H * W), OFASR_ERR_UNSUPPORTED,
                  "%s: more than 2^40 elements", name);
    return OFASR_OK;
}

template <int KIND, bool HAS_S, bool VEC>
static void l_fwd_launch(int P, hipStream_t st, LOperand O, LOperand T, LOperand S, long long plane, long long cpi,
                         long long total, float eps2, LPartial* part) {
    OFASR_LAUNCH((sr_loss_fwd_kernel<KIND, HAS_S, VEC>), dim3((unsigned)P), dim3(256), 0, st, O, T, S, plane, cpi, total, eps2,
                 part);
}
template <int KIND, bool HAS_S, bool VEC>
static void l_bwd_launch(int P, hipStream_t st, LOperand O, LOperand T, LOperand S, const float* g, float ca, float cb,
                         long long plane, long long cpi, long long total, float eps2, void* grad) {
    OFASR_LAUNCH((sr_loss_bwd_kernel<KIND, HAS_S, VEC>), dim3((unsigned)P), dim3(256), 0, st, O, T, S, g, ca, cb, plane, cpi,
                 total, eps2, grad);
}

// ------------------------------------------------------------------------------------------------ the SSIM term
// (ofasr_sr_loss_ssim_fwd / ofasr_sr_loss_ssim_bwd; losses.ssim_np and losses.sr_loss_ssim_grad_np are the host statement;
// DESIGN.md section 3.1s).  Per colour plane, on the fp32 readings of o and t promoted to fp64, no clamp and no
// quantisation: the metric's window (11 taps, sigma 1.5) at the positions where it lies inside the plane.
//
// Tiles of ST x ST, one workgroup of 256 lanes per (plane, tile), tiled as quality_y_tile_kernel is: the pixels under
// the tile go to LDS once as fp32, the horizontal 11-tap pass leaves the five sums G*o, G*t, G*oo, G*tt, G*ot of every
// row in LDS as fp64, and in the vertical pass a lane owns 4 vertically adjacent positions of one column and walks the
// 14 rows under them once.  Forward: a tile is ST x ST positions over (ST + 10)^2 pixels; the SSIM of its valid positions
// is folded in a fixed order into one fp64 partial.  Backward: a tile is ST x ST pixels of the gradient; the positions
// whose window holds one of them are the (ST + 10)^2 from 10 before the tile on, over (ST + 20)^2 pixels; dm, dp, dr are
// formed there (zero where the position is not a valid one), correlated back along W and along H with the taps
// mirrored, the pixel term of sr_loss_bwd_kernel is added and the element is stored once.  Nothing but the forward's
// partials passes through memory.  A pixel outside the plane is never loaded: its slot in LDS is a zero that only
// positions which are masked out read.
constexpr int ST = 16;             // tile edge
constexpr int SW = 11;             // window
constexpr int SR = SW - 1;         // how far a window reaches past its position
constexpr int SF = ST + SR;        // 26: pixels under a forward tile, per side; positions over a backward tile
constexpr int SB = ST + 2 * SR;    // 36: pixels under the positions of a backward tile
constexpr long long S_MAX_TILES = 0x7fffffffLL;

struct SGauss { double g[SW]; };

__device__ __forceinline__ float s_read(const LOperand& a, long long i) {
    if (a.fmt == OFASR_F32) return reinterpret_cast<const float*>(a.p)[i];
    if (a.fmt == OFASR_BF16) return to_float(reinterpret_cast<const bf16_t*>(a.p)[i]);
    return to_float(reinterpret_cast<const f16_t*>(a.p)[i]);
}

// pixels (y0 + r, x0 + c), r and c in [0, E), of the plane that starts at element `base`, into so / st (pitch E + 1);
// zero where the plane has no such pixel -- the load stands under that test
template <int E>
__device__ __forceinline__ void s_stage(const LOperand& O, const LOperand& T, long long base, long long H, long long W,
                                        long long y0, long long x0, float* so, float* st, int t) {
    for (int i = t; i < E * E; i += 256) {
        const int r = i / E, c = i - r * E;
        const long long y = y0 + r, x = x0 + c;
        float a = 0.0f, b = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            a = s_read(O, base + y * W + x);
            b = s_read(T, base + y * W + x);
        }
        so[r * (E + 1) + c] = a;
        st[r * (E + 1) + c] = b;
    }
}

// horizontal pass over E rows: hb[q][r * (E - SR) + c] = sum_k g[k] * f_q(pixel (r, c + k))
template <int E>
__device__ __forceinline__ void s_rows(const float* so, const float* st, double* hb, const SGauss& G, int t) {
    constexpr int PC = E - SR;
    for (int i = t; i < E * PC; i += 256) {
        const int r = i / PC, c = i - r * PC;
        double m1 = 0.0, m2 = 0.0, p = 0.0, q = 0.0, x = 0.0;
#pragma unroll
        for (int k = 0; k < SW; ++k) {
            const double a = (double)so[r * (E + 1) + c + k], b = (double)st[r * (E + 1) + c + k];
            m1 = fma(G.g[k], a, m1);
            m2 = fma(G.g[k], b, m2);
            p = fma(G.g[k], a * a, p);
            q = fma(G.g[k], b * b, q);
            x = fma(G.g[k], a * b, x);
        }
        hb[0 * E * PC + i] = m1;
        hb[1 * E * PC + i] = m2;
        hb[2 * E * PC + i] = p;
        hb[3 * E * PC + i] = q;
        hb[4 * E * PC + i] = x;
    }
}

// vertical pass: the five moments of the positions (r0 + j, c), j = 0 .. 3, from the rows r0 .. r0 + 13 (those below E)
template <int E>
__device__ __forceinline__ void s_cols(const double* hb, const SGauss& G, int r0, int c, double (&acc)[4][5]) {
    constexpr int PC = E - SR;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[j][q] = 0.0;
#pragma unroll
    for (int r = 0; r < 4 + SR; ++r) {
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = r0 + r < E ? hb[q * E * PC + (r0 + r) * PC + c] : 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = r - j;
            if (k >= 0 && k < SW) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[j][q] = fma(G.g[k], v[q], acc[j][q]);
            }
        }
    }
}

struct STerms { double A1, A2, B1, B2; };

__device__ __forceinline__ STerms s_terms(const double (&m)[5]) {
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double m11 = m[0] * m[0], m22 = m[1] * m[1], m12 = m[0] * m[1];
    const double s1 = m[2] - m11, s2 = m[3] - m22, s12 = m[4] - m12;
    return STerms{2.0 * m12 + C1, 2.0 * s12 + C2, m11 + m22 + C1, s1 + s2 + C2};
}

// which (plane, tile row, tile column) workgroup b is
__device__ __forceinline__ void s_tile(long long b, long long ty, long long tx, long long& pl, long long& by, long long& bx) {
    pl = b / (ty * tx);
    const long long r = b - pl * ty * tx;
    by = r / tx;
    bx = r - by * tx;
}

// grid: (3 N tiles_y tiles_x).  part[blockIdx.x] = sum of the SSIM of the tile's valid positions
__global__ void __launch_bounds__(256) sr_ssim_fwd_kernel(LOperand O, LOperand T, long long H, long long W, long long ty,
                                                          long long tx, SGauss G, double* __restrict__ part) {
    __shared__ float so[SF * (SF + 1)], st[SF * (SF + 1)];
    __shared__ double hb[5 * SF * ST];
    __shared__ double red[4];
    const int t = (int)threadIdx.x;
    long long pl, by, bx;
    s_tile(blockIdx.x, ty, tx, pl, by, bx);
    const long long y0 = by * ST, x0 = bx * ST;
    s_stage<SF>(O, T, pl * H * W, H, W, y0, x0, so, st, t);
    __syncthreads();
    s_rows<SF>(so, st, hb, G, t);
    __syncthreads();
    double ssim = 0.0;
    if (t < ST * (ST / 4)) {
        const int c = t % ST, r0 = (t / ST) * 4;
        double acc[4][5];
        s_cols<SF>(hb, G, r0, c, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (y0 + r0 + j < H - SR && x0 + c < W - SR) {
                const STerms s = s_terms(acc[j]);
                ssim += (s.A1 * s.A2) / (s.B1 * s.B2);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ssim += __shfl_xor(ssim, o, 64);
    if ((t & 63) == 0) red[t >> 6] = ssim;
    __syncthreads();
    if (t == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// grid: (1).  sr_loss_fold_kernel with the SSIM partials beside the stream kernel's: lane t adds partials t, t + 256, ...
// in order, the 256 lane totals are added pairwise in a fixed tree.  res[0 .. 7].
__global__ void __launch_bounds__(256) sr_loss_ssim_fold_kernel(const LPartial* __restrict__ part, int P,
                                                                const double* __restrict__ spart, long long tiles, double M,
                                                                double w_main, double w_kd, double count, double alpha,
                                                                double K, double* __restrict__ res) {
    __shared__ double ra[256], rb[256], rs[256];
    __shared__ long long re[256];
    const int t = (int)threadIdx.x;
    double a = 0.0, b = 0.0, s = 0.0;
    long long e = 0;
    for (int i = t; i < P; i += 256) {
        a += part[i].sa;
        b += part[i].sb;
        e += part[i].sse;
    }
    for (long long i = t; i < tiles; i += 256) s += spart[i];
    ra[t] = a;
    rb[t] = b;
    rs[t] = s;
    re[t] = e;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            ra[t] += ra[t + o];
            rb[t] += rb[t + o];
            rs[t] += rs[t + o];
            re[t] += re[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double Lpix = w_main * ra[0] / M + w_kd * rb[0] / M;
        const double S = rs[0] / K;
        const double L = (1.0 - alpha) * Lpix + alpha * (1.0 - S);
        const double mse = (double)re[0] / count;
        res[0] = ra[0];
        res[1] = rb[0];
        res[2] = L;
        reinterpret_cast<long long*>(res)[3] = re[0];
        res[4] = 20.0 * log10(255.0 / sqrt(mse));
        reinterpret_cast<unsigned long long*>(res)[5] = (unsigned long long)__float_as_uint((float)L);
        res[6] = rs[0];
        res[7] = S;
    }
}

// grid: (3 N tiles_y tiles_x), tiles of ST x ST gradient pixels.  G: the gradient, in O's format; every element of it is
// stored once, by the lane that owns the pixel.
template <int KIND, bool HAS_S>
__global__ void __launch_bounds__(256) sr_ssim_bwd_kernel(LOperand O, LOperand T, LOperand S, const float* __restrict__ gin,
                                                          float ca, float cb, double alpha, double K, long long H,
                                                          long long W, long long ty, long long tx, float eps2, SGauss G,
                                                          void* __restrict__ grad) {
    __shared__ float so[SB * (SB + 1)], st[SB * (SB + 1)];
    __shared__ double hb[5 * SB * SF];      // the five row sums; then the three maps correlated back along W
    __shared__ double dmap[3 * SF * SF];    // dm, dp, dr at the positions, zero where the position is not a valid one
    const int t = (int)threadIdx.x;
    long long pl, by, bx;
    s_tile(blockIdx.x, ty, tx, pl, by, bx);
    const long long y0 = by * ST, x0 = bx * ST, base = pl * H * W;
    s_stage<SB>(O, T, base, H, W, y0 - SR, x0 - SR, so, st, t);
    __syncthreads();
    s_rows<SB>(so, st, hb, G, t);
    __syncthreads();

    // ---- the moments of the positions (y0 - 10 + a, x0 - 10 + c), a and c in [0, SF), and the three derivatives
    if (t < SF * ((SF + 3) / 4)) {
        const int c = t % SF, r0 = (t / SF) * 4;
        double acc[4][5];
        s_cols<SB>(hb, G, r0, c, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = r0 + j;
            const long long i = y0 - SR + a, jx = x0 - SR + c;
            double dm = 0.0, dp = 0.0, dr = 0.0;
            if (i >= 0 && i < H - SR && jx >= 0 && jx < W - SR) {
                const STerms s = s_terms(acc[j]);
                const double inv = 1.0 / (s.B1 * s.B2), f = s.A1 * s.A2 * inv;
                dr = 2.0 * s.A1 * inv;
                dp = -f / s.B2;
                dm = 2.0 * acc[j][1] * (s.A2 - s.A1) * inv - 2.0 * acc[j][0] * f * (s.B2 - s.B1) * inv;
            }
            if (a < SF) {
                dmap[0 * SF * SF + a * SF + c] = dm;
                dmap[1 * SF * SF + a * SF + c] = dp;
                dmap[2 * SF * SF + a * SF + c] = dr;
            }
        }
    }
    __syncthreads();

    // ---- back along W: pixel column x0 + xx takes position column x0 - 10 + (xx + k) with tap 10 - k
    for (int i = t; i < SF * ST; i += 256) {
        const int a = i / ST, xx = i - a * ST;
        double u[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SW; ++k) {
#pragma unroll
            for (int q = 0; q < 3; ++q) u[q] = fma(G.g[SR - k], dmap[q * SF * SF + a * SF + xx + k], u[q]);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) hb[q * SF * ST + i] = u[q];
    }
    __syncthreads();

    // ---- back along H, the pixel term, the store: lane = pixel (y0 + yy, x0 + xx)
    const int yy = t / ST, xx = t - yy * ST;
    const long long y = y0 + yy, x = x0 + xx;
    if (y < H && x < W) {
        double u[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < SW; ++k) {
#pragma unroll
            for (int q = 0; q < 3; ++q) u[q] = fma(G.g[SR - k], hb[q * SF * ST + (yy + k) * ST + xx], u[q]);
        }
        const float o = so[(yy + SR) * (SB + 1) + xx + SR], h = st[(yy + SR) * (SB + 1) + xx + SR];
        const double dS = ((u[0] + 2.0 * (double)o * u[1]) + (double)h * u[2]) / K;
        const float g = *gin;
        const float ga = l_mul(ca, g), gb = l_mul(cb, g);
        const long long at = base + y * W + x;
        float v = l_mul(ga, l_drho<KIND>(l_sub(o, h), eps2));
        if (HAS_S) v = l_add(v, l_mul(gb, l_drho<KIND>(l_sub(o, s_read(S, at)), eps2)));
        v = l_add(v, (float)((double)g * -alpha * dS));
        asm volatile("" : "+v"(v));   // final in fp32 before it is narrowed (l_store8)
        if (O.fmt == OFASR_F32) reinterpret_cast<float*>(grad)[at] = v;
        else if (O.fmt == OFASR_BF16) reinterpret_cast<bf16_t*>(grad)[at] = from_float<bf16_t>(v);
        else reinterpret_cast<f16_t*>(grad)[at] = from_float<f16_t>(v);
    }
}

static SGauss s_gauss() {
    SGauss G;
    double sum = 0.0;
    for (int k = 0; k < SW; ++k) sum += (G.g[k] = exp(-(double)((k - SW / 2) * (k - SW / 2)) / (2.0 * 1.5 * 1.5)));
    for (int k = 0; k < SW; ++k) G.g[k] /= sum;
    return G;
}

// forward tiles (over the positions) and backward tiles (over the pixels) of a batch; 0 for a shape the calls refuse
static int64_t s_tiles(int64_t N, int64_t H, int64_t W, bool bwd, int64_t* ty, int64_t* tx) {
    if (N <= 0 || H < SW || W < SW || H > (1LL << 40) / W || N > (1LL << 40) / 3 / (H * W)) return 0;
    *ty = cdiv(bwd ? H : H - SR, ST);
    *tx = cdiv(bwd ? W : W - SR, ST);
    return 3 * N * *ty * *tx;
}

// what the two SSIM entry points check beyond l_check
static int s_check(const char* name, int64_t N, int64_t H, int64_t W, double alpha) {
    OFASR_REQUIRE(alpha > 0.0 && alpha <= 1.0, OFASR_ERR_INVALID_ARG, "%s: alpha must lie in (0, 1], got %g", name, alpha);
    OFASR_REQUIRE(H >= SW && W >= SW, OFASR_ERR_INVALID_ARG, "%s: a %lldx%lld plane has a side below the %d-pixel SSIM window",
                  name, (long long)H, (long long)W, SW);
    int64_t ty = 0, tx = 0;
    OFASR_REQUIRE(s_tiles(N, H, W, true, &ty, &tx) <= S_MAX_TILES, OFASR_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 tiles", name);
    return OFASR_OK;
}

template <int KIND, bool HAS_S>
static void s_bwd_launch(int64_t tiles, hipStream_t st, LOperand O, LOperand T, LOperand S, const float* g, float ca, float cb,
                         double alpha, double K, long long H, long long W, long long ty, long long tx, float eps2,
                         const SGauss& G, void* grad) {
    OFASR_LAUNCH((sr_ssim_bwd_kernel<KIND, HAS_S>), dim3((unsigned)tiles), dim3(256), 0, st, O, T, S, g, ca, cb, alpha, K, H, W,
                 ty, tx, eps2, G, grad);
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT size_t ofasr_sr_loss_workspace(int64_t elems) {
    return elems > 0 ? (size_t)l_parts(elems) * sizeof(LPartial) : 0;
}

OFASR_EXPORT int ofasr_sr_loss_fwd(const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s, int64_t N,
                                   int64_t H, int64_t W, int kind, double eps, double w_main, double w_kd, double psnr_count,
                                   double* result, void* workspace, size_t workspace_bytes, void* stream) {
    const char* name = "ofasr_sr_loss_fwd";
    OFASR_REQUIRE(result, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    const int rc = l_check(name, o, fmt_o, t, fmt_t, s, fmt_s, N, H, W, kind, eps);
    if (rc != OFASR_OK) return rc;
    OFASR_REQUIRE(psnr_count > 0.0, OFASR_ERR_INVALID_ARG, "%s: psnr_count must be positive, got %g", name, psnr_count);
    OFASR_REQUIRE(reinterpret_cast<uintptr_t>(result) % 8 == 0, OFASR_ERR_INVALID_ARG, "%s: result is not 8-byte aligned", name);
    const int64_t plane = H * W, elems = 3 * N * plane;
    const size_t need = ofasr_sr_loss_workspace(elems);
    OFASR_REQUIRE(workspace && workspace_bytes >= need && aligned16(workspace),
                  OFASR_ERR_WORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", name, need,
                  workspace_bytes);
    const int P = l_parts(elems);
    const long long cpi = cdiv(plane, LC), total = N * cpi;
    const float eps2 = (float)(eps * eps);
    const LOperand O{o, fmt_o}, T{t, fmt_t}, S{s, fmt_s};
    const bool vec = l_vec(plane, o, t, s, nullptr);
    hipStream_t st = as_stream(stream);
    prof_note((double)elems * (l_fmt_bytes(fmt_o) + l_fmt_bytes(fmt_t) + (s ? l_fmt_bytes(fmt_s) : 0.0)), 0.0);
    dispatch_int<OFASR_LOSS_MSE, OFASR_LOSS_L1, OFASR_LOSS_CHARBONNIER>(kind, [&](auto K) {
        dispatch_bool(s != nullptr, [&](auto KD) {
            dispatch_bool(vec, [&](auto VEC) {
                l_fwd_launch<K, KD, VEC>(P, st, O, T, S, plane, cpi, total, eps2, (LPartial*)workspace);
            });
        });
    });
    OFASR_LAUNCH(sr_loss_fold_kernel, dim3(1), dim3(256), 0, st, (const LPartial*)workspace, P, (double)elems, w_main, w_kd,
                 psnr_count, result);
    return check_launch(name);
}

OFASR_EXPORT int ofasr_sr_loss_bwd(const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s, const float* g,
                                   int64_t N, int64_t H, int64_t W, int kind, double eps, double w_main, double w_kd, void* grad,
                                   void* stream) {
    const char* name = "ofasr_sr_loss_bwd";
    OFASR_REQUIRE(g && grad, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    const int rc = l_check(name, o, fmt_o, t, fmt_t, s, fmt_s, N, H, W, kind, eps);
    if (rc != OFASR_OK) return rc;
    OFASR_REQUIRE(reinterpret_cast<uintptr_t>(g) % 4 == 0, OFASR_ERR_INVALID_ARG, "%s: g is not 4-byte aligned", name);
    const int64_t plane = H * W, elems = 3 * N * plane;
    const int P = l_parts(elems);
    const long long cpi = cdiv(plane, LC), total = N * cpi;
    const float eps2 = (float)(eps * eps);
    const float ca = (float)(w_main / (double)elems), cb = (float)(w_kd / (double)elems);
    const LOperand O{o, fmt_o}, T{t, fmt_t}, S{s, fmt_s};
    const bool vec = l_vec(plane, o, t, s, grad);
    hipStream_t st = as_stream(stream);
    prof_note((double)elems * (2.0 * l_fmt_bytes(fmt_o) + l_fmt_bytes(fmt_t) + (s ? l_fmt_bytes(fmt_s) : 0.0)), 0.0);
    dispatch_int<OFASR_LOSS_MSE, OFASR_LOSS_L1, OFASR_LOSS_CHARBONNIER>(kind, [&](auto K) {
        dispatch_bool(s != nullptr, [&](auto KD) {
            dispatch_bool(vec, [&](auto VEC) {
                l_bwd_launch<K, KD, VEC>(P, st, O, T, S, g, ca, cb, plane, cpi, total, eps2, grad);
            });
        });
    });
    return check_launch(name);
}

// ---- with the SSIM term: L = (1 - alpha) * L_pix + alpha * (1 - S)
OFASR_EXPORT size_t ofasr_sr_loss_ssim_workspace(int64_t N, int64_t H, int64_t W) {
    int64_t ty = 0, tx = 0;
    const int64_t tiles = s_tiles(N, H, W, false, &ty, &tx);
    if (tiles <= 0 || s_tiles(N, H, W, true, &ty, &tx) > S_MAX_TILES) return 0;
    return ofasr_sr_loss_workspace(3 * N * H * W) + (size_t)tiles * sizeof(double);
}

OFASR_EXPORT int ofasr_sr_loss_ssim_fwd(const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s, int64_t N,
                                        int64_t H, int64_t W, int kind, double eps, double w_main, double w_kd,
                                        double psnr_count, double alpha, double* result, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    const char* name = "ofasr_sr_loss_ssim_fwd";
    OFASR_REQUIRE(result, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    int rc = l_check(name, o, fmt_o, t, fmt_t, s, fmt_s, N, H, W, kind, eps);
    if (rc != OFASR_OK) return rc;
    if ((rc = s_check(name, N, H, W, alpha)) != OFASR_OK) return rc;
    OFASR_REQUIRE(psnr_count > 0.0, OFASR_ERR_INVALID_ARG, "%s: psnr_count must be positive, got %g", name, psnr_count);
    OFASR_REQUIRE(reinterpret_cast<uintptr_t>(result) % 8 == 0, OFASR_ERR_INVALID_ARG, "%s: result is not 8-byte aligned", name);
    const int64_t plane = H * W, elems = 3 * N * plane;
    const size_t need = ofasr_sr_loss_ssim_workspace(N, H, W);
    OFASR_REQUIRE(workspace && workspace_bytes >= need && aligned16(workspace),
                  OFASR_ERR_WORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", name, need,
                  workspace_bytes);
    const int P = l_parts(elems);
    int64_t ty = 0, tx = 0;
    const int64_t tiles = s_tiles(N, H, W, false, &ty, &tx);
    LPartial* part = (LPartial*)workspace;
    double* spart = reinterpret_cast<double*>(part + P);
    const long long cpi = cdiv(plane, LC), total = N * cpi;
    const float eps2 = (float)(eps * eps);
    const LOperand O{o, fmt_o}, T{t, fmt_t}, S{s, fmt_s};
    const bool vec = l_vec(plane, o, t, s, nullptr);
    hipStream_t st = as_stream(stream);
    prof_note((double)elems * (l_fmt_bytes(fmt_o) + l_fmt_bytes(fmt_t) + (s ? l_fmt_bytes(fmt_s) : 0.0)), 0.0);
    dispatch_int<OFASR_LOSS_MSE, OFASR_LOSS_L1, OFASR_LOSS_CHARBONNIER>(kind, [&](auto K) {
        dispatch_bool(s != nullptr, [&](auto KD) {
            dispatch_bool(vec, [&](auto VEC) {
                l_fwd_launch<K, KD, VEC>(P, st, O, T, S, plane, cpi, total, eps2, part);
            });
        });
    });
    prof_note((double)elems * (l_fmt_bytes(fmt_o) + l_fmt_bytes(fmt_t)), 0.0);
    OFASR_LAUNCH(sr_ssim_fwd_kernel, dim3((unsigned)tiles), dim3(256), 0, st, O, T, (long long)H, (long long)W, (long long)ty,
                 (long long)tx, s_gauss(), spart);
    OFASR_LAUNCH(sr_loss_ssim_fold_kernel, dim3(1), dim3(256), 0, st, (const LPartial*)part, P, (const double*)spart,
                 (long long)tiles, (double)elems, w_main, w_kd, psnr_count, alpha,
                 3.0 * (double)N * (double)(H - SR) * (double)(W - SR), result);
    return check_launch(name);
}

OFASR_EXPORT int ofasr_sr_loss_ssim_bwd(const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s,
                                        const float* g, int64_t N, int64_t H, int64_t W, int kind, double eps, double w_main,
                                        double w_kd, double alpha, void* grad, void* stream) {
    const char* name = "ofasr_sr_loss_ssim_bwd";
    OFASR_REQUIRE(g && grad, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    int rc = l_check(name, o, fmt_o, t, fmt_t, s, fmt_s, N, H, W, kind, eps);
    if (rc != OFASR_OK) return rc;
    if ((rc = s_check(name, N, H, W, alpha)) != OFASR_OK) return rc;
    OFASR_REQUIRE(reinterpret_cast<uintptr_t>(g) % 4 == 0, OFASR_ERR_INVALID_ARG, "%s: g is not 4-byte aligned", name);
    const int64_t elems = 3 * N * H * W;
    int64_t ty = 0, tx = 0;
    const int64_t tiles = s_tiles(N, H, W, true, &ty, &tx);
    const float eps2 = (float)(eps * eps);
    const float ca = (float)((1.0 - alpha) * w_main / (double)elems), cb = (float)((1.0 - alpha) * w_kd / (double)elems);
    const LOperand O{o, fmt_o}, T{t, fmt_t}, S{s, fmt_s};
    hipStream_t st = as_stream(stream);
    const SGauss G = s_gauss();
    prof_note((double)elems * (2.0 * l_fmt_bytes(fmt_o) + l_fmt_bytes(fmt_t) + (s ? l_fmt_bytes(fmt_s) : 0.0)), 0.0);
    dispatch_int<OFASR_LOSS_MSE, OFASR_LOSS_L1, OFASR_LOSS_CHARBONNIER>(kind, [&](auto K) {
        dispatch_bool(s != nullptr, [&](auto KD) {
            s_bwd_launch<K, KD>(tiles, st, O, T, S, g, ca, cb, alpha, 3.0 * (double)N * (double)(H - SR) * (double)(W - SR),
                                (long long)H, (long long)W, (long long)ty, (long long)tx, eps2, G, grad);
        });
    });
    return check_launch(name);
}
