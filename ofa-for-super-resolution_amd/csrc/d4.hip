// d4.hip -- the 8 flips / transposes of an NCHW batch and their fp32 merge, for geometric self-ensemble inference
// (ofasr_d4_apply / ofasr_d4_accumulate; host statement: upscale.d4_transform / d4_inverse).
//
//   T_t(x) = transpose^{b2}(flip_H^{b1}(flip_W^{b0}(x)))  on the last two axes, b_i = bit i of t
//   apply:       dst = T_t(src)                                                 (a permutation: bit-exact)
//   accumulate:  acc[n,c,y,x] = ((first ? 0 : acc[n,c,y,x]) + float(T_t^{-1}(src)[n,c,y,x])) * scale
// Both are ONE gather over the destination.  With (Hd, Wd) the destination plane, fx / fy a flip of the destination's
// x / y coordinate (xf = fx ? Wd-1-x : x, yf = fy ? Hd-1-y : y):
//   not transposing: dst[y][x] = src[yf][xf],   src plane [Hd][Wd]    apply: fx = b0, fy = b1    accumulate: the same
//   transposing:     dst[y][x] = src[xf][yf],   src plane [Wd][Hd]    apply: fx = b1, fy = b0    accumulate: fx = b0, fy = b1
// (apply: dst = F(src)^T with F the two flips, so dst[y][x] = F(src)[x][y]; accumulate: T^{-1}(z) = F(z^T).)
//
// d4_flip_kernel: a lane owns 4 consecutive destination elements of one row; the source is the mirrored 4-element group of
// the (mirrored) row, read as one vector and reversed inside the lane.  Vector access only when the width is a multiple
// of 4 and both base pointers are aligned for their vectors; otherwise element loads from clamped addresses and
// predicated element stores.
// d4_tr_kernel: 64 x 64 destination tiles through a padded LDS tile (65 words per row: the row-wise write and the
// column-wise read are both conflict-free), so both global sides move row-contiguous 64-element segments per wave.
// Every load is issued from an address clamped into the plane and the value is selected afterwards; no load stands under a
// lane-dependent branch (`first` is uniform), and the accumulate epilogue reads all its accumulator values before it
// stores any (a load behind a predicated store to the same tensor would wait for it).  Addressing is 64-bit across
// planes; inside a plane 32 bits suffice ((H + 64) * (W + 64) < 2^31 is required: the walk includes the rounded-up tile
// extents).  Planes beyond the grid's y extent are walked in a loop, so N * C is not limited by it.
// Plain loads and stores, no atomics: two calls give identical bits.
#include <type_traits>
#include "ofasr_common.h"

namespace ofasr {

template <typename T> __device__ __forceinline__ uint32_t d4_bits(T v) { return (uint32_t)v.v; }
template <> __device__ __forceinline__ uint32_t d4_bits<float>(float v) { return __float_as_uint(v); }
template <typename T> __device__ __forceinline__ T d4_from_bits(uint32_t b) {
    T r;
    r.v = (uint16_t)b;
    return r;
}
template <> __device__ __forceinline__ float d4_from_bits<float>(uint32_t b) { return __uint_as_float(b); }

__device__ __forceinline__ void d4_unpack4(float4 v, float* e) { e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w; }
template <typename T> __device__ __forceinline__ void d4_unpack4(uint2 v, T* e) {
    e[0].v = (uint16_t)(v.x & 0xffffu), e[1].v = (uint16_t)(v.x >> 16);
    e[2].v = (uint16_t)(v.y & 0xffffu), e[3].v = (uint16_t)(v.y >> 16);
}
__device__ __forceinline__ float4 d4_pack4(const float* e) { return make_float4(e[0], e[1], e[2], e[3]); }
template <typename T> __device__ __forceinline__ uint2 d4_pack4(const T* e) {
    return make_uint2((uint32_t)e[0].v | (uint32_t)e[1].v << 16, (uint32_t)e[2].v | (uint32_t)e[3].v << 16);
}

// one merged value: ((first ? nothing : a) + v) * scale, fp32 adds in the caller's order
__device__ __forceinline__ float d4_merge(float a, float v, int first, float scale) {
    return __fmul_rn(first ? v : __fadd_rn(a, v), scale);
}

// grid: (x: lanes over Hd * ceil(Wd / 4) in a grid-stride loop, y: planes in a grid-stride loop)
template <typename T, bool ACC, bool VEC>
__global__ void __launch_bounds__(256) d4_flip_kernel(const T* __restrict__ src, void* __restrict__ dstv, long long planes,
                                                      int Hd, int Wd, int fx, int fy, int first, float scale) {
    typedef typename std::conditional<ACC, float, T>::type D;
    typedef typename vec4<T>::type SV;
    D* dst = reinterpret_cast<D*>(dstv);
    const unsigned gw = ((unsigned)Wd + 3u) >> 2;
    const unsigned per = (unsigned)Hd * gw;
    const long long plane = (long long)Hd * Wd;
    for (long long p = blockIdx.y; p < planes; p += gridDim.y) {
        const T* sp = src + p * plane;
        D* dp = dst + p * plane;
        for (unsigned e = blockIdx.x * 256u + threadIdx.x; e < per; e += gridDim.x * 256u) {
            const int r = (int)(e / gw);
            const int x0 = (int)(e - (unsigned)r * gw) * 4;
            const long long srow = (long long)(fy ? Hd - 1 - r : r) * Wd;
            const long long drow = (long long)r * Wd;
            T v[4];
            if (VEC) {
                T u[4];
                d4_unpack4(*reinterpret_cast<const SV*>(sp + srow + (fx ? Wd - 4 - x0 : x0)), u);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = fx ? u[3 - j] : u[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = x0 + j < Wd ? x0 + j : Wd - 1;
                    v[j] = sp[srow + (fx ? Wd - 1 - x : x)];
                }
            }
            if (ACC) {
                float a[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
                float* ap = reinterpret_cast<float*>(dp) + drow;
                if (!first) {
                    if (VEC) {
                        d4_unpack4(*reinterpret_cast<const float4*>(ap + x0), a);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) a[j] = ap[x0 + j < Wd ? x0 + j : Wd - 1];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = d4_merge(a[j], to_float(v[j]), first, scale);
                if (VEC) {
                    *reinterpret_cast<float4*>(ap + x0) = d4_pack4(o);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x0 + j < Wd) ap[x0 + j] = o[j];
                }
            } else {
                T* tp = reinterpret_cast<T*>(dp) + drow;
                if (VEC) {
                    *reinterpret_cast<SV*>(tp + x0) = d4_pack4(v);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x0 + j < Wd) tp[x0 + j] = v[j];
                }
            }
        }
    }
}

constexpr int D4_TILE = 64;

// grid: (x: 64 x 64 destination tiles in a grid-stride loop, y: planes in a grid-stride loop); 4 waves, a wave per tile row
template <typename T, bool ACC>
__global__ void __launch_bounds__(256) d4_tr_kernel(const T* __restrict__ src, void* __restrict__ dstv, long long planes,
                                                    int Hd, int Wd, int fx, int fy, int first, float scale) {
    typedef typename std::conditional<ACC, float, T>::type D;
    __shared__ uint32_t tile[D4_TILE][D4_TILE + 1];
    D* dst = reinterpret_cast<D*>(dstv);
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const unsigned tx = ((unsigned)Wd + D4_TILE - 1) / D4_TILE, ty = ((unsigned)Hd + D4_TILE - 1) / D4_TILE;
    const unsigned tiles = tx * ty;
    const long long plane = (long long)Hd * Wd;
    for (long long p = blockIdx.y; p < planes; p += gridDim.y) {
        const T* sp = src + p * plane;     // the source plane is [Wd][Hd]
        D* dp = dst + p * plane;
        for (unsigned t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int ty0 = (int)(t / tx) * D4_TILE, tx0 = (int)(t % tx) * D4_TILE;
            {
                // tile[j][i] = dst value of (y = ty0 + i, x = tx0 + j): lanes run along a source row
                const int y = ty0 + lane < Hd ? ty0 + lane : Hd - 1;
                const int sc = fy ? Hd - 1 - y : y;
#pragma unroll
                for (int k = 0; k < D4_TILE / 4; ++k) {
                    const int j = wv + 4 * k;
                    const int x = tx0 + j < Wd ? tx0 + j : Wd - 1;
                    const int sr = fx ? Wd - 1 - x : x;
                    tile[j][lane] = d4_bits<T>(sp[(long long)sr * Hd + sc]);
                }
            }
            __syncthreads();
            {
                // lane -> x = tx0 + lane, row j -> y = ty0 + j.  The accumulator values are all read first (from clamped
                // addresses, the 16 loads in flight together), then merged, then stored: a load issued after a predicated
                // store to the same tensor would wait for that store, 16 round trips in a row.  A full tile stores
                // straight-line; only an edge tile predicates.
                constexpr int R = D4_TILE / 4;
                const int x = tx0 + lane;
                const int xc = x < Wd ? x : Wd - 1;
                const bool full = tx0 + D4_TILE <= Wd && ty0 + D4_TILE <= Hd;      // uniform over the workgroup
                long long off[R];
                float o[R];
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    const int y = ty0 + wv + 4 * k;
                    off[k] = (long long)(y < Hd ? y : Hd - 1) * Wd + xc;
                }
                if (ACC) {
                    float* ap = reinterpret_cast<float*>(dp);
                    float a[R];
#pragma unroll
                    for (int k = 0; k < R; ++k) a[k] = 0.f;
                    if (!first) {
#pragma unroll
                        for (int k = 0; k < R; ++k) a[k] = ap[off[k]];
                    }
#pragma unroll
                    for (int k = 0; k < R; ++k)
                        o[k] = d4_merge(a[k], to_float(d4_from_bits<T>(tile[lane][wv + 4 * k])), first, scale);
                    if (full) {
#pragma unroll
                        for (int k = 0; k < R; ++k) ap[off[k]] = o[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < R; ++k)
                            if (x < Wd && ty0 + wv + 4 * k < Hd) ap[off[k]] = o[k];
                    }
                } else {
                    T* tp = reinterpret_cast<T*>(dp);
                    if (full) {
#pragma unroll
                        for (int k = 0; k < R; ++k) tp[off[k]] = d4_from_bits<T>(tile[lane][wv + 4 * k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < R; ++k)
                            if (x < Wd && ty0 + wv + 4 * k < Hd) tp[off[k]] = d4_from_bits<T>(tile[lane][wv + 4 * k]);
                    }
                }
            }
            __syncthreads();
        }
    }
}

static unsigned d4_cap(long long v, long long cap) { return (unsigned)(v < 1 ? 1 : (v > cap ? cap : v)); }

// dst plane [Hd][Wd]; see the header for fx / fy
template <typename T, bool ACC>
static void d4_launch(const void* src, void* dst, int64_t planes, int64_t Hd, int64_t Wd, int tr, int fx, int fy, int first,
                      float scale, hipStream_t st) {
    const double elems = (double)planes * (double)Hd * (double)Wd;
    prof_note(ACC ? elems * (sizeof(T) + (first ? 4.0 : 8.0)) : elems * 2.0 * sizeof(T), 0.0);
    const unsigned gy = d4_cap(planes, 65535);
    if (tr) {
        const dim3 grid(d4_cap(cdiv(Hd, D4_TILE) * cdiv(Wd, D4_TILE), 65535), gy);
        OFASR_LAUNCH((d4_tr_kernel<T, ACC>), grid, dim3(256), 0, st, (const T*)src, dst, (long long)planes, (int)Hd, (int)Wd,
                     fx, fy, first, scale);
        return;
    }
    const size_t sal = 4 * sizeof(T), dal = ACC ? 16 : 4 * sizeof(T);
    const bool vec = Wd % 4 == 0 && reinterpret_cast<uintptr_t>(src) % sal == 0 && reinterpret_cast<uintptr_t>(dst) % dal == 0;
    const dim3 grid(d4_cap(cdiv(Hd * cdiv(Wd, 4), 256), 4096), gy);
    dispatch_bool(vec, [&](auto VEC) {
        OFASR_LAUNCH((d4_flip_kernel<T, ACC, VEC>), grid, dim3(256), 0, st, (const T*)src, dst, (long long)planes, (int)Hd,
                     (int)Wd, fx, fy, first, scale);
    });
}

template <bool ACC>
static void d4_dispatch(const void* src, void* dst, int64_t planes, int64_t Hd, int64_t Wd, int tr, int fx, int fy, int first,
                        float scale, int dtype, hipStream_t st) {
    dispatch_float(dtype, [&](auto t) {
        d4_launch<typename decltype(t)::type, ACC>(src, dst, planes, Hd, Wd, tr, fx, fy, first, scale, st);
    });
}

static int d4_check(const char* name, const void* src, const void* dst, int64_t N, int64_t C, int64_t H, int64_t W, int t,
                    int dtype) {
    OFASR_REQUIRE(src && dst, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(src != dst, OFASR_ERR_INVALID_ARG, "%s: source and destination are the same buffer", name);
    OFASR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE(t >= 0 && t < 8, OFASR_ERR_INVALID_ARG, "%s: transform %d outside 0..7", name, t);
    OFASR_REQUIRE_DTYPE(dtype);
    // 32-bit walk inside a plane (the rounded-up extents included), 64-bit across planes
    OFASR_REQUIRE(H < (1LL << 30) && W < (1LL << 30) && (H + 64) * (W + 64) < (1LL << 31), OFASR_ERR_UNSUPPORTED,
                  "%s: a %lldx%lld plane is too large", name, (long long)H, (long long)W);
    OFASR_REQUIRE(N <= (1LL << 40) / C && N * C <= (1LL << 40) / (H * W), OFASR_ERR_UNSUPPORTED, "%s: tensor too large",
                  name);
    return OFASR_OK;
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int ofasr_d4_apply(const void* src, void* dst, int64_t N, int64_t C, int64_t H, int64_t W, int t, int dtype,
                                void* stream) {
    const char* name = "ofasr_d4_apply";
    const int rc = d4_check(name, src, dst, N, C, H, W, t, dtype);
    if (rc != OFASR_OK) return rc;
    const int b0 = t & 1, b1 = (t >> 1) & 1, tr = (t >> 2) & 1;
    if (tr) d4_dispatch<false>(src, dst, N * C, W, H, 1, b1, b0, 1, 1.0f, dtype, as_stream(stream));
    else d4_dispatch<false>(src, dst, N * C, H, W, 0, b0, b1, 1, 1.0f, dtype, as_stream(stream));
    return check_launch(name);
}

OFASR_EXPORT int ofasr_d4_accumulate(const void* src, float* acc, int64_t N, int64_t C, int64_t H, int64_t W, int t,
                                     int dtype, int first, float scale, void* stream) {
    const char* name = "ofasr_d4_accumulate";
    const int rc = d4_check(name, src, acc, N, C, H, W, t, dtype);
    if (rc != OFASR_OK) return rc;
    OFASR_REQUIRE(reinterpret_cast<uintptr_t>(acc) % 4 == 0, OFASR_ERR_INVALID_ARG, "%s: acc is not 4-byte aligned", name);
    const int b0 = t & 1, b1 = (t >> 1) & 1, tr = (t >> 2) & 1;
    d4_dispatch<true>(src, acc, N * C, H, W, tr, b0, b1, first ? 1 : 0, scale, dtype, as_stream(stream));
    return check_launch(name);
}
