// yuv_block.h -- what the kernels that read or write planar YUV 4:2:0 frames share: the sample types of a plane,
// the 14-bit coefficient structs and their checks, the decode of one pixel from its luma and four chroma taps, and the
// encode + store of one 2 x 4 pixel block.  yuv.hip (the whole-frame conversions and the tile moves), resize_scatter.hip
// (the resampling scatter), augment.hip (the training gather) and reuse.hip (the frame checks) include it, so there is
// one statement of the decode and one of the encode.  The table rules and quant<MAXV> are tile_table.h's.
#pragma once
#include "tile_table.h"
#include <initializer_list>

namespace ofasr {

struct YuvDec { int yo, cy, rv, gu, gv, bu; };
struct YuvEnc { int yo, yr, yg, yb, ur, ug, ub, vr, vg, vb; };

// the sample type of a plane: its largest value, the chroma midpoint, how a stored sample is read, and the wide accesses
// (four luma samples of a row, two chroma samples), which the callers take at addresses aligned for them only
template <typename P> struct yuv_px;
template <> struct yuv_px<uint8_t> {
    static constexpr int maxv = 255, mid = 128;
    static __device__ __forceinline__ int sample(uint8_t s) { return s; }
    static __device__ __forceinline__ void load4(const uint8_t* p, int* o) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (int)((w >> (8 * k)) & 0xffu);
    }
    static __device__ __forceinline__ void store4(uint8_t* p, const int* Y) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)Y[0] | (uint32_t)Y[1] << 8 | (uint32_t)Y[2] << 16 | (uint32_t)Y[3] << 24;
    }
    static __device__ __forceinline__ void store2(uint8_t* p, int a, int b) { *reinterpret_cast<uint16_t*>(p) = (uint16_t)(a | b << 8); }
};
template <> struct yuv_px<uint16_t> {
    static constexpr int maxv = 1023, mid = 512;
    static __device__ __forceinline__ int sample(unsigned s) { return (int)(s < 1023u ? s : 1023u); }   // the top six bits are not trusted
    static __device__ __forceinline__ void load4(const uint16_t* p, int* o) {
        const uint2 w = *reinterpret_cast<const uint2*>(p);
        o[0] = sample(w.x & 0xffffu), o[1] = sample(w.x >> 16), o[2] = sample(w.y & 0xffffu), o[3] = sample(w.y >> 16);
    }
    static __device__ __forceinline__ void store4(uint16_t* p, const int* Y) {
        *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)Y[0] | (uint32_t)Y[1] << 16, (uint32_t)Y[2] | (uint32_t)Y[3] << 16);
    }
    static __device__ __forceinline__ void store2(uint16_t* p, int a, int b) { *reinterpret_cast<uint32_t*>(p) = (uint32_t)a | (uint32_t)b << 16; }
};

template <typename P> __device__ __forceinline__ int yuv_clampv(int v) { return v < 0 ? 0 : (v > yuv_px<P>::maxv ? yuv_px<P>::maxv : v); }

// RGB of one pixel from its luma sample and the four chroma taps of each plane in 9-3-3-1 order: the sample the pixel lies
// in, its neighbour in the row, its neighbour in the column, the diagonal one (yuv.hip's header states the siting)
template <typename P>
__device__ __forceinline__ void yuv_decode_px(const YuvDec& D, int Y, const int (&U)[4], const int (&V)[4], int (&rgb)[3]) {
    const int u = ((9 * U[0] + 3 * U[1] + 3 * U[2] + U[3] + 8) >> 4) - yuv_px<P>::mid;
    const int v = ((9 * V[0] + 3 * V[1] + 3 * V[2] + V[3] + 8) >> 4) - yuv_px<P>::mid;
    const int l = D.cy * (Y - D.yo) + (1 << 13);
    rgb[0] = yuv_clampv<P>((l + D.rv * v) >> 14);
    rgb[1] = yuv_clampv<P>((l + D.gu * u + D.gv * v) >> 14);
    rgb[2] = yuv_clampv<P>((l + D.bu * u) >> 14);
}

// RGB of the 2 x 4 block whose corner is the even frame position (by, bx): rgb[row][col][c].  Columns at or past W
// repeat column W - 1 (the caller masks them); by + 1 < H since H is even.
template <typename P>
__device__ __forceinline__ void yuv_decode_block(const P* __restrict__ yp, const P* __restrict__ up, const P* __restrict__ vp,
                                                 long long H, long long W, long long by, long long bx, const YuvDec& D,
                                                 int (&rgb)[2][4][3]) {
    typedef yuv_px<P> px;
    const long long CH = H >> 1, CW = W >> 1;
    const long long cy = by >> 1, cx = bx >> 1;
    long long rows[3], cols[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) rows[i] = clampll(cy - 1 + i, 0, CH - 1) * CW;
#pragma unroll
    for (int j = 0; j < 4; ++j) cols[j] = clampll(cx - 1 + j, 0, CW - 1);
    int cu[3][4], cv[3][4];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            cu[i][j] = px::sample(up[rows[i] + cols[j]]);
            cv[i][j] = px::sample(vp[rows[i] + cols[j]]);
        }
    int Y[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const P* p = yp + (by + r) * W + bx;
        if ((reinterpret_cast<uintptr_t>(p) & (4 * sizeof(P) - 1)) == 0 && bx + 4 <= W) {
            px::load4(p, Y[r]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) Y[r][k] = px::sample(p[bx + k < W ? k : (int)(W - 1 - bx)]);
        }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int nr = r == 0 ? 0 : 2;                   // the other chroma row: above for the even row, below for the odd
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c0 = 1 + (k >> 1);
            const int nc = (k & 1) ? c0 + 1 : c0 - 1;    // left for the even column, right for the odd
            const int tu[4] = {cu[1][c0], cu[1][nc], cu[nr][c0], cu[nr][nc]};
            const int tv[4] = {cv[1][c0], cv[1][nc], cv[nr][c0], cv[nr][nc]};
            yuv_decode_px<P>(D, Y[r][k], tu, tv, rgb[r][k]);
        }
    }
}

// luma of the 2 x 4 block rgb (columns < valid, valid = 2 or 4) and its one or two chroma pairs
template <typename P>
__device__ __forceinline__ void yuv_encode_block(const int (&rgb)[2][4][3], const YuvEnc& E, int (&Y)[2][4], int (&U)[2],
                                                 int (&V)[2]) {
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            Y[r][k] = yuv_clampv<P>(((E.yr * rgb[r][k][0] + E.yg * rgb[r][k][1] + E.yb * rgb[r][k][2] + (1 << 13)) >> 14) + E.yo);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int su = 0, sv = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 2 * j; k < 2 * j + 2; ++k) {
                su += E.ur * rgb[r][k][0] + E.ug * rgb[r][k][1] + E.ub * rgb[r][k][2];
                sv += E.vr * rgb[r][k][0] + E.vg * rgb[r][k][1] + E.vb * rgb[r][k][2];
            }
        U[j] = yuv_clampv<P>(((su + (1 << 15)) >> 16) + yuv_px<P>::mid);
        V[j] = yuv_clampv<P>(((sv + (1 << 15)) >> 16) + yuv_px<P>::mid);
    }
}

// the planes' samples of one encoded block at the even position (by, bx) of an [OH, OW] frame; valid = 2 or 4 columns
template <typename P>
__device__ __forceinline__ void yuv_store_block(P* __restrict__ yp, P* __restrict__ up, P* __restrict__ vp, long long OW,
                                                long long by, long long bx, int valid, const int (&Y)[2][4], const int (&U)[2],
                                                const int (&V)[2]) {
    typedef yuv_px<P> px;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        P* p = yp + (by + r) * OW + bx;
        if ((reinterpret_cast<uintptr_t>(p) & (4 * sizeof(P) - 1)) == 0 && valid == 4) {
            px::store4(p, Y[r]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < valid) p[k] = (P)Y[r][k];
        }
    }
    const long long co = (by >> 1) * (OW >> 1) + (bx >> 1);
    P* pu = up + co;
    P* pv = vp + co;
    if ((reinterpret_cast<uintptr_t>(pu) & (2 * sizeof(P) - 1)) == 0 && valid == 4) px::store2(pu, U[0], U[1]);
    else {
        pu[0] = (P)U[0];
        if (valid == 4) pu[1] = (P)U[1];
    }
    if ((reinterpret_cast<uintptr_t>(pv) & (2 * sizeof(P) - 1)) == 0 && valid == 4) px::store2(pv, V[0], V[1]);
    else {
        pv[0] = (P)V[0];
        if (valid == 4) pv[1] = (P)V[1];
    }
}

// the plane pointers of a 16-bit frame are aligned for their samples
inline bool yuv_planes_aligned2(std::initializer_list<const void*> planes) {
    uintptr_t bits = 0;
    for (const void* p : planes) bits |= reinterpret_cast<uintptr_t>(p);
    return (bits & 1) == 0;
}

static YuvDec yuv_dec(const int32_t* c) { return YuvDec{c[0], c[1], c[2], c[3], c[4], c[5]}; }
static YuvEnc yuv_enc(const int32_t* c) { return YuvEnc{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]}; }

// the 14-bit tables of every matrix / range stay below these bounds, which keep each sum below 2^24 (2^26 for the
// four-pixel chroma sum): int32 cannot overflow whatever the caller passes
static bool yuv_coeffs_ok(const int32_t* c, int n) {
    if (c[0] < 0 || c[0] > 255) return false;
    for (int i = 1; i < n; ++i)
        if (c[i] < -(1 << 16) || c[i] > (1 << 16)) return false;
    return true;
}

}  // namespace ofasr

#define YUV_REQUIRE_FRAME(H, W)                                                                                          \
    OFASR_REQUIRE((H) >= 2 && (W) >= 2, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);                          \
    OFASR_REQUIRE((H) % 2 == 0 && (W) % 2 == 0, OFASR_ERR_INVALID_ARG, "%s: a 4:2:0 frame needs even sides, got %lldx%lld", \
                  name, (long long)(H), (long long)(W));                                                                 \
    TILE_REQUIRE_FRAME_CAP(H, W)

// 16-bit planes: the one depth this library defines, and plane pointers (any number) aligned for their samples
#define YUV_REQUIRE_P16(depth, ...)                                                                                      \
    OFASR_REQUIRE((depth) == 10, OFASR_ERR_INVALID_ARG, "%s: depth %d is not supported (10 only)", name, (int)(depth));  \
    OFASR_REQUIRE(ofasr::yuv_planes_aligned2({__VA_ARGS__}), OFASR_ERR_INVALID_ARG,                                      \
                  "%s: a 16-bit plane pointer is not 2-byte aligned", name)
