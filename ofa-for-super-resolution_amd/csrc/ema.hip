// ema.hip -- the weight average of training as ONE launch over every parameter tensor (ofasr_ema_update) and the exchange
// of the parameters with their average (ofasr_ema_swap).  The host statement is ema.py (update_np):
//     e' = e + float32(w * float32(p - e))         three fp32 operations, each rounded once, never contracted
// table [rows, 3] int64 in GPU memory: {parameter address, shadow address, count}, 1 <= count <= EMA_CHUNK; a row never
// spans two tensors (ema.plan_chunks).  One workgroup per row.  A row takes the 16-byte path when BOTH of its addresses
// are 16-byte aligned and the element path otherwise (uniform per row: the choice is made from the row's own words);
// the tail of a row whose count is no multiple of 4 is element-wise.  A lane walks at most EMA_CHUNK / 4 / 256 vectors;
// the kernel is HBM-bound at a few waves per row, and the rows in flight on a CU are what hides the latency.  update
// reads p and e and writes e; swap writes both.  The host
// cannot see the counts, so the kernel clamps them to [0, EMA_CHUNK] and no launch carries algorithmic bytes (ops.py
// states them from the caller's element count).
#include <math.h>

#include "ofasr_common.h"

#pragma clang fp contract(off)   // every fp32 step of the statement is its own rounding

namespace ofasr {

constexpr int EMA_THREADS = 256;
constexpr int EMA_CHUNK = 4096;                              // elements per table row: 16 KiB per operand
static_assert(EMA_CHUNK % (4 * EMA_THREADS) == 0, "a row is a whole number of vectors per lane");

// The three steps spelled with operators HERE, under this file's contract(off): the header's __fmul_rn / __fadd_rn are
// plain operators compiled under the default contraction, and a product and a sum of theirs meet as one fused
// multiply-add once both are inlined (csrc/loss.hip has the same note).
__device__ __forceinline__ float ema1(float p, float e, float w) {
    const float d = p - e;
    const float m = w * d;
    return e + m;
}
__device__ __forceinline__ float4 ema4(float4 p, float4 e, float w) {
    return make_float4(ema1(p.x, e.x, w), ema1(p.y, e.y, w), ema1(p.z, e.z, w), ema1(p.w, e.w, w));
}

// grid: one workgroup per table row
template <bool SWAP> __global__ void __launch_bounds__(EMA_THREADS) ema_kernel(const long long* table, float w) {
    const long long* row = table + 3 * (long long)blockIdx.x;
    const long long pa = row[0], ea = row[1], cnt = row[2];
    float* p = reinterpret_cast<float*>(pa);
    float* e = reinterpret_cast<float*>(ea);
    const int n = cnt < 0 ? 0 : (cnt > EMA_CHUNK ? EMA_CHUNK : (int)cnt);
    const int tid = threadIdx.x;
    int done = 0;                                            // elements of the row that the vector path covers
    if (((pa | ea) & 15) == 0) {
        const int n4 = n >> 2;
        float4* p4 = reinterpret_cast<float4*>(p);
        float4* e4 = reinterpret_cast<float4*>(e);
        for (int g = tid; g < n4; g += EMA_THREADS) {
            const float4 pv = p4[g], ev = e4[g];
            if (SWAP)
                p4[g] = ev, e4[g] = pv;
            else
                e4[g] = ema4(pv, ev, w);
        }
        done = n4 << 2;
    }
    for (int i = done + tid; i < n; i += EMA_THREADS) {
        const float pv = p[i], ev = e[i];
        if (SWAP)
            p[i] = ev, e[i] = pv;
        else
            e[i] = ema1(pv, ev, w);
    }
}

static int ema_check(const char* name, const int64_t* table, int64_t rows) {
    OFASR_REQUIRE(rows >= 0, OFASR_ERR_INVALID_ARG, "%s: negative row count", name);
    OFASR_REQUIRE(table || rows == 0, OFASR_ERR_INVALID_ARG, "%s: null table", name);
    OFASR_REQUIRE(rows <= (1LL << 30), OFASR_ERR_UNSUPPORTED, "%s: table too large", name);
    return OFASR_OK;
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int64_t ofasr_ema_chunk(void) { return EMA_CHUNK; }

OFASR_EXPORT int ofasr_ema_update(const int64_t* table, int64_t rows, float w, void* stream) {
    const char* name = "ofasr_ema_update";
    const int rc = ema_check(name, table, rows);
    if (rc != OFASR_OK) return rc;
    OFASR_REQUIRE(isfinite(w) && w >= 0.0f && w <= 1.0f, OFASR_ERR_INVALID_ARG, "%s: weight outside [0, 1]", name);
    if (rows == 0) return OFASR_OK;
    OFASR_LAUNCH((ema_kernel<false>), dim3((unsigned)rows), dim3(EMA_THREADS), 0, as_stream(stream),
                 reinterpret_cast<const long long*>(table), w);
    return check_launch(name);
}

OFASR_EXPORT int ofasr_ema_swap(const int64_t* table, int64_t rows, void* stream) {
    const char* name = "ofasr_ema_swap";
    const int rc = ema_check(name, table, rows);
    if (rc != OFASR_OK) return rc;
    if (rows == 0) return OFASR_OK;
    OFASR_LAUNCH((ema_kernel<true>), dim3((unsigned)rows), dim3(EMA_THREADS), 0, as_stream(stream),
                 reinterpret_cast<const long long*>(table), 0.0f);
    return check_launch(name);
}
