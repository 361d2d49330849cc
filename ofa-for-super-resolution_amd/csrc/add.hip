// add.hip -- y = a + b over two equally shaped activations (ofasr_add): the long skip connection of the static SR
// networks at inference time, so that an eval-mode forward runs no ATen arithmetic kernel.  The add is fp32 with one RNE
// cast to the 16-bit types on store -- bit for bit what `a + b` gives.  A lane owns 4 consecutive elements (one vector
// per operand when all three pointers are aligned for it, element accesses from clamped addresses otherwise);
// 64-bit indexing; y may be a or b.
#include "ofasr_common.h"

namespace ofasr {

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
    return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}
template <typename T> __device__ __forceinline__ uint2 add4(uint2 a, uint2 b) {
    float a0, a1, a2, a3, b0, b1, b2, b3;
    unpack2<T>(a.x, a0, a1), unpack2<T>(a.y, a2, a3), unpack2<T>(b.x, b0, b1), unpack2<T>(b.y, b2, b3);
    return make_uint2(pack2<T>(__fadd_rn(a0, b0), __fadd_rn(a1, b1)), pack2<T>(__fadd_rn(a2, b2), __fadd_rn(a3, b3)));
}
template <typename T> __device__ __forceinline__ typename vec4<T>::type add_vec(typename vec4<T>::type a, typename vec4<T>::type b);
template <> __device__ __forceinline__ float4 add_vec<float>(float4 a, float4 b) { return add4(a, b); }
template <> __device__ __forceinline__ uint2 add_vec<bf16_t>(uint2 a, uint2 b) { return add4<bf16_t>(a, b); }
template <> __device__ __forceinline__ uint2 add_vec<f16_t>(uint2 a, uint2 b) { return add4<f16_t>(a, b); }

// grid: lanes over ceil(n / 4) groups in a grid-stride loop
template <typename T, bool VEC>
__global__ void __launch_bounds__(256) add_kernel(const T* a, const T* b, T* y, long long n) {
    typedef typename vec4<T>::type V;
    const long long groups = (n + 3) >> 2;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const long long i = g * 4;
        if (VEC && i + 4 <= n) {
            *reinterpret_cast<V*>(y + i) = add_vec<T>(*reinterpret_cast<const V*>(a + i), *reinterpret_cast<const V*>(b + i));
        } else {
            float s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long k = i + j < n ? i + j : n - 1;
                s[j] = __fadd_rn(to_float(a[k]), to_float(b[k]));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i + j < n) y[i + j] = from_float<T>(s[j]);
        }
    }
}

template <typename T> static void add_launch(const void* a, const void* b, void* y, int64_t n, hipStream_t st) {
    const uintptr_t al = 4 * sizeof(T);
    const bool vec = reinterpret_cast<uintptr_t>(a) % al == 0 && reinterpret_cast<uintptr_t>(b) % al == 0 &&
                     reinterpret_cast<uintptr_t>(y) % al == 0;
    const int64_t blocks = cdiv(cdiv(n, 4), 256);
    const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks)));
    prof_note(3.0 * (double)n * sizeof(T), (double)n);
    dispatch_bool(vec, [&](auto VEC) {
        OFASR_LAUNCH((add_kernel<T, VEC>), grid, dim3(256), 0, st, (const T*)a, (const T*)b, (T*)y, (long long)n);
    });
}

}  // namespace ofasr

using namespace ofasr;

OFASR_EXPORT int ofasr_add(const void* a, const void* b, void* y, int64_t n, int dtype, void* stream) {
    const char* name = "ofasr_add";
    OFASR_REQUIRE(a && b && y, OFASR_ERR_INVALID_ARG, "%s: null pointer", name);
    OFASR_REQUIRE(n > 0, OFASR_ERR_INVALID_ARG, "%s: non-positive size", name);
    OFASR_REQUIRE_DTYPE(dtype);
    OFASR_REQUIRE(n <= (1LL << 40), OFASR_ERR_UNSUPPORTED, "%s: tensor too large", name);
    hipStream_t st = as_stream(stream);
    dispatch_float(dtype, [&](auto t) { add_launch<typename decltype(t)::type>(a, b, y, n, st); });
    return check_launch(name);
}
