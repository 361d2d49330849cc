// launch.h -- what the host-side launch layers of csrc/ share, each stated once.  Host only; ofasr_common.h includes it.
//   dispatch_float / dispatch_16bit    a checked runtime dtype -> f(type_tag<T>), always tested in the order f32, bf16, f16;
//   dispatch_bool / dispatch_int       a runtime bool / small integer -> f(std::integral_constant), so that a ladder of
//                                      template instances is a nest of calls whose template arguments are read from the tags;
//   env_default_on / env_default_off / env_positive_int / env_value   the only readers of the environment;
//   OFASR_REQUIRE_DTYPE / _16BIT / _WORKSPACE, aligned16, elem_bytes, align_up   the operand checks of an entry point.
// The dispatchers return what f returns.  The ORDER of the checks inside an entry point is part of its contract (a call
// that is refused is refused with the same code and message whatever else is wrong with it): the macros are placed, not
// gathered.
#pragma once
#include <stdlib.h>
#include <type_traits>

namespace ofasr {

// ---- runtime value -> template argument ----------------------------------------------------------------------------------
// f(tag) with `typename decltype(tag)::type` = float / bf16_t / f16_t, for a dtype that OFASR_REQUIRE_DTYPE has accepted
template <typename T> struct type_tag { typedef T type; };
template <typename F> inline decltype(auto) dispatch_float(int dtype, F&& f) {
    if (dtype == OFASR_F32) return f(type_tag<float>{});
    if (dtype == OFASR_BF16) return f(type_tag<bf16_t>{});
    return f(type_tag<f16_t>{});
}
// the same for a dtype that OFASR_REQUIRE_16BIT (or a *_supported predicate) has accepted
template <typename F> inline decltype(auto) dispatch_16bit(int dtype, F&& f) {
    if (dtype == OFASR_BF16) return f(type_tag<bf16_t>{});
    return f(type_tag<f16_t>{});
}
// f(std::true_type{}) or f(std::false_type{}): `decltype(tag)::value` (or the tag itself) is a constant expression
template <typename F> inline decltype(auto) dispatch_bool(bool b, F&& f) {
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}
// f(std::integral_constant<int, V>{}) for the V of the list that equals v; the LAST of the list for any other v (the
// `default:` of the switches this replaces), so list the values in the order the checks leave them
template <int V0, int... Vs, typename F> inline decltype(auto) dispatch_int(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) {
        return f(std::integral_constant<int, V0>{});
    } else {
        if (v == V0) return f(std::integral_constant<int, V0>{});
        return dispatch_int<Vs...>(v, f);
    }
}

// ---- environment switches --------------------------------------------------------------------------------------------------
// A switch is read once per process: the call site keeps the value in its own `static const` (or std::atomic initialiser).
// Three meanings and no others: on unless the value starts with '0'; off unless it starts with '1'; a positive integer
// (atoi) or else the default.  env_value is the raw string for the one switch that is a word.
inline const char* env_value(const char* name) { return getenv(name); }
inline bool env_default_on(const char* name) {
    const char* e = env_value(name);
    return !(e && e[0] == '0');
}
inline bool env_default_off(const char* name) {
    const char* e = env_value(name);
    return e && e[0] == '1';
}
inline int env_positive_int(const char* name, int dflt) {
    const char* e = env_value(name);
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : dflt;
}

// ---- operand checks --------------------------------------------------------------------------------------------------------
inline bool is_16bit(int dtype) { return dtype == OFASR_F16 || dtype == OFASR_BF16; }
inline bool is_float_dtype(int dtype) { return dtype == OFASR_F32 || is_16bit(dtype); }
// bytes per element of a checked dtype
inline size_t elem_bytes(int dtype) { return dtype == OFASR_F32 ? 4 : 2; }
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// every pointer on a 16-byte boundary (a null pointer counts as aligned)
template <typename... P> inline bool aligned16(const P*... p) { return ((reinterpret_cast<uintptr_t>(p) | ... | uintptr_t(0)) & 15) == 0; }

}  // namespace ofasr

// In the style of OFASR_REQUIRE, with the entry point's local `name`.
#define OFASR_REQUIRE_DTYPE(dtype) \
    OFASR_REQUIRE(::ofasr::is_float_dtype(dtype), OFASR_ERR_INVALID_ARG, "%s: bad dtype", name)
// `msg`: the entry point's own wording ("16-bit only", "16-bit tensors only", ...)
#define OFASR_REQUIRE_16BIT(dtype, msg) OFASR_REQUIRE(::ofasr::is_16bit(dtype), OFASR_ERR_UNSUPPORTED, "%s: " msg, name)
#define OFASR_REQUIRE_WORKSPACE(ptr, bytes, need)                                                                      \
    OFASR_REQUIRE((ptr) && (bytes) >= (need), OFASR_ERR_WORKSPACE, "%s: workspace %zu B < required %zu B", name,       \
                  (size_t)(bytes), (size_t)(need))
