// quality_math.h -- the two per-pixel rules of the Y-channel metric, stated once for quality.hip (ofasr_quality_y) and
// loss.hip (the Y-SSE the training loss logs).  Host statement: utils._quantise_u8 and utils.y_exact.
#pragma once
#include "ofasr_common.h"

namespace ofasr {

// float -> uint8 as utils.tensor2img_np / tile_io.hip do: clamp to [0, 1], * 255 in fp32, round half to even
__device__ __forceinline__ uint32_t q_quant(float v) {
    const float f = fminf(fmaxf(v, 0.0f), 1.0f);
    return (uint32_t)rintf(__fmul_rn(f, 255.0f));
}

// Y = round_half_even((65481 R + 128553 G + 24966 B) / 255000 + 16), in integer arithmetic (exact)
__device__ __forceinline__ uint32_t q_luma(uint32_t r, uint32_t g, uint32_t b) {
    const uint32_t num = 65481u * r + 128553u * g + 24966u * b;   // <= 55 845 000
    const uint32_t q = num / 255000u, rem = num - q * 255000u;
    uint32_t y = q + 16u;
    if (rem > 127500u || (rem == 127500u && (y & 1u))) ++y;
    return y;
}

}  // namespace ofasr
