// Device side of SdDrop (style_dp_launch.h): which elements a training site of the style encoder / duration predictor keeps.
#pragma once
#include "common.h"
#include "style_dp_launch.h"

namespace st {

// element site: element index i of the (B, C, T) tensor the dropout acts on (the FFN sites' hash of the decoder)
__device__ __forceinline__ float sd_drop_elem(const SdDrop& d, unsigned long long i) {
    if (!d.thresh16) return 1.0f;
    const unsigned h = drop_ffn_hash(d, i);
    return ((i & 1) ? (h >> 16) : (h & 0xFFFFu)) >= d.thresh16 ? d.scale : 0.0f;
}
// attention site: row = (item * H + head) * T + query, key index (the decoder's attention sites' hash)
__device__ __forceinline__ float sd_drop_attn(const SdDrop& d, unsigned row, unsigned key) {
    if (!d.thresh16) return 1.0f;
    const unsigned h = drop_pair(drop_rowh(d.seed, row), drop_colh(d.seed, key >> 1));
    return ((key & 1) ? (h >> 16) : (h & 0xFFFFu)) >= d.thresh16 ? d.scale : 0.0f;
}

}  // namespace st
