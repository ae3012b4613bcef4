// How the vocoder entry points (engine_vocoder.h) cut a batch into chunks of whole utterances: pure host arithmetic over the
// lengths and a kind's limits.  No HIP header: a host compiler builds this alone (tests/host/chunk_plan_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace sthost {

// What one chunk may hold.  0 = no such cap for the two optional ones.
struct ChunkLimits {
    int64_t max_rows;               // flattened rows (frames) of a chunk: the 32-bit operand offsets of its GEMMs
    int64_t max_items;              // utterances of a chunk: a grid dimension
    int64_t max_padded_frames;      // optional: count * T, the padded frames of one launch over a ragged chunk
    int64_t head_rows;              // optional second row cap, a memory budget: one utterance above it still runs, alone
};

// Utterances per chunk of a dense batch (B x T, T >= 1 within max_rows): every chunk but the last holds this many.
inline int dense_chunk(int B, int T, const ChunkLimits& lim) {
    int64_t n = std::min<int64_t>({(int64_t)B, lim.max_rows / T, lim.max_items});
    if (lim.head_rows) n = std::min(n, std::max<int64_t>(1, lim.head_rows / T));
    return (int)n;
}

// Chunks of a ragged batch (every lengths[b] in [1, min(T, max_rows)], T within max_padded_frames): the first utterance of every
// chunk, then B.  Greedy: an utterance opens a new chunk when it would take the chunk past one of the caps.
inline std::vector<int> plan_chunks(const int64_t* lengths, int B, int T, const ChunkLimits& lim) {
    std::vector<int> starts;
    int64_t rows = 0;
    for (int b = 0; b < B; ++b) {
        const bool full = b > 0 && (rows + lengths[b] > lim.max_rows || (lim.head_rows && rows + lengths[b] > lim.head_rows) ||
                                    b - starts.back() >= lim.max_items ||
                                    (lim.max_padded_frames && (int64_t)(b - starts.back() + 1) * T > lim.max_padded_frames));
        if (b == 0 || full) { starts.push_back(b); rows = 0; }
        rows += lengths[b];
    }
    starts.push_back(B);
    return starts;
}

}  // namespace sthost
