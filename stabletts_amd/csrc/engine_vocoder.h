// What the Vocos and the FireflyGAN vocoder share behind the C ABI (engine_vocos.cpp, engine_ffgan.cpp): the entry sequence of
// st_*_forward and st_*_forward_ragged -- checks, chunk plan (chunk_plan.h), utterance tables (utt_slots.h), chunk loop -- and the
// flattened-row GEMM arguments.  A kind supplies a VocoderKind: its limits, its strides and its chunk function.  Not part of the C ABI.
#pragma once
#include "chunk_plan.h"
#include "utt_slots.h"

#include <cstring>
#include <string>

namespace sthost {

// One chunk of whole utterances: B utterances of mel (padded to T) to audio; rg = nullptr: dense, R = B * T rows.
using VocoderChunkFn = int (*)(st_engine* e, const float* mel, float* audio, int B, int T, const RaggedChunk* rg, hipStream_t s);

struct VocoderGeom {
    ChunkLimits dense, ragged;
    int channels, hop;      // mel channels; audio samples per frame
    UttSlots* slots;
};

struct VocoderKind {
    Kind kind;
    const char* indexing;                   // what an over-long utterance exceeds, as the messages name it
    int64_t max_T;                          // frames of one padded utterance, refused before the lengths are read (0: max_rows alone)
    VocoderGeom (*geom)(st_engine* e);      // of a handle of `kind`
    int (*dw_frames)(int64_t rows);         // the depthwise kernel's group length for a ragged chunk's packed rows
    VocoderChunkFn chunk;
};

// The arguments of a GEMM over the R flattened rows of a chunk (taps = 1: rows are independent); the caller adds sources and outputs
inline st::ConvGemmArgs flat_gemm_args(const st_engine* e, const Conv& cv, int64_t R) {
    st::ConvGemmArgs a; memset(&a, 0, sizeof(a));
    a.w = cv.w; a.bias = cv.bias; a.cout = cv.cout; a.T = (int)R; a.n_items = 1;
    a.a0_mod = 1; a.a1_mod = 1; a.mask_mod = 1; a.zeros = e->zeros;
    return a;
}

constexpr const char* kChunkedCapture = "debug capture holds whole-batch tensors: this batch runs in chunks";

inline int vocoder_forward(const VocoderKind& k, st_engine* e, const float* mel, float* audio, int B, int T, void* stream) {
    int rc = check_handle(e, k.kind); if (rc) return rc;
    if ((rc = check_finalized(e))) return rc;
    if (!mel || !audio) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if ((rc = check_sizes(e, B, T))) return rc;
    const VocoderGeom g = k.geom(e);
    if (T > g.dense.max_rows || (k.max_T && T > k.max_T))
        return e->fail(ST_ERR_INVALID, std::string("T too large: one utterance exceeds ") + k.indexing);
    const int chunk = dense_chunk(B, T, g.dense);
    if (chunk < B && e->capture) return e->fail(ST_ERR_INVALID, kChunkedCapture);
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t mel_item = (size_t)g.channels * T, audio_item = (size_t)T * g.hop;
    for (int b0 = 0; b0 < B; b0 += chunk)
        if ((rc = k.chunk(e, mel + b0 * mel_item, audio + b0 * audio_item, std::min(chunk, B - b0), T, nullptr, s))) return rc;
    return ST_OK;
}

// Validates everything and plans the chunks before touching the device: whole utterances, as many as the kind's limits allow
inline int vocoder_forward_ragged(const VocoderKind& k, st_engine* e, const float* mel, const int64_t* lengths, float* audio, int B, int T, void* stream) {
    int rc = check_handle(e, k.kind); if (rc) return rc;
    if ((rc = check_finalized(e))) return rc;
    if (!mel || !audio) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if (!lengths) return e->fail(ST_ERR_INVALID, "null lengths");
    if ((rc = check_sizes(e, B, T))) return rc;
    const VocoderGeom g = k.geom(e);
    if (k.max_T && T > k.max_T) return e->fail(ST_ERR_INVALID, std::string("T too large: one utterance exceeds ") + k.indexing);
    for (int b = 0; b < B; ++b)
        if (lengths[b] < 1 || lengths[b] > T)
            return e->fail(ST_ERR_INVALID, "lengths[" + std::to_string(b) + "] = " + std::to_string(lengths[b]) + " must be in [1, T = " + std::to_string(T) + "]");
    for (int b = 0; b < B; ++b)
        if (lengths[b] > g.ragged.max_rows)
            return e->fail(ST_ERR_INVALID, "lengths[" + std::to_string(b) + "] too large: one utterance exceeds " + k.indexing);
    if (g.ragged.max_padded_frames && T > g.ragged.max_padded_frames)
        return e->fail(ST_ERR_INVALID, "T too large: the padded audio of one utterance exceeds one launch");
    const std::vector<int> starts = plan_chunks(lengths, B, T, g.ragged);
    const int n_chunks = (int)starts.size() - 1;
    if (n_chunks > 1 && e->capture) return e->fail(ST_ERR_INVALID, kChunkedCapture);
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    int slot = 0;
    if ((rc = g.slots->acquire(e, B, &slot))) return rc;
    std::vector<RaggedChunk> chunks(n_chunks);
    for (int c = 0; c < n_chunks; ++c) chunks[c] = g.slots->fill(slot, lengths, starts[c], starts[c + 1], k.dw_frames);
    if ((rc = g.slots->upload(e, slot, B, s))) return rc;
    const size_t mel_item = (size_t)g.channels * T, audio_item = (size_t)T * g.hop;
    for (int c = 0; c < n_chunks && rc == ST_OK; ++c)
        rc = k.chunk(e, mel + starts[c] * mel_item, audio + starts[c] * audio_item, starts[c + 1] - starts[c], T, &chunks[c], s);
    hipError_t he = g.slots->record(slot, s);       // also after a failed chunk: the copy and the launches before it read the slot
    if (rc) return rc;
    HIPCHK(e, he);
    return ST_OK;
}

}  // namespace sthost
