// Utterance tables of the ragged vocoder entry points (st_vocos_forward_ragged, st_ffgan_forward_ragged): one VocUtt per utterance,
// written by the host into pinned memory and copied to a device slot on the caller's stream.  A slot is refilled only after the
// event of the call that used it last, so a call never waits for the one before it (as MelState, engine_audio.cpp).
#pragma once
#include "engine_internal.h"
#include "vocos_launch.h"

#include <vector>

namespace sthost {

// One chunk of a ragged batch: its utterance table (device, chunk-relative entries) and the sizes the host summed from it.
struct RaggedChunk {
    const st::VocUtt* utt;
    int64_t rows;
    int n_tiles, n_groups, dw_frames;
    int t_max;      // frames of its longest utterance
};

struct UttSlots {
    static constexpr int kSlots = 4;
    st::VocUtt* host[kSlots] = {};
    st::VocUtt* dev[kSlots] = {};
    hipEvent_t ev[kSlots] = {};
    bool used[kSlots] = {};
    int cap = 0, next = 0;

    // The next slot with room for B entries, free to be written: grows every slot (after their calls) when B exceeds the capacity.
    int acquire(st_engine* e, int B, int* slot) {
        if (B > cap) {
            for (int i = 0; i < kSlots; ++i) {
                if (used[i]) HIPCHK(e, hipEventSynchronize(ev[i]));
                if (host[i]) { hipHostFree(host[i]); host[i] = nullptr; }
                if (dev[i]) { hipFree(dev[i]); dev[i] = nullptr; }
                used[i] = false;
            }
            cap = 0;
            const int want = B > 64 ? B : 64;
            for (int i = 0; i < kSlots; ++i) {
                HIPCHK(e, hipHostMalloc((void**)&host[i], (size_t)want * sizeof(st::VocUtt)));
                HIPCHK(e, hipMalloc((void**)&dev[i], (size_t)want * sizeof(st::VocUtt)));
                if (!ev[i]) HIPCHK(e, hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
            }
            cap = want;
        }
        *slot = next;
        next = (next + 1) % kSlots;
        if (used[*slot]) HIPCHK(e, hipEventSynchronize(ev[*slot]));
        return ST_OK;
    }

    // Entries b0 .. b1 - 1 of the slot's host table, relative to their chunk (its rows, tables, mel and audio start at 0).
    // dw_frames_of: the depthwise kernel's group length for the chunk's packed rows.
    RaggedChunk fill(int slot, const int64_t* lengths, int b0, int b1, int (*dw_frames_of)(int64_t rows)) {
        RaggedChunk rg{dev[slot] + b0, 0, 0, 0, 1, 0};
        for (int b = b0; b < b1; ++b) rg.rows += lengths[b];
        rg.dw_frames = dw_frames_of(rg.rows);
        int row0 = 0;
        for (int b = b0; b < b1; ++b) {
            const int Tb = (int)lengths[b];
            host[slot][b] = st::VocUtt{row0, Tb, rg.n_tiles, rg.n_groups};
            row0 += Tb; rg.n_tiles += (Tb + 63) / 64; rg.n_groups += (Tb + rg.dw_frames - 1) / rg.dw_frames;
            if (Tb > rg.t_max) rg.t_max = Tb;
        }
        return rg;
    }

    int upload(st_engine* e, int slot, int B, hipStream_t s) {
        HIPCHK(e, hipMemcpyAsync(dev[slot], host[slot], (size_t)B * sizeof(st::VocUtt), hipMemcpyHostToDevice, s));
        used[slot] = true;
        return ST_OK;
    }

    // After the last launch that reads the slot -- also after a failed one: the copy and the launches before it read the slot.
    hipError_t record(int slot, hipStream_t s) { return hipEventRecord(ev[slot], s); }

    void destroy() {
        for (int i = 0; i < kSlots; ++i) {
            if (host[i]) hipHostFree(host[i]);
            if (dev[i]) hipFree(dev[i]);
            if (ev[i]) hipEventDestroy(ev[i]);
            host[i] = nullptr; dev[i] = nullptr; ev[i] = nullptr; used[i] = false;
        }
        cap = 0;
    }
};

}  // namespace sthost
