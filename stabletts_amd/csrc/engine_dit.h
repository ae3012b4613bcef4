// Host-side internals of the two kinds made of DiT blocks, the CFM decoder and the text encoder: their state (DitState), the weight
// packing, the workspace plan and the launch sequences.  Shared by engine.cpp (inference), engine_solve.cpp (the ODE solvers behind
// st_cfm_solve) and engine_train.cpp (training: forward that keeps activations + backward).  Not part of the C ABI.
#pragma once
#include "engine_internal.h"
#include "common.h"
#include "stream_fork.h"

constexpr int kMaxParts = 1 + sthost::StreamFork::kMaxChildren;      // solve parts: part 0 on the caller's stream, the others on part_streams
constexpr size_t kSplitKBytes = 32u << 20;

namespace sthost {

struct TrainState;     // engine_train.cpp

struct DitState : KindState {
    st_config cfg{};
    bool dec = true;                    // KIND_DECODER (false: the text encoder)
    int M = 0, Mp = 0, C = 0, F = 0, H = 0, L = 0, K = 0, G = 0;
    int n_vocab = 0;
    // parameter-name prefix of DiT block i: estimator.py:13,79 "blocks.i.block." / text_encoder.py:25 "encoder.i."
    std::string blk(int i) const { return dec ? "blocks." + std::to_string(i) + ".block." : "encoder." + std::to_string(i) + "."; }
    // Packing job lists (common.h: PackJob): pack_all / train_prepare record one job per packed tensor slice and run the list as ONE
    // launch, the first pack included; later re-packs of the same parameter tensors launch the uploaded list again.  Dropped whenever
    // a parameter pointer may have changed.  The blocks of a list run concurrently, so no two of its jobs may write the same
    // destination element: every job of the two lists has a buffer, row block or column slice of its own (split parts and the
    // [h_hi | h_lo] q/k/v halves are disjoint column ranges, q / k / v disjoint rows or planes, the two FFN stages disjoint slabs).
    struct PackList { std::vector<st::PackJob> jobs; st::PackJob* dev = nullptr; unsigned nblocks = 0; bool ready = false; };
    PackList pk_fwd, pk_T;
    bool packed_once = false;          // pack_all has allocated the packed-weight buffers (st_repack re-uses them)

    // packed weights
    std::vector<Conv> pre;              // 3 prenet convs
    Conv inx, inc, fin;                 // in_proj x-part / cond-part, final_proj
    std::vector<Conv> lsc, qkv, oproj, ffn1, ffn2;
    std::vector<void*> oproj_frag;      // per block: the out-projection weight in fragment order (oproj_ws.hip)
    std::vector<void*> qkv_frag;        // per block: the q/k/v weight in fragment order (qkv_ws.hip); empty if unsupported
    std::vector<void*> ffn_stream;      // per block: conv_1 + conv_2 weights as the fused FFN kernel's stream (ffn_fused.h); empty if unsupported

    float* rope_cos = nullptr; float* rope_sin = nullptr; int rope_T = 0;
    void* sink = nullptr;               // 64 KiB of scratch: store target of rows outside the tensor (qkv_ws.hip)

    int64_t last_nfe = 0, last_steps = 0, last_rejects = 0;   // statistics of the last solve
    // Non-finite guard: the boundary kernel that writes a call's output sets *status_host (host-mapped, no synchronisation) when a
    // value is NaN / Inf -- an f16 operand beyond 65504, a bad input.  st_output_status reads it after a stream sync; the next call
    // reads it without one and, if set, re-zeroes the arena (ragged tile skipping leaves stale frames that are only ever read by
    // don't-care positions, but 0 x NaN would leak: arena_fresh).
    int* status_host = nullptr; int* status_dev = nullptr;
    bool arena_poisoned(st_engine* e) { if (status_host && *status_host) { *status_host = 0; e->ws_sig = 0; return true; } return false; }

    void* adams_buf = nullptr; size_t adams_bytes = 0;     // extra state buffers of the implicit Adams solver (allocated at its first use)
    unsigned skip_mask = 0;             // developer tool, -DST_DEVTOOLS builds only (ST_SKIP_CLASSES, bit = profile class): launches of these classes of run_estimator are NOT issued -- what a
                                        // class costs the solve with its parts overlapping on four streams (tools/ab_engines.py); results are garbage
    int qkv_ws_min_tiles = 400;         // ... when the launch has at least this many 64-frame tiles (>= 5 per persistent block)
    int qkv_ws = 1;                     // fused q/k/v projection of big grids as the weight-stationary persistent kernel (qkv_ws.hip; default);
                                        // ST_QKV_WS=0: the generic conv tile
    int oproj_ws = 1;                   // out projection of big grids as the weight-stationary persistent kernel (oproj_ws.hip; default); ST_OPROJ_WS=0: the generic 256 x 256 tile
    int oproj_ws_min_tiles = 1000;      // ... from this many 32-frame tiles per launch
    int qkv_rc1 = 1;                    // fused q/k/v projection of big grids on 256 x 128 tiles with one weight buffer, two blocks per CU (ST_QKV_RC1=0: A/B)
    int fused_ffn = -1;                 // FFN of big grids as ONE kernel, the intermediate kept in LDS.  -1 = default = 1: the direct kernel on 32x32x16 MFMA
                                        // (ffn_fused.h, bit-identical to the two-kernel path); ST_FUSED_FFN=3 (opt-in, f16 only): Winograd F(2,3) along the frames
                                        // (ffn_wino.h: a third fewer MFMAs, -1.45 % per solve, NOT bit-identical -- rounded sums as operands, +20 % error, half the
                                        // f16 range for the intermediate); ST_FUSED_FFN=0: two kernels.  Read at st_create.
    int attn_split = 0;                 // st_set_option("attention_precision", 1): q and k as hi + lo operand pairs, scores from three products (attention.hip: SPLIT)
    unsigned* lse_cells = nullptr;      // kLseCells cells 64 B apart: max over attention rows of the log2-sum-exp since the last st_attention_stats (order-preserving int bits)
    int attn_small_blocks = 32;         // attention launches of <= this many 256-query blocks use the key-split kernel
    int conc = 1;                       // solve parts in flight on separate streams (their launches share the chip)
    StreamFork part_streams;            // streams of solve parts 1.. (part 0 runs on the caller's stream)

    // HIP-graph replay of the fixed-grid solve body (ST_HIP_GRAPH=1): one instantiated graph per solve signature
    struct SolveGraph {
        int B, T, n_steps, solver, use_cfg; float cfg_strength; const char* ws; int parts; int seen; hipGraphExec_t exec;
    };
    std::vector<SolveGraph> graphs;
    hipStream_t gstream = nullptr;      // capture stream
    void drop_graphs() {
        for (auto& g : graphs) if (g.exec) hipGraphExecDestroy(g.exec);
        graphs.clear();
    }

    // training (engine_train.cpp): transposed dgrad weights, saved activations, gradient buffers; allocated by the first training forward
    TrainState* train = nullptr;

    ~DitState() override;
    int finalize(st_engine* e) override;
    int repack(st_engine* e, hipStream_t s) override;
    int64_t device_bytes() const override;
    int64_t train_serial() const override;
    void params_moved() override { pk_fwd.ready = false; pk_T.ready = false; drop_graphs(); }      // the recorded re-pack jobs hold the old pointer, and instantiated
                                                                                                    // solve graphs read the fp32 linears (adaLN, FiLM, time MLP) through it
    void arena_moved() override { drop_graphs(); }      // instantiated graphs hold arena pointers
};

// The DiT state of a handle that check_handle (or check_ready's caller) has found to be a decoder or a text encoder
inline DitState* dit_of(st_engine* e) { return state_of<DitState>(e); }
inline const DitState* dit_of(const st_engine* e) { return state_of<DitState>(e); }
// ... and of any handle, for gemm() and the entry points that answer every kind: nullptr for the other kinds
inline const DitState* dit_or_null(const st_engine* e) { return e->kind == KIND_DECODER || e->kind == KIND_TEXT_ENCODER ? dit_of(e) : nullptr; }
inline DitState* dit_or_null(st_engine* e) { return const_cast<DitState*>(dit_or_null(const_cast<const st_engine*>(e))); }

// Ragged batches leave frame tiles past an utterance's end uncomputed; whatever the arena holds there is only ever read by
// don't-care positions (masked keys, frames whose results are multiplied by the mask), but it must be FINITE: 0 x NaN would
// leak.  Stale values of the SAME layout are real activations of an earlier call (finite); when the layout changes (other B, T,
// CFG, part count, entry point) the bytes would be re-interpreted under another type, so the used range is zeroed once, on `s`.
int arena_fresh(st_engine* e, uint64_t sig, size_t used_bytes, hipStream_t s);
int ensure_rope(st_engine* e, int T, hipStream_t s);
// The common entry checks of the DiT kinds' forwards: null handle, finalized, sizes, then the handle's kind and 32-bit row indexing
int check_ready(st_engine* e, Kind kind, int B, int T);
int pack_all(st_engine* e, hipStream_t s);            // (re)packs every 16-bit weight; allocates on the first call only
// recorder / replayer of a PackList: begin -> pk_push per job (append only) -> end (upload + one launch); replay = that launch again
bool pk_replay(st_engine* e, DitState::PackList& L, hipStream_t s, int* rc);      // true: the list was replayed (or failed: *rc)
void pk_begin(DitState::PackList& L);
void pk_push(DitState::PackList& L, st::PackJob j);
int pk_end(st_engine* e, DitState::PackList& L, hipStream_t s);

// ---- engine.cpp: the workspace plan of one estimator pass (or solve part) and the launch sequences that use it
struct Plan {
    int B, T, Tp, N, Pn, n_t;
    bool cfg;
    // 16-bit MFMA operands.  *lo tensors hold x - float(hi): the split-precision operand pairs of the three GEMMs
    // whose rounding error reaches the output un-gated (in_proj x-part and cond-part, final_proj)
    void *mu16, *pre1, *pre2, *cond16, *cond16lo, *x16, *x16lo, *h16, *h2_16, *q16, *k16, *q16lo, *k16lo, *vt16, *ao16, *u16, *cur16, *cur16lo;
    void* skip16[8];
    // fp32
    float *cpart, *X, *v32, *xstate, *kbuf[7], *ynew, *ode_partial, *ode_out, *tvals, *emb, *th, *tau, *film, *cvec, *ada, *ada_tmp;
    int *n_full, *kv_end;
    int* t_lim;         // [B + 1] frames of every utterance that are computed (mask_prep: last valid + 1 + halo), [B] = the longest
    float* kbias;
    float* maskbuf;     // engine-owned copy of the caller's (B,1,T) mask: the solve body touches arena memory only
    struct Slot { void** dst; size_t off; };
    std::vector<Slot> slots;
};
// Lays the tensors of one solve (or solve part) out in the arena starting at byte `off`; returns the end offset.
// Pointers become valid after ensure_ws() + bind_plan().
size_t layout_plan(st_engine* e, int B, int T, bool cfg, int n_t, size_t off, Plan* p);
void bind_plan(st_engine* e, Plan* p);
uint64_t layout_sig(int entry, int B, int T, int cfg, int n_t, int parts);
int run_prenet(st_engine* e, const Plan& p, hipStream_t s);
int run_adaln(st_engine* e, const Plan& p, hipStream_t s);
int run_time_tables(st_engine* e, const Plan& p, hipStream_t s);
int run_estimator(st_engine* e, const Plan& p, const float* mask, int ev, hipStream_t s);

// engine_train.cpp
int train_prepare(st_engine* e, hipStream_t s);       // packs the transposed (dgrad) weights if the parameters changed
void train_invalidate(DitState* dit);                 // the parameters changed: dgrad weights and held activations are stale
void train_destroy(DitState* dit);
int64_t train_bytes(const DitState* dit);             // device bytes held by the training state

}  // namespace sthost
