// Host side of libstabletts_hip.so: parameter store, weight packing, workspace arena and the estimator launch sequence behind
// the C ABI of include/stabletts_hip.h (the ODE solve around it: engine_solve.cpp).  Reference path: models/estimator.py:103-138.
#include "engine_dit.h"
#include "train_launch.h"
#include "mas_launch.h"
#include "align_train_launch.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace st;
using namespace sthost;

namespace sthost {
std::string g_create_error;

const char* kProfNames[PC_COUNT] = {
    "prep", "prenet_conv", "in_proj", "film_ln1", "qkv_rope", "attention", "out_proj", "ln2",
    "ffn_conv1", "ffn_conv2", "lsc_conv", "final_proj", "ode_update", "train_forward", "train_backward"};

int dev_alloc(st_engine* e, void** p, size_t bytes) {
    HIPCHK(e, hipMalloc(p, bytes ? bytes : 16));
    e->owned.push_back(*p);
    e->weight_bytes += (int64_t)bytes;
    return ST_OK;
}

void expect(st_engine* e, const std::string& name, std::vector<int64_t> shape) {
    Param p;
    p.shape = std::move(shape);
    e->params[name] = p;
}

void build_param_table(st_engine* e) {
    DitState* dit = dit_of(e);
    const int C = dit->C, F = dit->F, M = dit->M, K = dit->K, G = dit->G;
    if (e->kind == KIND_TEXT_ENCODER) {     // TextEncoder state_dict (models/text_encoder.py:22-26)
        expect(e, "emb.weight", {dit->n_vocab, C});
        for (int i = 0; i < dit->L; ++i) {
            const std::string p = dit->blk(i);
            for (const char* nm : {"q", "k", "v", "o"}) {
                expect(e, p + "attn.conv_" + nm + ".weight", {C, C, 1});
                expect(e, p + "attn.conv_" + nm + ".bias", {C});
            }
            expect(e, p + "mlp.conv_1.weight", {F, C, K}); expect(e, p + "mlp.conv_1.bias", {F});
            expect(e, p + "mlp.conv_2.weight", {C, F, K}); expect(e, p + "mlp.conv_2.bias", {C});
            if (G != C) { expect(e, p + "adaLN_modulation.0.weight", {C, G}); expect(e, p + "adaLN_modulation.0.bias", {C}); }
            expect(e, p + "adaLN_modulation.2.weight", {6 * C, C}); expect(e, p + "adaLN_modulation.2.bias", {6 * C});
        }
        expect(e, "proj.weight", {M, C, 1}); expect(e, "proj.bias", {M});
        return;
    }
    expect(e, "time_mlp.layer.0.weight", {F, C}); expect(e, "time_mlp.layer.0.bias", {F});
    expect(e, "time_mlp.layer.2.weight", {C, F}); expect(e, "time_mlp.layer.2.bias", {C});
    expect(e, "in_proj.weight", {C, C + M, 1}); expect(e, "in_proj.bias", {C});
    for (int i = 0; i < dit->L; ++i) {
        const std::string p = "blocks." + std::to_string(i) + ".";
        expect(e, p + "time_fusion.film.weight", {2 * C, C, 1}); expect(e, p + "time_fusion.film.bias", {2 * C});
        for (const char* nm : {"q", "k", "v", "o"}) {
            expect(e, p + "block.attn.conv_" + nm + ".weight", {C, C, 1});
            expect(e, p + "block.attn.conv_" + nm + ".bias", {C});
        }
        expect(e, p + "block.mlp.conv_1.weight", {F, C, K}); expect(e, p + "block.mlp.conv_1.bias", {F});
        expect(e, p + "block.mlp.conv_2.weight", {C, F, K}); expect(e, p + "block.mlp.conv_2.bias", {C});
        if (G != C) {
            expect(e, p + "block.adaLN_modulation.0.weight", {C, G});
            expect(e, p + "block.adaLN_modulation.0.bias", {C});
        }
        expect(e, p + "block.adaLN_modulation.2.weight", {6 * C, C});
        expect(e, p + "block.adaLN_modulation.2.bias", {6 * C});
    }
    expect(e, "final_proj.weight", {M, C, 1}); expect(e, "final_proj.bias", {M});
    expect(e, "cond_proj.0.weight", {F, M, K}); expect(e, "cond_proj.0.bias", {F});
    expect(e, "cond_proj.2.weight", {F, F, K}); expect(e, "cond_proj.2.bias", {F});
    expect(e, "cond_proj.4.weight", {C, F, K}); expect(e, "cond_proj.4.bias", {C});
    for (int i = 0; i < dit->L / 2; ++i) {
        expect(e, "lsc_layers." + std::to_string(i) + ".weight", {C, 2 * C, K});
        expect(e, "lsc_layers." + std::to_string(i) + ".bias", {C});
    }
}

const float* P(st_engine* e, const std::string& name) { return e->params.at(name).dev; }

// Tile configuration of one conv launch.  256x256 tiles (half the LDS traffic per MFMA of the 128-wide ones: the K
// loop is LDS-bound) whenever the output is a multiple of 256 channels, T fills 256-frame tiles about as well as
// 128-frame ones and the launch has enough of them for the chip (small grids would leave most CUs idle behind a
// few long-running blocks); otherwise row-complete 256x128 tiles where the epilogue needs whole rows (fused
// LayerNorm, QKV planes), the 3-buffer pipeline for deep k=3 convs, 128x128 tiles for the rest.
// 256 x 256 tiles (BIG / PHASED / RC1) are used when they waste little of the last frame tile and fill the chip
static int launches_in_flight(const DitState* dit) { return dit ? dit->conc : 1; }      // launch sequences that share the chip: the parts of a DiT solve
static bool big_tiles(const st_engine* e, int conc, const ConvGemmArgs& a) {
    const int T = a.T;
    const bool fills = ((T + 255) / 256) * 256 * 10 <= ((T + 127) / 128) * 128 * 11;
    const bool big_fills_chip = (int64_t)conc * a.n_items * ((T + 255) / 256) * (a.cout / 256) >= e->tile.big_min_blocks;
    return a.cout % 256 == 0 && fills && big_fills_chip;
}
bool gemm_is_phased(const st_engine* e, int taps, const ConvGemmArgs& a) {
    return taps == 3 && e->tile.phased && big_tiles(e, launches_in_flight(dit_or_null(e)), a);
}

hipError_t gemm(st_engine* e, int taps, int epi, const ConvGemmArgs& a, hipStream_t s) {
    const DitState* dit = dit_or_null(e);      // the weight-stationary kernels below are the DiT kinds' own
    const int conc = launches_in_flight(dit);
    const bool big = big_tiles(e, conc, a);
    const bool bf = e->dt == DT_BF16;
    const int T = a.T;
    if (epi == EPI_SILU && !(taps == 3 && e->tile.phased && big)) return hipErrorInvalidValue;      // callers ask gemm_is_phased first
    // Small grids (a few frame tiles in total: single-utterance synthesis): the K loop of one block is a serial chain
    // of DMA -> barrier -> MFMA stages, so a handful of blocks walking 24..48 stages each leaves the chip idle for
    // tens of microseconds.  Split the contraction over `ks` blocks per output tile (raw fp32 partial planes in
    // e->tile.kpart) and apply the epilogue -- including a fused LayerNorm -- in a row-wise finish kernel.
    if (e->tile.kpart && conc == 1 && a.cout == 256 && (epi == EPI_F32 || epi == EPI_RESGATE) && !a.w_item_stride) {
        const int nch = (a.c0 + a.c1 + a.c2) / 64;
        const int64_t blocks = (int64_t)a.n_items * ((T + 127) / 128) * 2;
        const int64_t plane = (int64_t)a.n_items * T * 256 * 4;
        int ks = (int)std::min<int64_t>(std::min(nch, e->tile.splitk_max), e->tile.splitk_target / blocks);
        ks = (int)std::min<int64_t>(ks, (int64_t)e->tile.kpart_bytes / plane);
        if (ks >= 2 && nch * taps >= e->tile.splitk_min_stages) {
            ConvGemmArgs pa = a;
            pa.t_lim = nullptr;
            pa.bias = nullptr; pa.flags = 0; pa.mask = nullptr; pa.add32 = nullptr; pa.out16 = nullptr; pa.out16_lo = nullptr;
            pa.ln_h16 = nullptr; pa.gate = nullptr; pa.res32 = nullptr; pa.branch32 = nullptr; pa.out32 = e->tile.kpart; pa.ksplit = ks;
            const int pcfg = e->tile.small_tiles ? G2_T64 : G2_T128;
            hipError_t he = bf ? launch_conv_gemm2_bf16(pcfg, taps, EPI_F32, pa, s) : launch_conv_gemm2_f16(pcfg, taps, EPI_F32, pa, s);
            if (he != hipSuccess) return he;
            return bf ? launch_splitk_finish_bf16(epi, a, e->tile.kpart, ks, s) : launch_splitk_finish_f16(epi, a, e->tile.kpart, ks, s);
        }
    }
    // the fused q/k/v projection of big grids: weights in registers, activations streamed (qkv_ws.hip; bit-identical)
    if (dit && epi == EPI_QKV && dit->qkv_ws && !a.q_lo && !a.vt_lo && dit->sink && a.w_frag && a.cout == 768 && a.c0 == 256 && !a.c1 && !a.c2 && a.n_heads == 4 &&
        (int64_t)a.n_items * ((T + 63) / 64) >= dit->qkv_ws_min_tiles) {      // (per LAUNCH: a block needs a handful of tiles to amortise its weight load)
        ConvGemmArgs b = a; b.sink = dit->sink;
        return launch_qkv_ws(e->dt, b, s);
    }
    // the out projection (+ LayerNorm_2) of big grids in the same style (oproj_ws.hip; bit-identical)
    if (dit && epi == EPI_RESGATE && taps == 1 && dit->oproj_ws && dit->sink && a.w_frag && a.ln_h16 && !a.ln_film && a.cout == 256 && a.c0 == 256 &&
        !a.c1 && !a.c2 && !a.out16 && !a.res32 && !a.branch32 && !a.out32_readonly && a.out32 &&
        (int64_t)a.n_items * ((T + 31) / 32) >= dit->oproj_ws_min_tiles) {
        ConvGemmArgs b = a; b.sink = dit->sink;
        return launch_oproj_ws(e->dt, b, s);
    }
    int cfg;
    if (big) cfg = (e->tile.phased && taps == 3) ? G2_PHASED : (dit && epi == EPI_QKV && dit->qkv_rc1) ? G2_RC1 : G2_BIG;
    else if (a.ln_h16 || epi == EPI_QKV) cfg = G2_RC;
    else if (taps == 3 && a.c0 + a.c1 >= 512 && a.c2 == 0) cfg = G2_K3PIPE;
    else cfg = G2_T128;
    // latency-bound small grids: 64-frame tiles double the block count and halve every block's serial work
    const bool tiny = e->tile.small_tiles && conc == 1 && (int64_t)a.n_items * ((T + 127) / 128) * (a.cout / 128) <= e->tile.small_tiles;
    if (tiny && cfg == G2_T128 && (epi == EPI_ACT16 ? taps == 3 : epi == EPI_F32)) cfg = G2_T64;
    if (tiny && cfg == G2_RC && epi == EPI_QKV) cfg = G2_RC64;
    return bf ? launch_conv_gemm2_bf16(cfg, taps, epi, a, s) : launch_conv_gemm2_f16(cfg, taps, epi, a, s);
}

// ---- profiling helpers -----------------------------------------------------------------------
ProfScope::ProfScope(st_engine* e_, hipStream_t s_, int cls, double flops) : e(e_), s(s_) {
    if (!e->prof || !((e->prof_mask >> cls) & 1ull)) return;
    if ((e->prof_seen[cls]++ % e->prof_stride) != 0) return;
    ProfEvent ev; ev.cls = cls; ev.flops = flops;
    for (hipEvent_t* h : {&ev.a, &ev.b}) {
        if (!e->ev_pool.empty()) { *h = e->ev_pool.back(); e->ev_pool.pop_back(); }
        else if (hipEventCreate(h) != hipSuccess) return;
    }
    hipEventRecord(ev.a, s);
    e->evs.push_back(ev);
    idx = (int)e->evs.size() - 1;
}
ProfScope::~ProfScope() { if (idx >= 0) hipEventRecord(e->evs[idx].b, s); }

void prof_collect(st_engine* e) {
    for (auto& ev : e->evs) {
        float ms = 0.f;
        if (hipEventSynchronize(ev.b) == hipSuccess && hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess) {
            e->prof_launches[ev.cls] += 1;
            e->prof_ms[ev.cls] += ms;
            e->prof_flops[ev.cls] = ev.flops;
        }
        e->ev_pool.push_back(ev.a); e->ev_pool.push_back(ev.b);
    }
    e->evs.clear();
}

// ---- debug capture ---------------------------------------------------------------------------
void capture(st_engine* e, const std::string& name, const void* dev, int64_t n, bool is16, hipStream_t s) {
    if (!e->capture) return;
    Captured& c = e->caps[name];
    const size_t bytes = (size_t)n * (is16 ? 2 : 4);
    if (c.dev) { hipFree(c.dev); c.dev = nullptr; }
    if (hipMalloc(&c.dev, bytes) != hipSuccess) { c.dev = nullptr; return; }
    c.n = n; c.is16 = is16;
    hipMemcpyAsync(c.dev, dev, bytes, hipMemcpyDeviceToDevice, s);
}

// ---- workspace plan (engine_internal.h: Plan) ------------------------------------------------
size_t layout_plan(st_engine* e, int B, int T, bool cfg, int n_t, size_t off, Plan* p) {
    DitState* dit = dit_of(e);
    const int C = dit->C, F = dit->F, Mp = dit->Mp, L = dit->L;
    p->B = B; p->T = T; p->cfg = cfg; p->n_t = n_t;
    p->Tp = (T + 63) / 64 * 64;
    p->N = cfg ? 2 * B : B;
    p->Pn = cfg ? B + 1 : B;
    const size_t N = p->N, Pn = p->Pn, TT = T;
    p->slots.clear();
    auto want = [&](void** dst, size_t bytes) { p->slots.push_back({dst, off}); off = align_up(off + bytes, 256); };
    want(&p->mu16, Pn * TT * Mp * 2);
    want(&p->pre1, Pn * TT * F * 2);
    want(&p->pre2, Pn * TT * F * 2);
    want(&p->cond16, Pn * TT * C * 2);
    want(&p->cond16lo, Pn * TT * C * 2);
    want((void**)&p->cpart, Pn * TT * C * 4);
    want(&p->x16, (size_t)B * TT * Mp * 2);
    want(&p->x16lo, (size_t)B * TT * Mp * 2);
    want((void**)&p->xstate, (size_t)B * TT * Mp * 4);
    for (int i = 0; i < 7; ++i) want((void**)&p->kbuf[i], (size_t)B * TT * Mp * 4);
    want((void**)&p->ynew, (size_t)B * TT * Mp * 4);
    want((void**)&p->ode_partial, (size_t)2 * kOdeNormBlocks * 4);
    want((void**)&p->ode_out, 16);
    want((void**)&p->X, N * TT * C * 4);
    want(&p->h16, N * TT * C * 2);
    // FFN input of the fused FFN kernel: its blocks read h2 rows of NEIGHBOURING tiles (conv halo) until their last chunk while
    // other blocks already write the next block's LayerNorm output -- which the two-kernel path puts into h16 itself (conv_1 has
    // finished with it by then).  A separate buffer removes that cross-block write-after-read (found as run-to-run differences of
    // 4e-5 with several solve parts in flight).
    want(&p->h2_16, N * TT * C * 2);
    want(&p->q16, N * TT * C * 2);
    want(&p->k16, N * TT * C * 2);
    want(&p->q16lo, N * TT * C * 2);      // split-precision attention operands (st_set_option "attention_precision"): always laid out,
    want(&p->k16lo, N * TT * C * 2);      // so that switching the mode does not move the arena
    want(&p->vt16, N * (size_t)C * p->Tp * 2);
    want(&p->ao16, N * TT * C * 2);
    want(&p->u16, N * TT * F * 2);
    want(&p->cur16, N * TT * C * 2);
    want(&p->cur16lo, N * TT * C * 2);
    for (int i = 0; i < L / 2; ++i) want(&p->skip16[i], N * TT * C * 2);
    want((void**)&p->v32, N * TT * Mp * 4);
    want((void**)&p->tvals, (size_t)n_t * 4);
    want((void**)&p->emb, (size_t)n_t * C * 4);
    want((void**)&p->th, (size_t)n_t * F * 4);
    want((void**)&p->tau, (size_t)n_t * C * 4);
    want((void**)&p->film, (size_t)L * n_t * 2 * C * 4);
    want((void**)&p->cvec, N * (size_t)dit->G * 4);
    want((void**)&p->ada_tmp, N * (size_t)C * 4);
    want((void**)&p->ada, (size_t)L * N * 6 * C * 4);
    want((void**)&p->n_full, (size_t)B * 4);
    want((void**)&p->kv_end, (size_t)B * 4);
    want((void**)&p->t_lim, (size_t)(B + 1) * 4);
    want((void**)&p->kbias, (size_t)B * p->Tp * 4);
    want((void**)&p->maskbuf, (size_t)B * TT * 4);
    return off;
}

int ensure_ws(st_engine* e, size_t bytes) {
    if (bytes <= e->ws_cap) return ST_OK;
    e->state->arena_moved();
    if (e->ws) { HIPCHK(e, hipDeviceSynchronize()); HIPCHK(e, hipFree(e->ws)); e->ws = nullptr; e->ws_cap = 0; }
    HIPCHK(e, hipMalloc((void**)&e->ws, bytes));
    e->ws_cap = bytes;
    e->ws_sig = 0;
    return ST_OK;
}

int arena_fresh(st_engine* e, uint64_t sig, size_t used_bytes, hipStream_t s) {
    if (sig == e->ws_sig) return ST_OK;
    HIPCHK(e, hipMemsetAsync(e->ws, 0, used_bytes, s));
    e->ws_sig = sig;
    return ST_OK;
}

uint64_t layout_sig(int entry, int B, int T, int cfg, int n_t, int parts) {
    uint64_t h = 1469598103934665603ull;
    for (uint64_t v : {(uint64_t)entry, (uint64_t)B, (uint64_t)T, (uint64_t)cfg, (uint64_t)n_t, (uint64_t)parts}) { h ^= v + 0x9E3779B97F4A7C15ull; h *= 1099511628211ull; }
    return h | 1ull;
}

void bind_plan(st_engine* e, Plan* p) {
    for (auto& sl : p->slots) *sl.dst = e->ws + sl.off;
}

int make_plan(st_engine* e, int B, int T, bool cfg, int n_t, Plan* p) {
    const size_t end = layout_plan(e, B, T, cfg, n_t, 0, p);
    int rc = ensure_ws(e, end); if (rc) return rc;
    bind_plan(e, p);
    return ST_OK;
}

int ensure_rope(st_engine* e, int T, hipStream_t s) {
    DitState* dit = dit_of(e);
    if (T <= dit->rope_T) return ST_OK;
    // cos/sin cache of RotaryPositionalEmbeddings._build_cache (diffusion_transformer.py:145-171),
    // d = head_dim/2 = 32 rotary features -> 16 angles theta_j = 10000^(-2j/32), fp32 arithmetic.
    const int newT = (T + 255) / 256 * 256;
    std::vector<float> hc((size_t)newT * 16), hs((size_t)newT * 16);
    for (int j = 0; j < 16; ++j) {
        const float theta = 1.0f / powf(10000.0f, (float)(2 * j) / 32.0f);
        for (int t = 0; t < newT; ++t) {
            const float ang = (float)t * theta;
            hc[(size_t)t * 16 + j] = cosf(ang);
            hs[(size_t)t * 16 + j] = sinf(ang);
        }
    }
    if (dit->rope_cos) {
        dit->drop_graphs();      // instantiated graphs bake the old table pointers into the QKV kernel arguments
        HIPCHK(e, hipDeviceSynchronize()); hipFree(dit->rope_cos); hipFree(dit->rope_sin);
        dit->rope_cos = dit->rope_sin = nullptr; dit->rope_T = 0;
    }
    HIPCHK(e, hipMalloc((void**)&dit->rope_cos, hc.size() * 4));
    HIPCHK(e, hipMalloc((void**)&dit->rope_sin, hs.size() * 4));
    HIPCHK(e, hipMemcpy(dit->rope_cos, hc.data(), hc.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(dit->rope_sin, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
    dit->rope_T = newT;
    (void)s;
    return ST_OK;
}

ConvGemmArgs base_args(const st_engine* e, const Plan& p, const Conv& cv, int n_items) {
    ConvGemmArgs a;
    memset(&a, 0, sizeof(a));
    a.w = cv.w; a.bias = cv.bias; a.cout = cv.cout; a.T = p.T; a.n_items = n_items;
    a.tiles_f = (p.T + kGemmFramesPerTile - 1) / kGemmFramesPerTile;
    a.tiles_c = cv.cout / kGemmChannelsPerTile;
    a.a0_mod = n_items; a.a1_mod = n_items; a.mask_mod = p.B;
    a.zeros = e->zeros;
    // ragged batches: tiles past an utterance's last needed frame are skipped (every frame is computed under debug
    // capture, whose taps are compared over the whole padded tensor).  The shared uncond prenet item (index B of B + 1)
    // is needed as far as the longest utterance: entry B of t_lim.
    if (e->tile.ragged_skip && !e->capture && e->kind == KIND_DECODER) { a.t_lim = p.t_lim; a.t_lim_mod = (n_items == p.B + 1) ? p.B + 1 : p.B; }
    return a;
}

// FLOPs of the reference's convolution (a split-precision operand triples the MFMA work of its small GEMM, not
// the algorithmic count)
inline double conv_flops(const Plan& p, const Conv& cv, int n_items) {
    return 2.0 * (double)n_items * p.T * cv.cout * (cv.split ? cv.cin / 3 : cv.cin) * cv.taps;
}

// cond prenet (estimator.py:83-89,118) + the loop-invariant cond half of in_proj (:120-121)
int run_prenet(st_engine* e, const Plan& p, hipStream_t s) {
    DitState* dit = dit_of(e);
    {
        ConvGemmArgs a = base_args(e, p, dit->pre[0], p.Pn);
        a.a0 = p.mu16; a.c0 = dit->Mp; a.flags = GF_SILU; a.out16 = p.pre1;
        ProfScope ps(e, s, PC_PRENET, conv_flops(p, dit->pre[0], p.Pn));
        HIPCHK(e, gemm(e, 3, EPI_ACT16, a, s));
    }
    {
        ConvGemmArgs a = base_args(e, p, dit->pre[1], p.Pn);
        a.a0 = p.pre1; a.c0 = dit->F; a.flags = GF_SILU; a.out16 = p.pre2;
        ProfScope ps(e, s, PC_PRENET, conv_flops(p, dit->pre[1], p.Pn));
        HIPCHK(e, gemm(e, 3, EPI_ACT16, a, s));
    }
    {
        ConvGemmArgs a = base_args(e, p, dit->pre[2], p.Pn);
        a.a0 = p.pre2; a.c0 = dit->F; a.out16 = p.cond16; a.out16_lo = p.cond16lo;
        ProfScope ps(e, s, PC_PRENET, conv_flops(p, dit->pre[2], p.Pn));
        HIPCHK(e, gemm(e, 3, EPI_F32, a, s));
    }
    capture(e, "cond", p.cond16, (int64_t)p.Pn * p.T * dit->C, true, s);
    {   // K = [cond_hi | cond_lo | cond_hi] against [W_hi | W_hi | W_lo]: once per solve, so the extra MFMA work is free
        ConvGemmArgs a = base_args(e, p, dit->inc, p.Pn);
        a.a0 = p.cond16; a.c0 = dit->C; a.a1 = p.cond16lo; a.c1 = dit->C; a.c2 = dit->C; a.out32 = p.cpart;
        ProfScope ps(e, s, PC_INPROJ, conv_flops(p, dit->inc, p.Pn));
        HIPCHK(e, gemm(e, 1, EPI_F32, a, s));
    }
    return ST_OK;
}

// adaLN-Zero parameters from the speaker vectors (diffusion_transformer.py:92-96,110): loop invariant
int run_adaln(st_engine* e, const Plan& p, hipStream_t s) {
    DitState* dit = dit_of(e);
    const int C = dit->C;
    ProfScope ps(e, s, PC_PREP, 0);
    if (dit->G == C) HIPCHK(e, launch_silu_rows(p.cvec, (int64_t)p.N * C, p.ada_tmp, s));      // SiLU(c): the same input for every block
    for (int i = 0; i < dit->L; ++i) {
        const std::string pre = dit->blk(i) + "adaLN_modulation.";
        if (dit->G != C) {
            HIPCHK(e, launch_linear(p.cvec, p.N, dit->G, P(e, pre + "0.weight"), P(e, pre + "0.bias"), C, p.ada_tmp, 0, 0, s));
            HIPCHK(e, launch_linear(p.ada_tmp, p.N, C, P(e, pre + "2.weight"), P(e, pre + "2.bias"), 6 * C,
                                    p.ada + (size_t)i * p.N * 6 * C, 1, 0, s));
        } else {
            HIPCHK(e, launch_linear(p.ada_tmp, p.N, C, P(e, pre + "2.weight"), P(e, pre + "2.bias"), 6 * C,
                                    p.ada + (size_t)i * p.N * 6 * C, 0, 0, s));
        }
    }
    return ST_OK;
}

// time embedding -> MLP -> FiLM (gamma, beta) for every evaluation time (estimator.py:117,31-33)
int run_time_tables(st_engine* e, const Plan& p, hipStream_t s) {
    DitState* dit = dit_of(e);
    const int C = dit->C, F = dit->F;
    ProfScope ps(e, s, PC_PREP, 0);
    HIPCHK(e, launch_time_embed(p.tvals, p.n_t, C, p.emb, s));
    HIPCHK(e, launch_linear(p.emb, p.n_t, C, P(e, "time_mlp.layer.0.weight"), P(e, "time_mlp.layer.0.bias"), F, p.th, 0, 1, s));
    HIPCHK(e, launch_linear(p.th, p.n_t, F, P(e, "time_mlp.layer.2.weight"), P(e, "time_mlp.layer.2.bias"), C, p.tau, 0, 0, s));
    for (int i = 0; i < dit->L; ++i) {
        const std::string pre = "blocks." + std::to_string(i) + ".time_fusion.film.";
        HIPCHK(e, launch_linear(p.tau, p.n_t, C, P(e, pre + "weight"), P(e, pre + "bias"), 2 * C,
                                p.film + (size_t)i * p.n_t * 2 * C, 0, 0, s));
    }
    return ST_OK;
}

// The L DiT blocks and the output projection, for both kinds that are made of them.
// Decoder: one vector-field evaluation over N items given x16/x16lo (B items), cpart, ada, film; output p.v32.
//   ev: index into the time tables (scalar t shared by all items) or -1 for per-item t (n_t == B).
// Text encoder (models/text_encoder.py:40-42): the residual stream p.X comes masked from the embedding kernel; outputs p.X
//   and p.v32 (proj); ev is not read.
// Every FiLM + LayerNorm + modulate runs inside the epilogue of the GEMM that produces its input (row-complete
// tiles): in_proj -> LN1 of block 0, FFN conv_2 -> LN1 of the next block, long-skip conv -> LN1, out-proj -> LN2.
int run_estimator(st_engine* e, const Plan& p, const float* mask, int ev, hipStream_t s) {
    DitState* dit = dit_of(e);
    const int C = dit->C, F = dit->F, L = dit->L, N = p.N, T = p.T;
    const int64_t rowsC = (int64_t)N * T * C;
    const bool cap = e->capture;
    // What the text encoder's blocks leave out of the decoder's, said once:
    const bool dec = e->kind == KIND_DECODER;
    const bool film = dec;       // FiLM in front of every LN1, and in_proj to carry block 0's (else: the stand-alone LN kernel)
    const bool skips = dec;      // U-Net long skips: skip16 copies out of the first half, long-skip convs into the second
    const bool dec_fast_paths = dec;      // decoder-only paths not yet passed for the text encoder: the weight-stationary out-projection,
                                          // the fused FFN, split q / k operands, the lse statistic, ragged tile skipping, x3's dead fp32 copy
    const bool split_qk = dec_fast_paths && dit->attn_split;
    const bool ragged = dec_fast_paths && e->tile.ragged_skip && !cap;
    const int ln1_by_ffn = skips ? L / 2 : L;      // blocks below this take their LN1 from the previous block's conv_2 (the others from their long-skip conv)
    auto ada_of = [&](int i) { return p.ada + (size_t)i * N * 6 * C; };
    // [FiLM_i +] LN1_i + modulate (start of block i) fused into the producing GEMM
    auto fuse_ln1 = [&](ConvGemmArgs& a, int i) {
        a.ln_film = nullptr; a.ln_film_stride = 0; a.ln_film_mod = 1;
        if (film) {
            const float* fb = p.film + (size_t)i * p.n_t * 2 * C;
            if (ev >= 0) a.ln_film = fb + (size_t)ev * 2 * C;
            else         { a.ln_film = fb; a.ln_film_stride = 2 * C; a.ln_film_mod = p.B; }
        }
        a.ln_ada = ada_of(i); a.ln_ada_stride = 6 * C; a.ln_shift_off = 0; a.ln_scale_off = C;
        a.ln_mask_out = 0; a.ln_h16 = p.h16; a.mask = mask;
    };
    if (film) {   // in_proj: X = Wx.x + (Wc.cond + b); also the first long-skip (estimator.py:120-121,129).  The fp32 ODE state
        // enters as the operand pair (x_hi, x_lo): K = [x_hi | x_lo | x_hi] against [W_hi | W_hi | W_lo]
        ConvGemmArgs a = base_args(e, p, dit->inx, N);
        a.a0 = p.x16; a.c0 = dit->Mp; a.a0_mod = p.B; a.a1 = p.x16lo; a.c1 = dit->Mp; a.a1_mod = p.B; a.c2 = dit->Mp;
        a.bias = nullptr;
        a.add32 = p.cpart; a.add_clamp = p.B;
        a.out32 = p.X; a.out16 = p.skip16[0];
        fuse_ln1(a, 0);
        ProfScope ps(e, s, PC_INPROJ, conv_flops(p, dit->inx, N));
        HIPCHK(e, gemm(e, 1, EPI_F32, a, s));
    } else {      // no GEMM in front of block 0: its LN1 + modulate as a kernel of its own
        FilmLnArgs a; memset(&a, 0, sizeof(a));
        a.X = p.X; a.h16 = p.h16; a.film = nullptr; a.film_mod = 1;
        a.ada = ada_of(0); a.ada_stride = 6 * C; a.shift_off = 0; a.scale_off = C;
        a.mask = mask; a.mask_mod = p.B; a.mask_out = 0; a.T = T; a.rows = N * T;
        ProfScope ps(e, s, PC_FILM_LN1, 0);
        HIPCHK(e, launch_film_ln(e->dt, a, s));
    }
    if (film && cap) capture(e, "h0", p.skip16[0], rowsC, true, s);
    for (int i = 0; i < L; ++i) {
        const std::string bn = "b" + std::to_string(i) + ".";
        const float* ada_i = ada_of(i);
        if (skips && i >= L / 2) {   // U-Net long skip merge (estimator.py:131-132)
            const int j = i - L / 2;
            ConvGemmArgs a = base_args(e, p, dit->lsc[j], N);
            a.a0 = p.cur16; a.c0 = C; a.a1 = p.skip16[L - 1 - i]; a.c1 = C;
            a.out32 = p.X;
            fuse_ln1(a, i);
            ProfScope ps(e, s, PC_LSC, conv_flops(p, dit->lsc[j], N));
            if (!(dit->skip_mask >> PC_LSC & 1)) HIPCHK(e, gemm(e, 3, EPI_F32, a, s));
        }
        if (cap) { capture(e, bn + "x1", p.X, rowsC, false, s); capture(e, bn + "h1", p.h16, rowsC, true, s); }
        {   // q, k, v projections + RoPE (diffusion_transformer.py:59-61,74-75)
            ConvGemmArgs a = base_args(e, p, dit->qkv[i], N);
            a.a0 = p.h16; a.c0 = C;
            a.q = p.q16; a.k = p.k16; a.vt = p.vt16; a.rope_cos = dit->rope_cos; a.rope_sin = dit->rope_sin;
            if (split_qk) { a.q_lo = p.q16lo; a.k_lo = p.k16lo; }      // (the generic tile writes the residual planes; the weight-stationary kernel has no room for them)
            a.Tp = p.Tp; a.n_heads = dit->H;
            if ((int)dit->qkv_frag.size() == L) a.w_frag = dit->qkv_frag[i];
            a.qscale = 1.4426950408889634f / sqrtf((float)(C / dit->H));
            ProfScope ps(e, s, PC_QKV, conv_flops(p, dit->qkv[i], N));
            if (!(dit->skip_mask >> PC_QKV & 1)) HIPCHK(e, gemm(e, 1, EPI_QKV, a, s));
        }
        if (cap) {
            capture(e, bn + "q", p.q16, rowsC, true, s); capture(e, bn + "k", p.k16, rowsC, true, s);
            capture(e, bn + "vt", p.vt16, (int64_t)N * C * p.Tp, true, s);
        }
        {
            AttnArgs a; memset(&a, 0, sizeof(a));
            a.q = p.q16; a.k = p.k16; a.vt = p.vt16; a.out = p.ao16; a.kbias = p.kbias; a.mask_mod = p.B; a.zeros = e->zeros;
            a.kv_end = p.kv_end; a.n_full = p.n_full; a.T = T; a.Tp = p.Tp; a.H = dit->H; a.n_items = N;
            a.small_max_blocks = dit->conc == 1 ? dit->attn_small_blocks : 0;
            if (split_qk) { a.q_lo = p.q16lo; a.k_lo = p.k16lo; }
            if (dec_fast_paths) a.lse_max = dit->lse_cells;
            if (ragged) a.t_lim = p.t_lim;
            ProfScope ps(e, s, PC_ATTN, 4.0 * (double)N * dit->H * (double)T * T * (C / dit->H));
            if (!(dit->skip_mask >> PC_ATTN & 1)) HIPCHK(e, launch_attention(e->dt, a, s));
        }
        if (cap) capture(e, bn + "attn", p.ao16, rowsC, true, s);
        // Big grids: the whole FFN as ONE kernel, u never leaves the CU (ffn_fused.h; bit-identical to the two launches below).
        // Debug capture keeps the two-kernel path (it taps u).
        const bool fused = dec_fast_paths && dit->fused_ffn && !cap && (int)dit->ffn_stream.size() == L && dit->ffn_stream[i] &&
                           (int64_t)dit->conc * N * ((T + kFfnFusedFrames - 1) / kFfnFusedFrames) >= e->tile.big_min_blocks;
        void* h2buf = fused ? p.h2_16 : p.h16;
        {   // out projection, gate, mask, residual (diffusion_transformer.py:65,111) + LN2, modulate, mask (:112,26)
            ConvGemmArgs a = base_args(e, p, dit->oproj[i], N);
            a.a0 = p.ao16; a.c0 = C; a.mask = mask; a.gate = ada_i + 2 * C; a.gate_stride = 6 * C; a.out32 = p.X;
            a.ln_h16 = h2buf; a.ln_film = nullptr; a.ln_film_mod = 1;
            a.ln_ada = ada_i; a.ln_ada_stride = 6 * C; a.ln_shift_off = 3 * C; a.ln_scale_off = 4 * C; a.ln_mask_out = 1;
            if (dec_fast_paths && (int)dit->oproj_frag.size() == L && !cap) a.w_frag = dit->oproj_frag[i];
            ProfScope ps(e, s, PC_OPROJ, conv_flops(p, dit->oproj[i], N));
            if (!(dit->skip_mask >> PC_OPROJ & 1)) HIPCHK(e, gemm(e, 1, EPI_RESGATE, a, s));
        }
        if (cap) { capture(e, bn + "x2", p.X, rowsC, false, s); capture(e, bn + "h2", p.h16, rowsC, true, s); }
        if (!fused) {   // FFN conv_1 + SiLU + mask (diffusion_transformer.py:26-28)
            ConvGemmArgs a = base_args(e, p, dit->ffn1[i], N);
            a.a0 = p.h16; a.c0 = C; a.mask = mask; a.flags = GF_SILU | GF_MASK; a.out16 = p.u16;
            ProfScope ps(e, s, PC_FFN1, conv_flops(p, dit->ffn1[i], N));
            HIPCHK(e, gemm(e, 3, EPI_ACT16, a, s));
        }
        if (cap) capture(e, bn + "u", p.u16, (int64_t)N * T * F, true, s);
        void* copy16 = (skips && i + 1 < L / 2) ? p.skip16[i + 1] : p.cur16;
        {   // FFN conv_2, mask, gate, residual (diffusion_transformer.py:29-30,112) [+ FiLM/LN1 of block i+1]
            ConvGemmArgs a = base_args(e, p, dit->ffn2[i], N);
            a.a0 = p.u16; a.c0 = F; a.mask = mask; a.gate = ada_i + 5 * C; a.gate_stride = 6 * C; a.out32 = p.X;
            if (fused) { a.a0 = h2buf; a.c0 = C; a.w = dit->ffn_stream[i]; a.bias1 = dit->ffn1[i].bias; a.cmid = F; a.flags = GF_SILU | GF_MASK; }
            a.out16 = copy16;
            if (i + 1 == L) a.out16_lo = p.cur16lo;        // operand pair of final_proj / proj
            if (i + 1 < ln1_by_ffn) fuse_ln1(a, i + 1);    // the decoder's blocks >= L/2 start with the long-skip conv instead
            // ... which rebuilds the residual stream from the 16-bit operands (and final_proj reads only those): from
            // block L/2 - 1 on the fp32 copy of x3 is dead, so it is not written (40 % of this epilogue's HBM bytes)
            else if (dec_fast_paths && !cap) a.out32_readonly = 1;
            ProfScope ps(e, s, PC_FFN2, conv_flops(p, dit->ffn2[i], N) + (fused ? conv_flops(p, dit->ffn1[i], N) : 0.0));
            if (dit->skip_mask >> PC_FFN2 & 1) {}
            else if (fused && dit->fused_ffn == 3) HIPCHK(e, launch_ffn_wino_f16(a, s));
            else if (fused) HIPCHK(e, e->dt == DT_BF16 ? launch_ffn_fused_bf16(a, s) : launch_ffn_fused_f16(a, s));
            else HIPCHK(e, gemm(e, 3, EPI_RESGATE, a, s));
        }
        if (cap) {
            if (film && i + 1 < ln1_by_ffn) capture(e, bn + "x3", copy16, rowsC, true, s);   // X already holds the FiLM'd value
            else capture(e, bn + "x3", p.X, rowsC, false, s);
        }
    }
    {   // final_proj (estimator.py:136-138) / mu_x = proj(x) * x_mask (text_encoder.py:42); block output is already zero on padded frames
        ConvGemmArgs a = base_args(e, p, dit->fin, N);
        a.a0 = p.cur16; a.c0 = C; a.a1 = p.cur16lo; a.c1 = C; a.c2 = C; a.mask = mask; a.flags = GF_MASK; a.out32 = p.v32;
        ProfScope ps(e, s, PC_FINAL, conv_flops(p, dit->fin, N));
        HIPCHK(e, gemm(e, 1, EPI_F32, a, s));
    }
    if (cap) capture(e, "v", p.v32, (int64_t)N * T * dit->Mp, false, s);
    return ST_OK;
}

int check_handle(st_engine* e, Kind kind) {
    if (!e) return ST_ERR_INVALID;
    if (e->kind != kind)
        return e->fail(ST_ERR_STATE, std::string("this handle is not a ") + kKinds[kind].what + " (" + kKinds[kind].creator + ")");
    return ST_OK;
}

int check_finalized(st_engine* e) {
    return e->finalized ? ST_OK : e->fail(ST_ERR_STATE, "st_finalize() has not been called after loading parameters");
}

int check_sizes(st_engine* e, int B, int T, const char* t_name) {
    return B >= 1 && T >= 1 ? ST_OK : e->fail(ST_ERR_INVALID, std::string("B and ") + t_name + " must be >= 1");
}

int check_dropout(st_engine* e, float p_dropout) {
    return p_dropout >= 0.0f && p_dropout < 1.0f ? ST_OK : e->fail(ST_ERR_INVALID, "p_dropout must be in [0, 1)");
}

int check_ready(st_engine* e, Kind kind, int B, int T) {
    if (!e) return ST_ERR_INVALID;
    int rc = check_finalized(e); if (rc) return rc;
    if ((rc = check_sizes(e, B, T))) return rc;
    const DitState* dit = dit_or_null(e);
    if (dit && (int64_t)2 * B * T * dit->F >= (int64_t)1 << 31) return e->fail(ST_ERR_INVALID, "B*T too large for 32-bit row indexing");
    return check_handle(e, kind);
}

int new_handle(Kind kind, int device, std::unique_ptr<KindState> state, st_engine** out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { g_create_error = "no such HIP device"; return ST_ERR_HIP; }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return ST_ERR_HIP; }
    st_engine* e = new st_engine();
    e->device = device; e->kind = kind; e->state = std::move(state);
    *out = e;
    return ST_OK;
}

int KindState::repack(st_engine* e, hipStream_t) { return e->fail(ST_ERR_UNSUPPORTED, repack_refusal); }

void free_owned(st_engine* e) {
    for (void* p : e->owned) hipFree(p);
    e->owned.clear(); e->weight_bytes = 0;
}

// st_load_param / st_bind_param: the table row of `name`, if the caller's shape is the expected one
static int find_param(st_engine* e, const char* name, const float* data, const int64_t* shape, int ndim, Param** out) {
    if (!e) return ST_ERR_INVALID;
    if (!name || !data || !shape) return e->fail(ST_ERR_INVALID, "null argument");
    auto it = e->params.find(name);
    if (it == e->params.end()) return e->fail(ST_ERR_INVALID, std::string("unexpected parameter name: ") + name);
    Param& p = it->second;
    bool ok = (int)p.shape.size() == ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = p.shape[i] == shape[i];
    if (!ok) return e->fail(ST_ERR_INVALID, std::string("shape mismatch for ") + name);
    *out = &p;
    return ST_OK;
}

}  // namespace sthost

// ============================================================================================ C ABI
extern "C" {

int st_abi_version(void) { return ST_ABI_VERSION; }

static int create_engine(const st_config* cfg, Kind kind, int n_vocab, int device, st_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ST_ERR_INVALID; }
    auto bad = [&](const char* m) { g_create_error = m; return ST_ERR_INVALID; };
    // the reference's own assertions
    if (kind == KIND_DECODER && (cfg->n_layers % 2 != 0 || cfg->n_layers < 2 || cfg->n_layers > 16))
        return bad("n_layers must be even (estimator.py:92) and in [2, 16]");
    if (kind == KIND_TEXT_ENCODER && (cfg->n_layers < 1 || cfg->n_layers > 16)) return bad("n_layers must be in [1, 16]");
    if (kind == KIND_TEXT_ENCODER && n_vocab < 1) return bad("n_vocab must be >= 1");
    if (cfg->hidden_channels % 2 != 0) return bad("SinusoidalPosEmb requires dim to be even (estimator.py:39)");
    if (cfg->n_heads < 1 || cfg->hidden_channels % cfg->n_heads != 0)
        return bad("channels % n_heads != 0 (diffusion_transformer.py:35)");
    // limits of this native build
    if (cfg->hidden_channels != 256) { g_create_error = "native kernels are built for hidden_channels == 256"; return ST_ERR_UNSUPPORTED; }
    if (cfg->hidden_channels / cfg->n_heads != 64) { g_create_error = "native kernels are built for head_dim == 64"; return ST_ERR_UNSUPPORTED; }
    if (cfg->kernel_size != 3) { g_create_error = "native kernels are built for kernel_size == 3"; return ST_ERR_UNSUPPORTED; }
    if (cfg->filter_channels % 128 != 0 || cfg->filter_channels < 128) { g_create_error = "filter_channels must be a multiple of 128"; return ST_ERR_UNSUPPORTED; }
    if (cfg->noise_channels < 1 || cfg->noise_channels > 1024) return bad("noise_channels out of range");
    if (cfg->gin_channels < 4 || cfg->gin_channels % 4 != 0) return bad("gin_channels must be a positive multiple of 4");
    if (cfg->operand_dtype != ST_OPERAND_BF16 && cfg->operand_dtype != ST_OPERAND_F16) return bad("operand_dtype");
    st_engine* e = nullptr;
    if (int rc = new_handle(kind, device, std::make_unique<DitState>(), &e)) return rc;
    DitState* dit = dit_of(e);
    dit->cfg = *cfg; dit->dec = kind == KIND_DECODER;
    e->dt = cfg->operand_dtype == ST_OPERAND_BF16 ? DT_BF16 : DT_F16;
    dit->M = cfg->noise_channels; dit->Mp = (dit->M + 127) / 128 * 128;
    dit->C = cfg->hidden_channels; dit->F = cfg->filter_channels; dit->H = cfg->n_heads; dit->L = cfg->n_layers;
    dit->K = cfg->kernel_size; dit->G = cfg->gin_channels;
    dit->n_vocab = n_vocab;
    if (const char* mb = getenv("ST_BIG_MIN_BLOCKS")) e->tile.big_min_blocks = atoi(mb);
    if (const char* v = getenv("ST_PHASED")) e->tile.phased = atoi(v);
    if (const char* v = getenv("ST_FUSED_FFN")) dit->fused_ffn = atoi(v);
    // Default = the direct fused kernel, bit-identical to the two-kernel path.  Round 5 put the Winograd form on trial with O(1) adaLN
    // gates at B = 32 x T = 1000 (tools/parity_trained.py): one evaluation 8.8e-4 against the direct kernel's 7.3e-4 -- too close to the
    // 1e-3 bar for a 1.45 % gain, so it is opt-in (ST_FUSED_FFN=3; f16 only: it forms its operands with packed f16 adds).
    if (dit->fused_ffn < 0 || dit->fused_ffn > 3 || dit->fused_ffn == 2) dit->fused_ffn = 1;
    if (dit->fused_ffn == 3 && e->dt != DT_F16) dit->fused_ffn = 1;
    if (const char* v = getenv("ST_RAGGED_SKIP")) e->tile.ragged_skip = atoi(v);
#ifdef ST_DEVTOOLS      // developer builds only (ST_BUILD_DEFS=-DST_DEVTOOLS): a shipping library must not return garbage because of an environment variable
    if (const char* v = getenv("ST_SKIP_CLASSES")) dit->skip_mask = (unsigned)strtoul(v, nullptr, 0);
#endif
    if (const char* v = getenv("ST_QKV_WS")) dit->qkv_ws = atoi(v);
    if (const char* v = getenv("ST_QKV_WS_MIN_TILES")) dit->qkv_ws_min_tiles = atoi(v);
    if (const char* v = getenv("ST_OPROJ_WS")) dit->oproj_ws = atoi(v);
    if (const char* v = getenv("ST_OPROJ_WS_MIN_TILES")) dit->oproj_ws_min_tiles = atoi(v);
    if (const char* v = getenv("ST_QKV_RC1")) dit->qkv_rc1 = atoi(v);     // 0: compute every padded frame tile (A/B runs)
    if (const char* v = getenv("ST_SMALL_GRID")) {      // 0: none of the small-grid variants (split-K convs, 64-frame tiles,
        if (atoi(v) == 0) {                               // key-split attention): results independent of the batch composition
            e->tile.splitk_target = 0; e->tile.small_tiles = 0; dit->attn_small_blocks = 0;
        }
    }
    build_param_table(e);
    if (hipMalloc((void**)&e->tile.kpart, kSplitKBytes) == hipSuccess) e->tile.kpart_bytes = kSplitKBytes; else e->tile.kpart = nullptr;
    if (hipMalloc(&dit->sink, 65536) != hipSuccess) dit->sink = nullptr;      // (without it the q/k/v projection stays on the generic tile)
    if (hipMalloc((void**)&dit->lse_cells, kLseCells * 64) != hipSuccess ||
        hipMemsetD32((hipDeviceptr_t)dit->lse_cells, (int)0x80000000, kLseCells * 16) != hipSuccess) { (void)hipGetLastError(); dit->lse_cells = nullptr; }
    if (hipMalloc(&e->zeros, 256) != hipSuccess || hipMemset(e->zeros, 0, 256) != hipSuccess) {
        g_create_error = "hipMalloc failed";
        delete e;
        return ST_ERR_HIP;
    }
    if (hipHostMalloc((void**)&dit->status_host, sizeof(int), hipHostMallocMapped) == hipSuccess &&
        hipHostGetDevicePointer((void**)&dit->status_dev, dit->status_host, 0) == hipSuccess) *dit->status_host = 0;
    else { (void)hipGetLastError(); dit->status_host = nullptr; dit->status_dev = nullptr; }      // (guard unavailable: st_output_status says so)
    *out = e;
    return ST_OK;
}

int st_create(const st_config* cfg, int device, st_engine** out) { return create_engine(cfg, KIND_DECODER, 0, device, out); }

int st_create_text_encoder(const st_config* cfg, int n_vocab, int device, st_engine** out) {
    return create_engine(cfg, KIND_TEXT_ENCODER, n_vocab, device, out);
}

void st_destroy(st_engine* e) {
    if (!e) return;
    hipSetDevice(e->device);
    hipDeviceSynchronize();
    delete e;
}

const char* st_last_error(const st_engine* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int st_num_params(const st_engine* e) { return e ? (int)e->params.size() : ST_ERR_INVALID; }

int st_param_info(const st_engine* e, int index, const char** name, int64_t* shape) {
    if (!e || index < 0 || index >= (int)e->params.size()) return ST_ERR_INVALID;
    auto it = e->params.begin();
    std::advance(it, index);
    if (name) *name = it->first.c_str();
    if (shape) for (size_t i = 0; i < it->second.shape.size(); ++i) shape[i] = it->second.shape[i];
    return (int)it->second.shape.size();
}

int st_load_param(st_engine* e, const char* name, const float* data, const int64_t* shape, int ndim) {
    Param* pp = nullptr;
    if (int rc = find_param(e, name, data, shape, ndim, &pp)) return rc;
    Param& p = *pp;
    HIPCHK(e, hipSetDevice(e->device));
    if (p.borrowed) { p.dev = nullptr; p.borrowed = false; }
    if (!p.dev) { HIPCHK(e, hipMalloc((void**)&p.dev, (size_t)p.numel() * 4)); e->state->params_moved(); }
    HIPCHK(e, hipMemcpy(p.dev, data, (size_t)p.numel() * 4, hipMemcpyDefault));
    p.loaded = true;
    e->finalized = false;
    return ST_OK;
}

int st_bind_param(st_engine* e, const char* name, const float* data, const int64_t* shape, int ndim) {
    Param* pp = nullptr;
    if (int rc = find_param(e, name, data, shape, ndim, &pp)) return rc;
    Param& p = *pp;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, data) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != e->device) {
        (void)hipGetLastError();
        return e->fail(ST_ERR_INVALID, std::string("st_bind_param needs a pointer to memory of the engine's device: ") + name);
    }
    if (p.dev && !p.borrowed) { HIPCHK(e, hipSetDevice(e->device)); HIPCHK(e, hipDeviceSynchronize()); hipFree(p.dev); }
    p.dev = const_cast<float*>(data);
    p.borrowed = true;
    p.loaded = true;
    e->finalized = false;
    e->state->params_moved();
    return ST_OK;
}

int st_repack(st_engine* e, void* stream) {
    if (!e) return ST_ERR_INVALID;
    return e->state->repack(e, (hipStream_t)stream);
}

int st_finalize(st_engine* e) {
    if (!e) return ST_ERR_INVALID;
    HIPCHK(e, hipSetDevice(e->device));
    for (auto& kv : e->params)
        if (!kv.second.loaded) return e->fail(ST_ERR_STATE, "parameter not loaded: " + kv.first);
    HIPCHK(e, hipDeviceSynchronize());
    if (int rc = e->state->finalize(e)) return rc;
    e->finalized = true;
    return ST_OK;
}

}  // extern "C"

st_engine::~st_engine() {
    state.reset();
    for (auto& kv : params) if (kv.second.dev && !kv.second.borrowed) hipFree(kv.second.dev);
    for (void* p : owned) hipFree(p);
    for (auto& kv : caps) if (kv.second.dev) hipFree(kv.second.dev);
    prof_collect(this);
    for (hipEvent_t ev : ev_pool) hipEventDestroy(ev);
    if (ws) hipFree(ws);
    if (zeros) hipFree(zeros);
    if (tile.kpart) hipFree(tile.kpart);
}

namespace sthost {
DitState::~DitState() {
    drop_graphs();
    train_destroy(this);
    if (gstream) hipStreamDestroy(gstream);
    part_streams.destroy();
    if (adams_buf) hipFree(adams_buf);
    if (pk_fwd.dev) hipFree(pk_fwd.dev);
    if (pk_T.dev) hipFree(pk_T.dev);
    if (rope_cos) hipFree(rope_cos);
    if (rope_sin) hipFree(rope_sin);
    if (sink) hipFree(sink);
    if (lse_cells) hipFree(lse_cells);
    if (status_host) hipHostFree(status_host);
}

int DitState::finalize(st_engine* e) {
    params_moved();        // a re-bind may have changed the fp32 parameter pointers
    int rc = pack_all(e, nullptr); if (rc) return rc;
    HIPCHK(e, hipDeviceSynchronize());
    train_invalidate(this);
    return ST_OK;
}

int DitState::repack(st_engine* e, hipStream_t s) {
    if (!packed_once) return e->fail(ST_ERR_STATE, "st_repack needs one earlier st_finalize (it allocates the packed buffers)");
    // A re-bind / re-load since the last st_finalize may have moved fp32 tensors: st_repack is for in-place updates only.
    if (!e->finalized && !pk_fwd.ready)
        return e->fail(ST_ERR_STATE, "st_repack after st_bind_param / st_load_param of a new pointer: call st_finalize");
    for (auto& kv : e->params)
        if (!kv.second.loaded) return e->fail(ST_ERR_STATE, "parameter not loaded: " + kv.first);
    HIPCHK(e, hipSetDevice(e->device));
    int rc = pack_all(e, s); if (rc) return rc;
    train_invalidate(this);
    e->finalized = true;
    return ST_OK;
}

int64_t DitState::device_bytes() const { return train_bytes(this); }

// A PackList (engine_dit.h): begin -> pk_push per job -> end (upload + the one launch); replay = the one launch again.
void pk_begin(DitState::PackList& L) { L.jobs.clear(); L.nblocks = 0; L.ready = false; }
void pk_push(DitState::PackList& L, PackJob j) {
    j.blk0 = L.nblocks;
    L.nblocks += pack_job_blocks(j);
    L.jobs.push_back(j);
}
static int pk_run(st_engine* e, DitState::PackList& L, hipStream_t s) {
    HIPCHK(e, launch_pack_jobs(e->dt, L.dev, (int)L.jobs.size(), L.nblocks, s));
    return ST_OK;
}
int pk_end(st_engine* e, DitState::PackList& L, hipStream_t s) {
    if (L.jobs.empty()) return ST_OK;
    if (L.dev) { HIPCHK(e, hipStreamSynchronize(s)); hipFree(L.dev); L.dev = nullptr; }
    HIPCHK(e, hipMalloc((void**)&L.dev, L.jobs.size() * sizeof(PackJob)));
    HIPCHK(e, hipMemcpyAsync(L.dev, L.jobs.data(), L.jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice, s));
    int rc = pk_run(e, L, s); if (rc) return rc;
    HIPCHK(e, hipStreamSynchronize(s));        // (pageable source; once per parameter binding)
    L.ready = true;
    return ST_OK;
}
bool pk_replay(st_engine* e, DitState::PackList& L, hipStream_t s, int* rc) {
    if (!L.ready) return false;
    *rc = pk_run(e, L, s);
    return true;
}

// Packs every convolution's weights into the 16-bit MFMA operand layouts on stream `s`.  The packed buffers are
// allocated by the first call and re-used by every later one (shapes are fixed by the configuration), so instantiated
// HIP graphs and in-flight launch sequences keep valid pointers and a re-pack is pure stream work: one launch of the
// job list the first call recorded, for as long as the parameter tensors stay where they are.
int pack_all(st_engine* e, hipStream_t s) {
    DitState* dit = dit_of(e);
    const int C = dit->C, F = dit->F, M = dit->M, Mp = dit->Mp, K = dit->K, L = dit->L;
    {
        int prc;
        if (dit->packed_once && pk_replay(e, dit->pk_fwd, s, &prc)) return prc;
    }
    DitState::PackList& PL = dit->pk_fwd;
    pk_begin(PL);
    // generic packer: (cout, cin_total, taps) source slice -> Conv with padded dims.  split: the packed K dimension
    // is [W_hi | W_hi | W_lo] (W_lo = W - float(W_hi)), the weight side of a split-precision operand
    auto pack = [&](Conv& cv, const std::string& wname, const float* bias_src, int cout, int cout_p, int cin_total,
                    int taps, int ci_off, int ci_cnt, int cin_p, bool split) -> int {
        cv.cout = cout_p; cv.cin = split ? 3 * cin_p : cin_p; cv.taps = taps; cv.split = split;
        const size_t wbytes = (size_t)cout_p * taps * cv.cin * 2;
        int rc;
        // (the zero padding is written once, at allocation: a re-pack rewrites exactly the payload elements)
        if (!cv.w) { if ((rc = dev_alloc(e, &cv.w, wbytes))) return rc; HIPCHK(e, hipMemsetAsync(cv.w, 0, wbytes, s)); }
        for (int part = 0; part < (split ? 3 : 1); ++part)
            pk_push(PL, pack_job_weight(P(e, wname), cout, cin_total, taps, ci_off, ci_cnt, cv.w, 0, cv.cin, part * cin_p, cin_p, part == 2));
        if (!cv.bias) { if ((rc = dev_alloc(e, (void**)&cv.bias, (size_t)cout_p * 4))) return rc; HIPCHK(e, hipMemsetAsync(cv.bias, 0, (size_t)cout_p * 4, s)); }
        if (bias_src) pk_push(PL, pack_job_copy(cv.bias, bias_src, cout));
        return ST_OK;
    };
    int rc;
    if (e->kind == KIND_TEXT_ENCODER) {
        if ((rc = pack(dit->fin, "proj.weight", P(e, "proj.bias"), M, Mp, C, 1, 0, C, C, true))) return rc;      // split precision: its error reaches mu_x un-gated
    } else {
    if (dit->pre.size() != 3) dit->pre.assign(3, Conv());
    if ((rc = pack(dit->pre[0], "cond_proj.0.weight", P(e, "cond_proj.0.bias"), F, F, M, K, 0, M, Mp, false))) return rc;
    if ((rc = pack(dit->pre[1], "cond_proj.2.weight", P(e, "cond_proj.2.bias"), F, F, F, K, 0, F, F, false))) return rc;
    if ((rc = pack(dit->pre[2], "cond_proj.4.weight", P(e, "cond_proj.4.bias"), C, C, F, K, 0, F, F, false))) return rc;
    // in_proj input channel order [x(M) ; cond(C)] (estimator.py:120); both halves and final_proj take
    // split-precision operands: their rounding error reaches the estimator output without a gate in between
    if ((rc = pack(dit->inx, "in_proj.weight", nullptr, C, C, C + M, 1, 0, M, Mp, true))) return rc;
    if ((rc = pack(dit->inc, "in_proj.weight", P(e, "in_proj.bias"), C, C, C + M, 1, M, C, C, true))) return rc;
    if ((rc = pack(dit->fin, "final_proj.weight", P(e, "final_proj.bias"), M, Mp, C, 1, 0, C, C, true))) return rc;
    if ((int)dit->lsc.size() != L / 2) dit->lsc.assign(L / 2, Conv());
    for (int i = 0; i < L / 2; ++i) {
        const std::string n = "lsc_layers." + std::to_string(i);
        if ((rc = pack(dit->lsc[i], n + ".weight", P(e, n + ".bias"), C, C, 2 * C, K, 0, 2 * C, 2 * C, false))) return rc;
    }
    }
    if ((int)dit->qkv.size() != L) { dit->qkv.assign(L, Conv()); dit->oproj.assign(L, Conv()); dit->ffn1.assign(L, Conv()); dit->ffn2.assign(L, Conv()); }
    for (int i = 0; i < L; ++i) {
        const std::string b = dit->blk(i);
        Conv& q = dit->qkv[i];
        q.cout = 3 * C; q.cin = C; q.taps = 1;
        if (!q.w && (rc = dev_alloc(e, &q.w, (size_t)3 * C * C * 2))) return rc;
        if (!q.bias && (rc = dev_alloc(e, (void**)&q.bias, (size_t)3 * C * 4))) return rc;
        int r = 0;
        const bool frag = C == 256 && dit->H == 4;      // the weight-stationary kernel's copy (qkv_ws.hip)
        if (frag) {
            if ((int)dit->qkv_frag.size() != L) dit->qkv_frag.assign(L, nullptr);
            if (!dit->qkv_frag[i] && (rc = dev_alloc(e, &dit->qkv_frag[i], (size_t)3 * C * C * 2))) return rc;
        }
        for (const char* nm : {"q", "k", "v"}) {
            const std::string n = b + "attn.conv_" + nm;
            if (frag) pk_push(PL, pack_job_qkv_frag(P(e, n + ".weight"), r, dit->qkv_frag[i]));
            pk_push(PL, pack_job_weight(P(e, n + ".weight"), C, C, 1, 0, C, q.w, r * C, C, 0, C, 0));
            pk_push(PL, pack_job_copy(q.bias + (size_t)r * C, P(e, n + ".bias"), C));
            ++r;
        }
        if ((rc = pack(dit->oproj[i], b + "attn.conv_o.weight", P(e, b + "attn.conv_o.bias"), C, C, C, 1, 0, C, C, false))) return rc;
        if (frag) {      // the weight-stationary out-projection kernel's copy (oproj_ws.hip): plane 0 of the same fragment order
            if ((int)dit->oproj_frag.size() != L) dit->oproj_frag.assign(L, nullptr);
            if (!dit->oproj_frag[i] && (rc = dev_alloc(e, &dit->oproj_frag[i], (size_t)C * C * 2))) return rc;
            pk_push(PL, pack_job_qkv_frag(P(e, b + "attn.conv_o.weight"), 0, dit->oproj_frag[i]));
        }
        if ((rc = pack(dit->ffn1[i], b + "mlp.conv_1.weight", P(e, b + "mlp.conv_1.bias"), F, F, C, K, 0, C, C, false))) return rc;
        if ((rc = pack(dit->ffn2[i], b + "mlp.conv_2.weight", P(e, b + "mlp.conv_2.bias"), C, C, F, K, 0, F, F, false))) return rc;
        if (e->kind == KIND_DECODER && C == 256 && K == 3 && F % 256 == 0 && F <= 2048) {      // the fused FFN kernel's weight stream (ffn_fused.h)
            if ((int)dit->ffn_stream.size() != L) dit->ffn_stream.assign(L, nullptr);
            if (!dit->ffn_stream[i] && (rc = dev_alloc(e, &dit->ffn_stream[i], (size_t)2 * F * C * K * 2))) return rc;
            for (int st = 0; st < 2; ++st) {
                const float* src = P(e, b + (st ? "mlp.conv_2.weight" : "mlp.conv_1.weight"));
                // (ST_FUSED_FFN=3, ffn_wino.h: three transformed planes per tap triple)
                pk_push(PL, dit->fused_ffn == 3 ? pack_job_ffn_wino(src, st, F, dit->ffn_stream[i]) : pack_job_ffn_stream(src, st, F, dit->ffn_stream[i]));
            }
        }
    }
    dit->packed_once = true;
    return pk_end(e, PL, s);
}
}  // namespace sthost

extern "C" {

int st_estimator_forward(st_engine* e, const float* t, int t_len, const float* x, const float* mu,
                         const float* mask, const float* c, float* out, int B, int T, void* stream) {
    int rc = check_ready(e, KIND_DECODER, B, T); if (rc) return rc;
    DitState* dit = dit_of(e);
    if (!t || !x || !mu || !mask || !c || !out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if (t_len != 1 && t_len != B) return e->fail(ST_ERR_INVALID, "t must have 1 or B elements");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    Plan p;
    if ((rc = make_plan(e, B, T, false, t_len, &p))) return rc;
    dit->arena_poisoned(e);      // an earlier call produced NaN / Inf: its stale frames must not be trusted (re-zero below)
    if ((rc = arena_fresh(e, layout_sig(1, B, T, 0, t_len, 1), layout_plan(e, B, T, false, t_len, 0, &p), s))) return rc;
    bind_plan(e, &p);
    if ((rc = ensure_rope(e, T, s))) return rc;
    {
        ProfScope ps(e, s, PC_PREP, 0);
        HIPCHK(e, launch_mask_prep(mask, B, T, p.Tp, p.n_full, p.kv_end, p.kbias, p.t_lim, s));
        HIPCHK(e, hipMemsetAsync(p.v32, 0, (size_t)p.N * T * dit->Mp * 4, s));      // frames of skipped tiles: v = 0 (estimator.py:138)
        HIPCHK(e, launch_to_time_major(e->dt, mu, B, dit->M, T, dit->Mp, nullptr, p.mu16, nullptr, s));
        HIPCHK(e, launch_to_time_major(e->dt, x, B, dit->M, T, dit->Mp, nullptr, p.x16, p.x16lo, s));
        HIPCHK(e, hipMemcpyAsync(p.cvec, c, (size_t)B * dit->G * 4, hipMemcpyDeviceToDevice, s));
        HIPCHK(e, hipMemcpyAsync(p.tvals, t, (size_t)t_len * 4, hipMemcpyDeviceToDevice, s));
    }
    if ((rc = run_prenet(e, p, s))) return rc;
    if ((rc = run_adaln(e, p, s))) return rc;
    if ((rc = run_time_tables(e, p, s))) return rc;
    if ((rc = run_estimator(e, p, mask, t_len == 1 ? 0 : -1, s))) return rc;
    {
        ProfScope ps(e, s, PC_PREP, 0);
        HIPCHK(e, launch_from_time_major(p.v32, B, dit->M, T, dit->Mp, out, s, dit->status_dev));
    }
    return ST_OK;
}

int st_text_encoder_forward(st_engine* e, const int64_t* tokens, const int64_t* lengths, const float* c,
                            float* x_out, float* mu_out, float* mask_out, int B, int T, void* stream) {
    int rc = check_ready(e, KIND_TEXT_ENCODER, B, T); if (rc) return rc;
    DitState* dit = dit_of(e);
    if (!tokens || !lengths || !c || !x_out || !mu_out || !mask_out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    Plan p;
    if ((rc = make_plan(e, B, T, false, 1, &p))) return rc;
    e->ws_sig = 0;         // (the text encoder computes every frame; whatever uses the arena next re-zeroes it)
    if ((rc = ensure_rope(e, T, s))) return rc;
    {
        ProfScope ps(e, s, PC_PREP, 0);
        // embedding * sqrt(C) * mask -> residual stream; the (B,1,T) mask is written straight into the caller's tensor
        HIPCHK(e, launch_embed_tokens((const long long*)tokens, (const long long*)lengths, P(e, "emb.weight"), dit->n_vocab,
                                      dit->C, sqrtf((float)dit->C), B, T, p.X, mask_out, s));
        HIPCHK(e, launch_mask_prep(mask_out, B, T, p.Tp, p.n_full, p.kv_end, p.kbias, nullptr, s));
        HIPCHK(e, launch_cvec_prep(c, nullptr, B, dit->G, p.cvec, s));
    }
    if ((rc = run_adaln(e, p, s))) return rc;
    if ((rc = run_estimator(e, p, mask_out, 0, s))) return rc;
    {
        ProfScope ps(e, s, PC_PREP, 0);
        HIPCHK(e, launch_from_time_major(p.X, B, dit->C, T, dit->C, x_out, s));
        HIPCHK(e, launch_from_time_major(p.v32, B, dit->M, T, dit->Mp, mu_out, s));
    }
    return ST_OK;
}

// ---- duration -> alignment -> mu_y: stateless helpers (no engine handle; errors through st_last_error(NULL))
static int align_fail(int code, const char* msg) { g_create_error = msg; return code; }

int st_durations(const float* logw, const float* x_mask, float length_scale, int B, int Tx, float* w_ceil, float* cum,
                 int64_t* y_lengths, void* stream) {
    if (!logw || !x_mask || !w_ceil || !cum || !y_lengths) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || Tx < 1) return align_fail(ST_ERR_INVALID, "B and Tx must be >= 1");
    if (launch_durations(logw, x_mask, length_scale, B, Tx, w_ceil, cum, (long long*)y_lengths, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "durations kernel launch failed");
    return ST_OK;
}

int st_generate_path(const float* duration, const float* mask, int B, int Tx, int Ty, float* cum_scratch, float* path, void* stream) {
    if (!duration || !mask || !cum_scratch || !path) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || Tx < 1 || Ty < 1 || B > 65535 || Tx > 65535) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (launch_cumsum_rows(duration, B, Tx, cum_scratch, (hipStream_t)stream) != hipSuccess ||
        launch_path(cum_scratch, mask, B, Tx, Ty, path, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "generate_path kernel launch failed");
    return ST_OK;
}

int st_align(const float* cum, const float* x_mask, const int64_t* y_lengths, const float* mu_x, int B, int M, int Tx, int Ty,
             float* attn, float* mu_y, float* y_mask, void* stream) {
    if (!cum || !x_mask || !y_lengths || !mu_x || !mu_y) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || M < 1 || Tx < 1 || Ty < 1 || B > 65535) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (launch_align(cum, x_mask, (const long long*)y_lengths, mu_x, B, M, Tx, Ty, attn, mu_y, y_mask, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "align kernel launch failed");
    return ST_OK;
}

// ---- monotonic alignment search: stateless helpers (errors through st_last_error(NULL))
int64_t st_maximum_path_workspace_bytes(int B, int Ty, int Tx) { return (int64_t)mas_workspace_bytes(B, Ty, Tx); }

int st_maximum_path(const float* neg_cent, const int32_t* t_y, const int32_t* t_x, int B, int Ty, int Tx, float* path,
                    int32_t* durations, void* workspace, void* stream) {
    if (!neg_cent || !t_y || !t_x || !path) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || Ty < 1 || Tx < 1 || B > 65535) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (Tx > kMasMaxTx) return align_fail(ST_ERR_UNSUPPORTED, "maximum_path supports Tx <= 4096 (one row per wave in registers)");
    if (mas_workspace_bytes(B, Ty, Tx) && !workspace)
        return align_fail(ST_ERR_INVALID, "this shape needs st_maximum_path_workspace_bytes() of workspace");
    if (launch_mas_path(neg_cent, t_y, t_x, B, Ty, Tx, path, durations, workspace, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "maximum_path kernel launch failed");
    return ST_OK;
}

int st_mas_neg_cent(const float* mu_x, const float* y, int B, int D, int Tx, int Ty, float* neg_cent, void* stream) {
    if (!mu_x || !y || !neg_cent) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || D < 1 || Tx < 1 || Ty < 1 || B > 65535 || (Ty + 63) / 64 > 65535) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (launch_mas_neg_cent(mu_x, y, B, D, Tx, Ty, neg_cent, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "neg_cent kernel launch failed");
    return ST_OK;
}

// ---- training side of the alignment step: stateless helpers (errors through st_last_error(NULL))
int st_align_train_scratch_floats(int B, int M, int Ty) {
    if (B < 1 || M < 1 || Ty < 1) return ST_ERR_INVALID;
    return align_train_scratch_floats(B, M, Ty);
}

static int align_train_shape(int B, int M, int Tx, int Ty) {
    if (B < 1 || M < 1 || Tx < 1 || Ty < 1 || B > 65535 || (M + kAlignTrainChannels - 1) / kAlignTrainChannels > 65535 ||
        align_train_scratch_floats(B, M, Ty) < 0)
        return align_fail(ST_ERR_INVALID, "shape out of range");
    if (Tx > kAlignTrainMaxTx) return align_fail(ST_ERR_UNSUPPORTED, "the alignment training kernels support Tx <= 4096 (one item's running sum in LDS)");
    return ST_OK;
}

int st_align_train_forward(const int32_t* durations, const float* x_mask, const float* y_mask, const float* mu_x, const float* y,
                           const float* fake_content, const float* keep, int B, int M, int Tx, int Ty, int32_t* frame_token,
                           float* mu_y, float* mu_y_masked, float* scratch, float* prior_loss, void* stream) {
    if (!durations || !x_mask || !y_mask || !mu_x || !y || !frame_token || !mu_y_masked || !scratch || !prior_loss)
        return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (int rc = align_train_shape(B, M, Tx, Ty)) return rc;
    if (launch_align_train_forward(durations, x_mask, y_mask, mu_x, y, fake_content, keep, B, M, Tx, Ty, frame_token, mu_y, mu_y_masked,
                                   scratch, prior_loss, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "align_train_forward kernel launch failed");
    return ST_OK;
}

int st_align_train_backward(const int32_t* durations, const float* x_mask, const float* y_mask, const float* mu_x, const float* y,
                            const float* keep, const float* scratch, const float* grad_mu_y_masked, const float* grad_mu_y,
                            const float* grad_prior, int B, int M, int Tx, int Ty, float* grad_mu_x, float* grad_fake_content,
                            void* stream) {
    if (!durations || !x_mask || !mu_x || !grad_mu_x) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (grad_prior && (!y || !y_mask || !scratch)) return align_fail(ST_ERR_INVALID, "grad_prior needs y, y_mask and the forward's scratch");
    if (int rc = align_train_shape(B, M, Tx, Ty)) return rc;
    if (launch_align_train_backward(durations, x_mask, y_mask, mu_x, y, keep, scratch, grad_mu_y_masked, grad_mu_y, grad_prior, B, M, Tx,
                                    Ty, grad_mu_x, grad_fake_content, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "align_train_backward kernel launch failed");
    return ST_OK;
}

int st_duration_loss_scratch_floats(void) { return kDurLossScratchFloats; }

int st_duration_loss(const float* logw, const int32_t* durations, const float* x_mask, const int64_t* x_lengths, int B, int Tx,
                     float* logw_target, float* scratch, float* loss, void* stream) {
    if (!logw || !durations || !x_mask || !x_lengths || !scratch || !loss) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || Tx < 1) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (launch_duration_loss(logw, durations, x_mask, (const long long*)x_lengths, B, Tx, logw_target, scratch, loss, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "duration_loss kernel launch failed");
    return ST_OK;
}

int st_duration_loss_backward(const float* logw, const int32_t* durations, const float* x_mask, const float* scratch,
                              const float* grad_loss, int B, int Tx, float* grad_logw, void* stream) {
    if (!logw || !durations || !x_mask || !scratch || !grad_loss || !grad_logw) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || Tx < 1) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (launch_duration_loss_bwd(logw, durations, x_mask, scratch, grad_loss, B, Tx, grad_logw, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "duration_loss_bwd kernel launch failed");
    return ST_OK;
}

int st_output_status(st_engine* e, void* stream, int* nonfinite) {
    if (!e) return ST_ERR_INVALID;
    if (!nonfinite) return e->fail(ST_ERR_INVALID, "null argument");
    DitState* dit = dit_or_null(e);
    if (!dit || !dit->status_host) return e->fail(ST_ERR_UNSUPPORTED, "host-mapped status word unavailable on this device");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    *nonfinite = *dit->status_host != 0;
    dit->arena_poisoned(e);      // clears the word; the next call re-zeroes the arena
    return ST_OK;
}

// ---- compute_loss's own arithmetic: stateless helpers (errors through st_last_error(NULL))
int st_cfm_loss_prep(const float* x1, const float* z, const float* t_rand, float sigma_min, int B, int M, int T, float* t, float* y,
                     float* u, void* stream) {
    if (!x1 || !z || !t_rand || !t || !y || !u) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || M < 1 || T < 1 || B > 65535) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (launch_cfm_loss_prep(x1, z, t_rand, sigma_min, B, M, T, t, y, u, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "cfm_loss_prep kernel launch failed");
    return ST_OK;
}

int st_cfm_loss(const float* pred, const float* u, const float* mask, int B, int M, int T, float* scratch, float* loss, void* stream) {
    if (!pred || !u || !mask || !scratch || !loss) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || M < 1 || T < 1) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (launch_cfm_loss(pred, u, mask, B, M, T, scratch, loss, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "cfm_loss kernel launch failed");
    return ST_OK;
}

int st_cfm_loss_backward(const float* pred, const float* u, const float* scratch, const float* grad_loss, int B, int M, int T,
                         float* grad_pred, void* stream) {
    if (!pred || !u || !scratch || !grad_loss || !grad_pred) return align_fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || M < 1 || T < 1) return align_fail(ST_ERR_INVALID, "shape out of range");
    if (launch_cfm_loss_bwd(pred, u, scratch, grad_loss, B, M, T, grad_pred, (hipStream_t)stream) != hipSuccess)
        return align_fail(ST_ERR_HIP, "cfm_loss_bwd kernel launch failed");
    return ST_OK;
}

int st_cfm_loss_scratch_floats(void) { return 2 * kCfmLossBlocks + 2; }

int st_last_solve_stats(const st_engine* e, int64_t* nfe, int64_t* steps, int64_t* rejects) {
    if (!e) return ST_ERR_INVALID;
    const DitState* dit = dit_or_null(e);      // (a handle that never solves: zeros)
    if (nfe) *nfe = dit ? dit->last_nfe : 0;
    if (steps) *steps = dit ? dit->last_steps : 0;
    if (rejects) *rejects = dit ? dit->last_rejects : 0;
    return ST_OK;
}

// Engine options by name (no reference analogue: the reference computes in fp32).
//   "attention_precision"  0 (default): q, k, v enter the attention as 16-bit operands;  1: q and k as hi + lo pairs of 16-bit operands,
//                          scores = q_hi k_hi + q_lo k_hi + q_hi k_lo (inference / solve path; for checkpoints whose softmax is an
//                          arg-max -- see st_attention_stats).  Takes effect at the next call.
//   "fused_ffn"            read-only: 0 two-kernel FFN, 1 fused direct kernel, 3 fused Winograd kernel (ST_FUSED_FFN at st_create).
int st_set_option(st_engine* e, const char* name, int value) {
    if (!e || !name) return ST_ERR_INVALID;
    const std::string n(name);
    if (n == "attention_precision") {
        if (value != 0 && value != 1) return e->fail(ST_ERR_INVALID, "attention_precision: 0 (16-bit q / k operands) or 1 (split hi + lo operands)");
        if (e->kind != KIND_DECODER) return e->fail(ST_ERR_UNSUPPORTED, "attention_precision: CFM decoder handles only");
        DitState* dit = dit_of(e);
        if (value != dit->attn_split) { dit->drop_graphs(); dit->attn_split = value; }
        return ST_OK;
    }
    if (n == "fused_ffn") return e->fail(ST_ERR_INVALID, "fused_ffn is read-only (ST_FUSED_FFN at st_create)");
    return e->fail(ST_ERR_INVALID, std::string("unknown option: ") + name);
}

int st_get_option(const st_engine* e, const char* name, int* value) {
    if (!e || !name || !value) return ST_ERR_INVALID;
    const DitState* dit = dit_or_null(e);      // (the other kinds answer with the values of a handle that st_create never configured)
    const std::string n(name);
    if (n == "attention_precision") { *value = dit ? dit->attn_split : 0; return ST_OK; }
    if (n == "fused_ffn") { *value = dit ? dit->fused_ffn : -1; return ST_OK; }
    return ST_ERR_INVALID;
}

// Largest log-sum-exp (natural-log units, of the scaled scores q.k / sqrt(d) + mask) over every valid attention row of the estimator
// evaluations completed on `stream` since the last query; -inf when there were none.  The row's score maximum lies within log(T) below
// it.  Synchronises `stream`, reads 16 words, resets the cells.
int st_attention_stats(st_engine* e, void* stream, float* max_lse) {
    if (!e || !max_lse) return ST_ERR_INVALID;
    DitState* dit = dit_or_null(e);
    if (!dit || !dit->lse_cells) return e->fail(ST_ERR_STATE, "attention statistics unavailable (allocation failed at st_create)");
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    int cells[kLseCells * 16];
    HIPCHK(e, hipMemcpy(cells, dit->lse_cells, sizeof(cells), hipMemcpyDeviceToHost));
    int best = (int)0x80000000;
    for (int c = 0; c < kLseCells; ++c) best = std::max(best, cells[c * 16]);
    HIPCHK(e, hipMemsetD32((hipDeviceptr_t)dit->lse_cells, (int)0x80000000, kLseCells * 16));
    if (best == (int)0x80000000) { *max_lse = -INFINITY; return ST_OK; }
    const int bits = best >= 0 ? best : best ^ 0x7fffffff;
    float v; memcpy(&v, &bits, 4);
    *max_lse = v * 0.6931471805599453f;      // the kernel works in log2 units (q is pre-scaled by log2 e / sqrt(d))
    return ST_OK;
}

int st_debug_capture(st_engine* e, int enable) {
    if (!e) return ST_ERR_INVALID;
    e->capture = enable != 0;
    if (!enable) {
        hipSetDevice(e->device);
        hipDeviceSynchronize();
        for (auto& kv : e->caps) if (kv.second.dev) hipFree(kv.second.dev);
        e->caps.clear();
    }
    return ST_OK;
}

int64_t st_debug_fetch(st_engine* e, const char* name, float* host_out, int64_t capacity) {
    if (!e || !name) return ST_ERR_INVALID;
    auto it = e->caps.find(name);
    if (it == e->caps.end() || !it->second.dev) { e->err = std::string("no captured tensor named ") + name; return ST_ERR_INVALID; }
    Captured& c = it->second;
    if (!host_out) return c.n;
    if (capacity < c.n) { e->err = "capacity too small"; return ST_ERR_INVALID; }
    if (hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ST_ERR_HIP;
    if (!c.is16) {
        if (hipMemcpy(host_out, c.dev, (size_t)c.n * 4, hipMemcpyDeviceToHost) != hipSuccess) return ST_ERR_HIP;
        return c.n;
    }
    float* tmp = nullptr;
    if (hipMalloc((void**)&tmp, (size_t)c.n * 4) != hipSuccess) return ST_ERR_HIP;
    hipError_t r = launch_cvt16_to_f32(e->dt, c.dev, tmp, c.n, nullptr);
    if (r == hipSuccess) r = hipMemcpy(host_out, tmp, (size_t)c.n * 4, hipMemcpyDeviceToHost);
    hipFree(tmp);
    return r == hipSuccess ? c.n : (int64_t)ST_ERR_HIP;
}

int st_profile_enable(st_engine* e, int enable) {
    if (!e) return ST_ERR_INVALID;
    hipSetDevice(e->device);
    prof_collect(e);
    e->prof = enable != 0;
    for (int i = 0; i < PC_COUNT; ++i) { e->prof_launches[i] = 0; e->prof_ms[i] = 0; e->prof_flops[i] = 0; }
    return ST_OK;
}

int st_profile_select(st_engine* e, uint64_t class_mask) {
    if (!e) return ST_ERR_INVALID;
    e->prof_mask = class_mask;
    return ST_OK;
}

int st_profile_stride(st_engine* e, int stride) {
    if (!e || stride < 1) return ST_ERR_INVALID;
    e->prof_stride = stride;
    for (int i = 0; i < PC_COUNT; ++i) e->prof_seen[i] = 0;
    return ST_OK;
}

int st_profile_num_classes(void) { return PC_COUNT; }

const char* st_profile_class_name(int cls) { return (cls >= 0 && cls < PC_COUNT) ? kProfNames[cls] : ""; }

int st_profile_read(st_engine* e, int cls, int64_t* launches, double* total_ms, double* flops_per_launch) {
    if (!e || cls < 0 || cls >= PC_COUNT) return ST_ERR_INVALID;
    hipSetDevice(e->device);
    prof_collect(e);
    if (launches) *launches = e->prof_launches[cls];
    if (total_ms) *total_ms = e->prof_ms[cls];
    if (flops_per_launch) *flops_per_launch = e->prof_flops[cls];
    e->prof_launches[cls] = 0; e->prof_ms[cls] = 0;
    return ST_OK;
}

int64_t st_device_bytes(const st_engine* e) {
    if (!e) return ST_ERR_INVALID;
    int64_t n = e->weight_bytes + (int64_t)e->ws_cap + e->state->device_bytes();
    for (auto& kv : e->params) if (kv.second.dev && !kv.second.borrowed) n += kv.second.numel() * 4;
    return n;
}

}  // extern "C"
