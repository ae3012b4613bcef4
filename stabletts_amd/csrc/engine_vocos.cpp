// Vocos vocoder behind the C ABI (st_create_vocoder / st_vocos_forward / st_vocos_forward_ragged): parameter table, weight
// packing and the launch sequence.  Reference: vocoders/vocos/models/model.py:11-20, backbone.py:21-56, module.py:16-46,
// head.py:17-117; config.py:4-19,46-50.  The five GEMM shapes (embed as an im2col GEMM, pwconv1 + GELU, pwconv2 +
// layer scale + residual, head) run on the implicit-GEMM kernels of the decoder over the FLATTENED rows of the batch
// (taps = 1: rows are independent); everything between them is in vocos_kernels.hip.
#include "engine_internal.h"
#include "engine_vocoder.h"
#include "vocos_launch.h"

#include <algorithm>
#include <limits>
#include <string>

using namespace st;
using namespace sthost;

namespace sthost {

struct VocosState : HeldState {      // (held: st_vocos_train_forward's activations, engine_vocos_train.cpp)
    VocosState() : HeldState("st_repack: vocoder handles re-pack through st_finalize") {}
    ~VocosState() override { slots.destroy(); }
    int finalize(st_engine* e) override;
    st_vocos_config cfg{};
    Conv embed, head;
    std::vector<Conv> pw1, pw2;
    UttSlots slots;      // ragged calls: the utterance tables (utt_slots.h)
    int grid_y = 0;      // the device's hipDeviceAttributeMaxGridDimY: the dense im2col and overlap-add kernels put the utterance on grid.y
};

static std::string vblk(int i) { return "backbone.convnext." + std::to_string(i) + "."; }

void vocos_build_params(st_engine* e, const st_vocos_config& c) {
    const int64_t C = c.dim, F = c.intermediate_dim, M = c.input_channels;
    expect(e, "backbone.embed.weight", {C, M, 7}); expect(e, "backbone.embed.bias", {C});                 // backbone.py:28
    expect(e, "backbone.norm.weight", {C}); expect(e, "backbone.norm.bias", {C});                        // :29
    for (int i = 0; i < c.num_layers; ++i) {                                                       // module.py:22-31
        const std::string p = vblk(i);
        expect(e, p + "dwconv.weight", {C, 1, 7}); expect(e, p + "dwconv.bias", {C});
        expect(e, p + "norm.weight", {C}); expect(e, p + "norm.bias", {C});
        expect(e, p + "pwconv1.weight", {F, C}); expect(e, p + "pwconv1.bias", {F});
        expect(e, p + "pwconv2.weight", {C, F}); expect(e, p + "pwconv2.bias", {C});
        expect(e, p + "gamma", {C});
    }
    expect(e, "backbone.final_layer_norm.weight", {C}); expect(e, "backbone.final_layer_norm.bias", {C});   // backbone.py:41
    expect(e, "head.out.weight", {c.n_fft + 2, C}); expect(e, "head.out.bias", {c.n_fft + 2});            // head.py:88-89
    expect(e, "head.istft.window", {c.n_fft});                                                         // head.py:27-28
}

// st_finalize of a vocoder handle: 16-bit GEMM weights.  Linear weights (out, in) are k = 1 convolutions; the k = 7
// embed convolution packs as [cout][tap][cin] = the K order of launch_voc_im2col7's rows, each row padded with zeros to
// voc_im2col_pitch(M).  The head's n_fft + 2 output rows are laid out as two planes of voc_head_plane(n_fft) rows
// (log-magnitude 0..n_fft/2, phase 0..n_fft/2, zero rows between): 1152 at n_fft 2048, 640 / 384 / 256 at 1024 / 512 / 256.
int VocosState::finalize(st_engine* e) {
    HeldState::finalize(e);
    free_owned(e);
    VocosState* v = this;
    const st_vocos_config& c = v->cfg;
    const int C = c.dim, F = c.intermediate_dim, M = c.input_channels, L = c.num_layers;
    hipStream_t s = nullptr;
    auto pack = [&](Conv& cv, const std::string& wname, const std::string& bname, int cout, int cin, int taps) -> int {
        cv.cout = cout; cv.cin = cin; cv.taps = taps; cv.split = false;
        int rc = dev_alloc(e, &cv.w, (size_t)cout * taps * cin * 2); if (rc) return rc;
        HIPCHK(e, launch_pack_weight(e->dt, P(e, wname), cout, cin, taps, 0, cin, cv.w, 0, cin, 0, cin, 0, s));
        rc = dev_alloc(e, (void**)&cv.bias, (size_t)cout * 4); if (rc) return rc;
        HIPCHK(e, hipMemcpyAsync(cv.bias, P(e, bname), (size_t)cout * 4, hipMemcpyDeviceToDevice, s));
        return ST_OK;
    };
    // the pointwise convs of the ConvNeXt blocks with SPLIT WEIGHTS (round 6): K = [x | x] against [W_hi | W_lo] -- the activation operand is read
    // twice, no producer changes; twice the MFMA work of the backbone's GEMMs.  Takes the weights' share out of the waveform's 16-bit error
    // (it sat 3 % under its 1e-3 gate).
    auto pack_wsplit = [&](Conv& cv, const std::string& wname, const std::string& bname, int cout, int cin) -> int {
        cv.cout = cout; cv.cin = 2 * cin; cv.taps = 1; cv.split = false;
        int rc = dev_alloc(e, &cv.w, (size_t)cout * 2 * cin * 2); if (rc) return rc;
        for (int k2 = 0; k2 < 2; ++k2)
            HIPCHK(e, launch_pack_weight(e->dt, P(e, wname), cout, cin, 1, 0, cin, cv.w, 0, 2 * cin, k2 * cin, cin, k2 == 1, s));
        rc = dev_alloc(e, (void**)&cv.bias, (size_t)cout * 4); if (rc) return rc;
        HIPCHK(e, hipMemcpyAsync(cv.bias, P(e, bname), (size_t)cout * 4, hipMemcpyDeviceToDevice, s));
        return ST_OK;
    };
    int rc;
    const int Kp = voc_im2col_pitch(M);
    if (Kp == 7 * M) {
        if ((rc = pack(v->embed, "backbone.embed.weight", "backbone.embed.bias", C, M, 7))) return rc;
    } else {        // M % 64 != 0: [cout][7 M] packed into a staging buffer, then copied into rows of pitch Kp whose tail stays zero
        Conv& cv = v->embed;
        cv.cout = C; cv.split = false;
        if ((rc = dev_alloc(e, &cv.w, (size_t)C * Kp * 2))) return rc;
        if ((rc = dev_alloc(e, (void**)&cv.bias, (size_t)C * 4))) return rc;
        void* stage = nullptr;
        HIPCHK(e, hipMalloc(&stage, (size_t)C * 7 * M * 2));
        hipError_t he = launch_pack_weight(e->dt, P(e, "backbone.embed.weight"), C, M, 7, 0, M, stage, 0, M, 0, M, 0, s);
        if (he == hipSuccess) he = hipMemsetAsync(cv.w, 0, (size_t)C * Kp * 2, s);
        if (he == hipSuccess) he = hipMemcpy2DAsync(cv.w, (size_t)Kp * 2, stage, (size_t)7 * M * 2, (size_t)7 * M * 2, C, hipMemcpyDeviceToDevice, s);
        if (he == hipSuccess) he = hipStreamSynchronize(s);
        hipFree(stage);
        HIPCHK(e, he);
        HIPCHK(e, hipMemcpyAsync(cv.bias, P(e, "backbone.embed.bias"), (size_t)C * 4, hipMemcpyDeviceToDevice, s));
    }
    v->embed.cin = Kp; v->embed.taps = 1;        // consumed as a k = 1 GEMM over the im2col rows
    v->pw1.assign(L, Conv()); v->pw2.assign(L, Conv());
    for (int i = 0; i < L; ++i) {
        if ((rc = pack_wsplit(v->pw1[i], vblk(i) + "pwconv1.weight", vblk(i) + "pwconv1.bias", F, C))) return rc;
        if ((rc = pack_wsplit(v->pw2[i], vblk(i) + "pwconv2.weight", vblk(i) + "pwconv2.bias", C, F))) return rc;
    }
    {
        Conv& h = v->head;
        const int bins = c.n_fft / 2 + 1, plane = voc_head_plane(c.n_fft), planes = 2 * plane;
        // split-precision operands (round 5), as for the decoder's in_proj / final_proj: the head's output x feeds exp(x) -- an absolute
        // error of x is a RELATIVE error of the magnitude -- so the 16-bit rounding of its operands reached the waveform un-attenuated
        // (f16: hidden 4.8e-4 -> audio 1.1e-3).  K = [h_hi | h_lo | h_hi] against [W_hi | W_hi | W_lo]: 3x the MFMA work of one small GEMM.
        h.cout = planes; h.cin = 3 * C; h.taps = 1; h.split = true;
        if ((rc = dev_alloc(e, &h.w, (size_t)planes * 3 * C * 2))) return rc;
        if ((rc = dev_alloc(e, (void**)&h.bias, (size_t)planes * 4))) return rc;
        HIPCHK(e, hipMemsetAsync(h.w, 0, (size_t)planes * 3 * C * 2, s));
        HIPCHK(e, hipMemsetAsync(h.bias, 0, (size_t)planes * 4, s));
        const float* W = P(e, "head.out.weight"); const float* Bv = P(e, "head.out.bias");
        for (int part = 0; part < 2; ++part) {       // head.py:104: mag, p = x.chunk(2, dim=1)
            for (int k3 = 0; k3 < 3; ++k3)
                HIPCHK(e, launch_pack_weight(e->dt, W + (size_t)part * bins * C, bins, C, 1, 0, C, h.w, part * plane, 3 * C, k3 * C, C, k3 == 2, s));
            HIPCHK(e, hipMemcpyAsync(h.bias + part * plane, Bv + (size_t)part * bins, (size_t)bins * 4, hipMemcpyDeviceToDevice, s));
        }
    }
    HIPCHK(e, hipDeviceSynchronize());
    return ST_OK;
}

const st_vocos_config& vocos_config_of(const st_engine* e) { return state_of<VocosState>(e)->cfg; }

}  // namespace sthost

extern "C" {

int st_create_vocoder(const st_vocos_config* cfg, int device, st_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ST_ERR_INVALID; }
    auto bad = [&](const char* m, int code) { g_create_error = m; return code; };
    if (cfg->num_layers < 1 || cfg->num_layers > 32) return bad("num_layers must be in [1, 32]", ST_ERR_INVALID);
    if (cfg->input_channels < 1 || cfg->dim < 1 || cfg->intermediate_dim < 1) return bad("channel counts must be positive", ST_ERR_INVALID);
    if (cfg->operand_dtype != ST_OPERAND_BF16 && cfg->operand_dtype != ST_OPERAND_F16) return bad("operand_dtype", ST_ERR_INVALID);
    // limits of this native build
    if (!voc_dim_supported(cfg->dim)) return bad("native vocoder kernels are built for dim == 512, 768 or 1024", ST_ERR_UNSUPPORTED);
    if (!voc_nfft_supported(cfg->n_fft) || cfg->hop_length != cfg->n_fft / 4)
        return bad("native ISTFT is built for n_fft == 256, 512, 1024 or 2048 with hop_length == n_fft / 4", ST_ERR_UNSUPPORTED);
    if (cfg->input_channels % 16 != 0 || cfg->input_channels > 192) return bad("input_channels must be a multiple of 16 up to 192", ST_ERR_UNSUPPORTED);
    if (cfg->intermediate_dim % 256 != 0) return bad("intermediate_dim must be a multiple of 256", ST_ERR_UNSUPPORTED);
    auto state = std::make_unique<VocosState>();
    state->cfg = *cfg;
    st_engine* e = nullptr;
    if (int rc = new_handle(KIND_VOCODER, device, std::move(state), &e)) return rc;
    e->dt = cfg->operand_dtype == ST_OPERAND_BF16 ? DT_BF16 : DT_F16;
    e->tile.splitk_target = 0;      // no split-K convs: the vocoder's GEMMs run over the flattened rows of the whole batch
    vocos_build_params(e, *cfg);
    if (hipMalloc(&e->zeros, 256) != hipSuccess || hipMemset(e->zeros, 0, 256) != hipSuccess) {
        delete e;
        return bad("hipMalloc failed", ST_ERR_HIP);
    }
    if (hipDeviceGetAttribute(&state_of<VocosState>(e)->grid_y, hipDeviceAttributeMaxGridDimY, e->device) != hipSuccess) {
        delete e;
        return bad("hipDeviceGetAttribute failed", ST_ERR_HIP);
    }
    *out = e;
    return ST_OK;
}

// One chunk of whole utterances: every GEMM runs over its R flattened rows, R = B * T, or the packed rows of a ragged chunk
// (rg: mel and audio stay padded to T; only the im2col, the depthwise conv and the overlap-add know utterances and take the
// ragged launcher).  The K loop of the conv GEMM forms an activation row's byte offset as a 32-bit value (t * cin * 2,
// conv_gemm2_impl.h), so the callers size chunks to keep R * max(voc_im2col_pitch(M), C, F) * 2 below 2^31.
static int vocos_forward_chunk(st_engine* e, const float* mel, float* audio, int B, int T, const RaggedChunk* rg, hipStream_t s) {
    VocosState* v = state_of<VocosState>(e);
    const st_vocos_config& c = v->cfg;
    const int C = c.dim, F = c.intermediate_dim, M = c.input_channels, L = c.num_layers;
    const int Kp = voc_im2col_pitch(M), plane = voc_head_plane(c.n_fft);
    const int64_t R = rg ? rg->rows : (int64_t)B * T;

    // workspace: im2col rows, fp32 residual stream, 16-bit operands, head output, windowed frames
    size_t off = 0;
    auto want = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_a16 = want((size_t)R * Kp * 2), o_x = want((size_t)R * C * 4), o_h16 = want((size_t)R * C * 2), o_h16lo = want((size_t)R * C * 2);
    const size_t o_u16 = want((size_t)R * F * 2), o_head = want((size_t)R * 2 * plane * 4), o_fr = want((size_t)R * c.n_fft * 4);
    const size_t o_tiles = rg ? want((size_t)rg->n_tiles * sizeof(VocSeg)) : 0, o_groups = rg ? want((size_t)rg->n_groups * sizeof(VocSeg)) : 0;
    int rc = ensure_ws(e, off); if (rc) return rc;
    VocSeg* tiles = (VocSeg*)(e->ws + o_tiles); VocSeg* groups = (VocSeg*)(e->ws + o_groups);
    void* a16 = e->ws + o_a16; float* x = (float*)(e->ws + o_x); void* h16 = e->ws + o_h16; void* h16lo = e->ws + o_h16lo; void* u16 = e->ws + o_u16;
    float* head = (float*)(e->ws + o_head); float* frames = (float*)(e->ws + o_fr);

    auto args = [&](const Conv& cv) { return flat_gemm_args(e, cv, R); };
    const bool cap = e->capture;
    {   // embed (backbone.py:51) + LayerNorm (:52)
        ProfScope ps(e, s, PC_PRENET, 2.0 * R * C * 7.0 * M);
        if (rg) {
            HIPCHK(e, launch_voc_segments(rg->utt, B, rg->dw_frames, tiles, groups, s));
            HIPCHK(e, launch_voc_im2col7_ragged(e->dt, mel, tiles, rg->n_tiles, M, T, a16, s));
        } else {
            HIPCHK(e, launch_voc_im2col7(e->dt, mel, B, M, T, a16, s));
        }
        ConvGemmArgs a = args(v->embed); a.a0 = a16; a.c0 = Kp; a.out32 = x;
        HIPCHK(e, gemm(e, 1, EPI_F32, a, s));
        HIPCHK(e, launch_voc_ln(e->dt, x, P(e, "backbone.norm.weight"), P(e, "backbone.norm.bias"), R, C, x, nullptr, nullptr, s));
    }
    if (cap) capture(e, "voc.embed", x, R * C, false, s);
    for (int i = 0; i < L; ++i) {       // ConvNeXtBlock.forward (module.py:33-46)
        const std::string p = vblk(i);
        {
            ProfScope ps(e, s, PC_FILM_LN1, 0);
            const float *dw = P(e, p + "dwconv.weight"), *db = P(e, p + "dwconv.bias"), *nw = P(e, p + "norm.weight"), *nb = P(e, p + "norm.bias");
            if (rg) HIPCHK(e, launch_voc_dwconv_ln_ragged(e->dt, x, dw, db, nw, nb, groups, rg->n_groups, rg->dw_frames, C, h16, s));
            else    HIPCHK(e, launch_voc_dwconv_ln(e->dt, x, dw, db, nw, nb, B, T, C, h16, s));
        }
        {
            ProfScope ps(e, s, PC_FFN1, 2.0 * R * C * (double)F);
            ConvGemmArgs a = args(v->pw1[i]); a.a0 = h16; a.c0 = C; a.a1 = h16; a.c1 = C; a.out16 = u16;      // [x | x] . [W_hi | W_lo]
            HIPCHK(e, gemm(e, 1, EPI_GELU16, a, s));
        }
        {   // pwconv2, layer scale, residual (:40-45): x += gamma * (W u + b)
            ProfScope ps(e, s, PC_FFN2, 2.0 * R * C * (double)F);
            ConvGemmArgs a = args(v->pw2[i]); a.a0 = u16; a.c0 = F; a.a1 = u16; a.c1 = F; a.out32 = x; a.gate = P(e, p + "gamma"); a.gate_stride = 0;
            HIPCHK(e, gemm(e, 1, EPI_RESGATE, a, s));
        }
        if (cap) capture(e, "voc.block" + std::to_string(i), x, R * C, false, s);
    }
    {   // final LayerNorm (backbone.py:55) + head projection (head.py:103)
        ProfScope ps(e, s, PC_FINAL, 2.0 * R * C * (double)(c.n_fft + 2));
        HIPCHK(e, launch_voc_ln(e->dt, x, P(e, "backbone.final_layer_norm.weight"), P(e, "backbone.final_layer_norm.bias"), R, C,
                                cap ? x : nullptr, h16, h16lo, s));
        ConvGemmArgs a = args(v->head); a.a0 = h16; a.c0 = C; a.a1 = h16lo; a.c1 = C; a.c2 = C; a.out32 = head;
        HIPCHK(e, gemm(e, 1, EPI_F32, a, s));
    }
    if (cap) { capture(e, "voc.hidden", x, R * C, false, s); capture(e, "voc.head_out", head, R * 2 * plane, false, s); }
    {   // ISTFT (head.py:104-116)
        ProfScope ps(e, s, PC_ODE, 0);
        HIPCHK(e, launch_voc_spec_ifft(head, P(e, "head.istft.window"), R, c.n_fft, frames, s));
        if (rg) HIPCHK(e, launch_voc_overlap_add_ragged(frames, P(e, "head.istft.window"), rg->utt, B, T, c.n_fft, audio, s));
        else    HIPCHK(e, launch_voc_overlap_add(frames, P(e, "head.istft.window"), B, T, c.n_fft, audio, s));
    }
    return ST_OK;
}

// rows per chunk: 32-bit GEMM operand offsets (widest operand row: the im2col rows, C or F) and head output indices
static int64_t vocos_max_rows(const st_vocos_config& c) {
    const int64_t widest = std::max({(int64_t)voc_im2col_pitch(c.input_channels), (int64_t)c.dim, (int64_t)c.intermediate_dim, (int64_t)voc_head_plane(c.n_fft)});
    return (((int64_t)1 << 31) - 1) / (widest * 2);
}

// dense: the utterance on grid.y; ragged: the padded frames of one overlap-add launch
static VocoderGeom vocos_geom(st_engine* e) {
    VocosState* v = state_of<VocosState>(e);
    const int64_t max_rows = vocos_max_rows(v->cfg), no_cap = std::numeric_limits<int64_t>::max();
    return {{max_rows, v->grid_y, 0, 0}, {max_rows, no_cap, kVocMaxPaddedFrames, 0}, v->cfg.input_channels, v->cfg.hop_length, &v->slots};
}
static const VocoderKind kVocosKind = {KIND_VOCODER, "the vocoder's 32-bit row indexing", 0, vocos_geom, voc_dw_frames, vocos_forward_chunk};

int st_vocos_forward(st_engine* e, const float* mel, float* audio, int B, int T, void* stream) {
    return vocoder_forward(kVocosKind, e, mel, audio, B, T, stream);
}

int st_vocos_forward_ragged(st_engine* e, const float* mel, const int64_t* lengths, float* audio, int B, int T, void* stream) {
    return vocoder_forward_ragged(kVocosKind, e, mel, lengths, audio, B, T, stream);
}

}  // extern "C"
