// MelStyleEncoder behind the C ABI (st_create_style_encoder / st_style_encoder_forward): parameter table and launch
// sequence.  Reference: models/reference_encoder.py:22-93 (eval mode), built as models/model.py:38 does.  All fp32
// (style_dp_kernels.hip); the parameters are read in place from the tensors st_load_param / st_bind_param hold.
#include "engine_internal.h"
#include "style_dp_launch.h"

#include <algorithm>
#include <string>

using namespace st;
using namespace sthost;

namespace sthost {

// Reads the loaded parameters in place: nothing to pack
struct StyleState : HeldState {
    st_style_encoder_config cfg{};
    StyleState() : HeldState("st_repack: style-encoder / duration-predictor handles read their parameters in place") {}
};

static void style_build_params(st_engine* e, const st_style_encoder_config& c) {
    const int64_t I = c.n_mel_channels, Hd = c.style_hidden, O = c.style_vector_dim, K = c.style_kernel_size;
    expect(e, "spectral.0.weight", {Hd, I}); expect(e, "spectral.0.bias", {Hd});             // reference_encoder.py:44-51
    expect(e, "spectral.3.weight", {Hd, Hd}); expect(e, "spectral.3.bias", {Hd});
    for (int i = 0; i < 2; ++i) {                                                      // :53-56, Conv1dGLU :13
        const std::string p = "temporal." + std::to_string(i) + ".conv1.";
        expect(e, p + "weight", {2 * Hd, Hd, K}); expect(e, p + "bias", {2 * Hd});
    }
    expect(e, "slf_attn.in_proj_weight", {3 * Hd, Hd}); expect(e, "slf_attn.in_proj_bias", {3 * Hd});     // :58-63
    expect(e, "slf_attn.out_proj.weight", {Hd, Hd}); expect(e, "slf_attn.out_proj.bias", {Hd});
    expect(e, "fc.weight", {O, Hd}); expect(e, "fc.bias", {O});                              // :65
}

int sd_train_grow(st_engine* e, char** buf, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return ST_OK;
    if (*buf) { HIPCHK(e, hipDeviceSynchronize()); HIPCHK(e, hipFree(*buf)); *buf = nullptr; *cap = 0; }
    HIPCHK(e, hipMalloc((void**)buf, bytes));
    *cap = bytes;
    return ST_OK;
}

HeldState::~HeldState() {
    if (held.act) hipFree(held.act);
    if (held.scr) hipFree(held.scr);
}

int HeldState::finalize(st_engine*) { held.have = false; return ST_OK; }

void sd_train_commit(SdTrain* st, int B, int T, float p_dropout, unsigned long long seed, bool masked) {
    st->serial += 1; st->have = true; st->B = B; st->T = T; st->p = p_dropout; st->seed = seed; st->masked = masked;
}

int sd_train_check(st_engine* e, const SdTrain& st, const char* entry, const char* t_name, int64_t serial, int B, int T) {
    const std::string fn(entry);
    if (!st.have) return e->fail(ST_ERR_STATE, fn + "_backward needs a preceding " + fn + "_forward");
    if ((serial >= 0 && serial != st.serial) || B != st.B || T != st.T) {
        const std::string t = std::string(", ") + t_name + "=";
        const std::string held = "B=" + std::to_string(st.B) + t + std::to_string(st.T), asked = "B=" + std::to_string(B) + t + std::to_string(T);
        if (serial < 0) return e->fail(ST_ERR_STATE, fn + "_backward: the engine holds the activations of a forward with " + held + ", not " + asked);
        return e->fail(ST_ERR_STATE, fn + "_backward: the engine holds the activations of forward #" + std::to_string(st.serial) +
                       " (" + held + "), not of #" + std::to_string(serial) + " (" + asked + ")");
    }
    return ST_OK;
}

}  // namespace sthost

extern "C" {

int st_create_style_encoder(const st_style_encoder_config* cfg, int device, st_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ST_ERR_INVALID; }
    auto bad = [&](const char* m, int code) { g_create_error = m; return code; };
    if (cfg->n_mel_channels < 1 || cfg->style_hidden < 1 || cfg->style_vector_dim < 1 || cfg->style_kernel_size < 1 || cfg->style_head < 1)
        return bad("sizes must be positive", ST_ERR_INVALID);
    if (cfg->style_hidden % cfg->style_head != 0) return bad("embed_dim must be divisible by num_heads (nn.MultiheadAttention)", ST_ERR_INVALID);
    // limits of this native build
    if (cfg->style_hidden / cfg->style_head != 64) return bad("native attention is built for head_dim == 64", ST_ERR_UNSUPPORTED);
    if (cfg->style_kernel_size != 1 && cfg->style_kernel_size != 3 && cfg->style_kernel_size != 5)
        return bad("native convolutions are built for style_kernel_size 1, 3 or 5", ST_ERR_UNSUPPORTED);
    auto state = std::make_unique<StyleState>();
    state->cfg = *cfg;
    st_engine* e = nullptr;
    if (int rc = new_handle(KIND_STYLE_ENCODER, device, std::move(state), &e)) return rc;
    style_build_params(e, *cfg);
    *out = e;
    return ST_OK;
}

int st_style_encoder_forward(st_engine* e, const float* mel, const float* mask, float* c_out, int B, int T, void* stream) {
    int rc = check_handle(e, KIND_STYLE_ENCODER); if (rc) return rc;
    if ((rc = check_finalized(e))) return rc;
    if (!mel || !c_out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if ((rc = check_sizes(e, B, T))) return rc;
    const st_style_encoder_config& c = state_of<StyleState>(e)->cfg;
    const int I = c.n_mel_channels, Hd = c.style_hidden, O = c.style_vector_dim, K = c.style_kernel_size, NH = c.style_head;
    const int64_t R = (int64_t)B * T;
    if (R * 3 * Hd >= ((int64_t)1 << 31) || R * O >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "B*T too large");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;

    // workspace: two hidden planes, the GLU / q-k-v plane, the fc output (all (B, C, T) fp32)
    FloatArena ar;
    const size_t o_h1 = ar.want((size_t)R * Hd), o_h2 = ar.want((size_t)R * Hd), o_u = ar.want((size_t)R * 3 * Hd), o_f = ar.want((size_t)R * O);
    if ((rc = ensure_ws(e, ar.off * 4))) return rc;
    float* ws = (float*)e->ws;
    float* h1 = ws + o_h1; float* h2 = ws + o_h2; float* u = ws + o_u; float* f = ws + o_f;

    auto conv = [&](const float* in, int cin, const std::string& w, const std::string& b, int cout, int taps, int epi, float* out) {
        SdConvArgs a; a.in = in; a.Cin = cin; a.w = P(e, w); a.bias = P(e, b); a.out = out; a.Cout = cout;
        a.B = B; a.T = T; a.taps = taps; a.epi = epi;
        return launch_sd_conv(a, s);
    };
    // spectral (:79-80): Linear -> Mish -> Linear -> Mish, on the channel-major mel (a Linear over channels is a k = 1 conv)
    HIPCHK(e, conv(mel, I, "spectral.0.weight", "spectral.0.bias", Hd, 1, SD_EPI_MISH, h1));
    HIPCHK(e, conv(h1, Hd, "spectral.3.weight", "spectral.3.bias", Hd, 1, SD_EPI_MISH, h2));
    // temporal (:82-83): two Conv1dGLU, padded frames unmasked as in the reference
    for (int i = 0; i < 2; ++i) {
        const std::string p = "temporal." + std::to_string(i) + ".conv1.";
        HIPCHK(e, conv(h2, Hd, p + "weight", p + "bias", 2 * Hd, K, SD_EPI_NONE, u));
        HIPCHK(e, launch_sd_glu_residual(h2, u, B, Hd, T, s));
    }
    // self-attention (:85-88): in_proj -> per-head softmax(q k^T / sqrt(64)) v with key_padding_mask -> out_proj
    HIPCHK(e, conv(h2, Hd, "slf_attn.in_proj_weight", "slf_attn.in_proj_bias", 3 * Hd, 1, SD_EPI_NONE, u));
    HIPCHK(e, launch_sd_attention(u, mask, h1, B, NH, T, s));
    HIPCHK(e, conv(h1, Hd, "slf_attn.out_proj.weight", "slf_attn.out_proj.bias", Hd, 1, SD_EPI_NONE, h2));
    // fc (:90) and the temporal average pool (:92)
    HIPCHK(e, conv(h2, Hd, "fc.weight", "fc.bias", O, 1, SD_EPI_NONE, f));
    HIPCHK(e, launch_sd_mean_pool(f, mask, c_out, B, O, T, s));
    return ST_OK;
}

}  // extern "C"

// ---- training: the forward above with its activations kept, dropout at the five sites of the reference in train
// mode, and the backward.  Salts 64 .. 68 (include/stabletts_hip.h).
namespace {

struct StyleActs {      // float offsets into SdTrain::act; R = B * T
    size_t mel, mask, pre1, h1, pre2, g0, u0, g1, u1, g2, qkv, att, stats, ao, f, end;
};

StyleActs style_acts(const st_style_encoder_config& c, int B, int T) {
    const size_t R = (size_t)B * T, Hd = c.style_hidden;
    StyleActs a{};
    FloatArena ar;
    a.mel = ar.want(R * c.n_mel_channels); a.mask = ar.want(R);
    a.pre1 = ar.want(R * Hd); a.h1 = ar.want(R * Hd); a.pre2 = ar.want(R * Hd); a.g0 = ar.want(R * Hd);
    a.u0 = ar.want(R * 2 * Hd); a.g1 = ar.want(R * Hd); a.u1 = ar.want(R * 2 * Hd); a.g2 = ar.want(R * Hd);
    a.qkv = ar.want(R * 3 * Hd); a.att = ar.want(R * Hd); a.stats = ar.want(2 * R * c.style_head); a.ao = ar.want(R * Hd);
    a.f = ar.want(R * c.style_vector_dim);
    a.end = ar.off;
    return a;
}

}  // namespace

extern "C" {

int st_style_encoder_train_forward(st_engine* e, const float* mel, const float* mask, float* c_out, int B, int T,
                                   float p_dropout, uint64_t seed, void* stream) {
    int rc = check_handle(e, KIND_STYLE_ENCODER); if (rc) return rc;
    if ((rc = check_finalized(e))) return rc;
    if (!mel || !c_out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if ((rc = check_sizes(e, B, T))) return rc;
    if ((rc = check_dropout(e, p_dropout))) return rc;
    const st_style_encoder_config& c = state_of<StyleState>(e)->cfg;
    const int I = c.n_mel_channels, Hd = c.style_hidden, O = c.style_vector_dim, K = c.style_kernel_size, NH = c.style_head;
    const int64_t R = (int64_t)B * T;
    if (R * 3 * Hd >= ((int64_t)1 << 31) || R * O >= ((int64_t)1 << 31) || R * I >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "B*T too large");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    SdTrain* st = state_of<StyleState>(e)->begin();
    const StyleActs A = style_acts(c, B, T);
    if ((rc = sd_train_grow(e, &st->act, &st->act_cap, A.end * 4))) return rc;
    float* act = (float*)st->act;
    auto at = [&](size_t o) { return act + o; };
    HIPCHK(e, hipMemcpyAsync(at(A.mel), mel, (size_t)R * I * 4, hipMemcpyDeviceToDevice, s));
    if (mask) HIPCHK(e, hipMemcpyAsync(at(A.mask), mask, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    const float* kmask = mask ? at(A.mask) : nullptr;
    SdDrop dr[5];
    for (int i = 0; i < 5; ++i) dr[i] = sd_make_drop(p_dropout, seed, 64 + i);

    auto conv = [&](const float* in, int cin, const std::string& w, const std::string& b, int cout, int taps, float* out) {
        SdConvArgs a; a.in = in; a.Cin = cin; a.w = P(e, w); a.bias = P(e, b); a.out = out; a.Cout = cout;
        a.B = B; a.T = T; a.taps = taps;
        return launch_sd_conv(a, s);
    };
    // spectral: the inference launches' fused Mish epilogue (bitwise the inference activations), the pre-activations kept
    auto conv_mish = [&](const float* in, int cin, const std::string& w, const std::string& b, float* pre, float* out) {
        SdConvArgs a; a.in = in; a.Cin = cin; a.w = P(e, w); a.bias = P(e, b); a.out = out; a.pre = pre; a.Cout = Hd;
        a.B = B; a.T = T; a.taps = 1; a.epi = SD_EPI_MISH;
        return launch_sd_conv_pre(a, s);
    };
    HIPCHK(e, conv_mish(at(A.mel), I, "spectral.0.weight", "spectral.0.bias", at(A.pre1), at(A.h1)));
    HIPCHK(e, launch_sd_drop(at(A.h1), dr[0], R * Hd, s));
    HIPCHK(e, conv_mish(at(A.h1), Hd, "spectral.3.weight", "spectral.3.bias", at(A.pre2), at(A.g0)));
    HIPCHK(e, launch_sd_drop(at(A.g0), dr[1], R * Hd, s));
    HIPCHK(e, conv(at(A.g0), Hd, "temporal.0.conv1.weight", "temporal.0.conv1.bias", 2 * Hd, K, at(A.u0)));
    HIPCHK(e, launch_sd_glu_train(at(A.g0), at(A.u0), at(A.g1), dr[2], B, Hd, T, s));
    HIPCHK(e, conv(at(A.g1), Hd, "temporal.1.conv1.weight", "temporal.1.conv1.bias", 2 * Hd, K, at(A.u1)));
    HIPCHK(e, launch_sd_glu_train(at(A.g1), at(A.u1), at(A.g2), dr[3], B, Hd, T, s));
    HIPCHK(e, conv(at(A.g2), Hd, "slf_attn.in_proj_weight", "slf_attn.in_proj_bias", 3 * Hd, 1, at(A.qkv)));
    HIPCHK(e, launch_sd_attention_train(at(A.qkv), kmask, at(A.att), at(A.stats), dr[4], B, NH, T, s));
    HIPCHK(e, conv(at(A.att), Hd, "slf_attn.out_proj.weight", "slf_attn.out_proj.bias", Hd, 1, at(A.ao)));
    HIPCHK(e, conv(at(A.ao), Hd, "fc.weight", "fc.bias", O, 1, at(A.f)));
    HIPCHK(e, launch_sd_mean_pool(at(A.f), kmask, c_out, B, O, T, s));
    sd_train_commit(st, B, T, p_dropout, seed, mask != nullptr);
    return ST_OK;
}

int st_style_encoder_train_backward(st_engine* e, int64_t serial, int B, int T, const float* grad_c, float* grad_flat, void* stream) {
    int rc = check_handle(e, KIND_STYLE_ENCODER); if (rc) return rc;
    if (!grad_c || !grad_flat) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    StyleState* sty = state_of<StyleState>(e);
    SdTrain* st = &sty->held;
    if ((rc = sd_train_check(e, *st, "st_style_encoder_train", "T", serial, B, T))) return rc;
    const st_style_encoder_config& c = sty->cfg;
    const int I = c.n_mel_channels, Hd = c.style_hidden, O = c.style_vector_dim, K = c.style_kernel_size, NH = c.style_head;
    const int64_t R = (int64_t)B * T;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const StyleActs A = style_acts(c, B, T);
    float* act = (float*)st->act;
    auto at = [&](size_t o) { return act + o; };
    const float* kmask = st->masked ? at(A.mask) : nullptr;
    SdDrop dr[5];
    for (int i = 0; i < 5; ++i) dr[i] = sd_make_drop(st->p, st->seed, 64 + i);

    // scratch: dF (O), two hidden-width planes, d att, d qkv / d u (3 Hd), the attention row sums, the split-K planes
    size_t ws = 0;
    ws = std::max(ws, sd_wgrad_scratch_floats(B, Hd, O, T, 1));
    ws = std::max(ws, sd_wgrad_scratch_floats(B, Hd, 3 * Hd, T, 1));
    ws = std::max(ws, sd_wgrad_scratch_floats(B, Hd, 2 * Hd, T, K));
    ws = std::max(ws, sd_wgrad_scratch_floats(B, Hd, Hd, T, 1));
    ws = std::max(ws, sd_wgrad_scratch_floats(B, I, Hd, T, 1));
    FloatArena ar;
    const size_t o_dF = ar.want(R * O), o_x = ar.want(R * Hd), o_y = ar.want(R * Hd), o_z = ar.want(R * Hd), o_d3 = ar.want(R * 3 * Hd),
                 o_ds = ar.want(R * NH), o_ws = ar.want(ws);
    if ((rc = sd_train_grow(e, &st->scr, &st->scr_cap, ar.off * 4))) return rc;
    float* scr = (float*)st->scr;
    float* dF = scr + o_dF; float* X = scr + o_x; float* Y = scr + o_y; float* Z = scr + o_z; float* D3 = scr + o_d3;
    float* dsum = scr + o_ds; float* wsp = scr + o_ws;

    std::map<std::string, int64_t> goff;
    train_grad_layout(e, &goff);
    auto G = [&](const std::string& n) { return grad_flat + goff.at(n); };
    // weight + bias gradient of the conv `name` (weight name + "weight" / "bias") from dY (cout) and its input x (cin)
    auto wb = [&](const std::string& w, const std::string& b, const float* dy, int cout, const float* x, int cin, int taps) {
        SdWgradArgs a; a.dy = dy; a.in = x; a.dw = G(w); a.scratch = wsp; a.B = B; a.Cin = cin; a.Cout = cout; a.T = T; a.taps = taps;
        hipError_t r = launch_sd_wgrad(a, s);
        if (r != hipSuccess) return r;
        return launch_sd_sum_frames(dy, G(b), B, cout, T, 0, s);
    };
    auto dgrad = [&](const std::string& w, const float* dy, int cout, int cin, int taps, const float* res, float* out) {
        SdConvArgs a; a.in = dy; a.Cin = cout; a.w = P(e, w); a.out = out; a.Cout = cin; a.B = B; a.T = T; a.taps = taps; a.res = res;
        return launch_sd_conv_dgrad(a, s);
    };
    HIPCHK(e, launch_sd_mean_pool_bwd(grad_c, kmask, dF, B, O, T, s));
    HIPCHK(e, wb("fc.weight", "fc.bias", dF, O, at(A.ao), Hd, 1));
    HIPCHK(e, dgrad("fc.weight", dF, O, Hd, 1, nullptr, X));                                   // d ao
    HIPCHK(e, wb("slf_attn.out_proj.weight", "slf_attn.out_proj.bias", X, Hd, at(A.att), Hd, 1));
    HIPCHK(e, dgrad("slf_attn.out_proj.weight", X, Hd, Hd, 1, nullptr, Y));                    // d att
    HIPCHK(e, launch_sd_attention_bwd(at(A.qkv), kmask, at(A.att), Y, at(A.stats), dsum, D3, dr[4], B, NH, T, s));
    HIPCHK(e, wb("slf_attn.in_proj_weight", "slf_attn.in_proj_bias", D3, 3 * Hd, at(A.g2), Hd, 1));
    HIPCHK(e, dgrad("slf_attn.in_proj_weight", D3, 3 * Hd, Hd, 1, nullptr, X));               // d g2
    HIPCHK(e, launch_sd_glu_bwd(X, at(A.u1), D3, dr[3], B, Hd, T, s));                         // d u1
    HIPCHK(e, wb("temporal.1.conv1.weight", "temporal.1.conv1.bias", D3, 2 * Hd, at(A.g1), Hd, K));
    HIPCHK(e, dgrad("temporal.1.conv1.weight", D3, 2 * Hd, Hd, K, X, Y));                      // d g1 (+ the residual)
    HIPCHK(e, launch_sd_glu_bwd(Y, at(A.u0), D3, dr[2], B, Hd, T, s));                         // d u0
    HIPCHK(e, wb("temporal.0.conv1.weight", "temporal.0.conv1.bias", D3, 2 * Hd, at(A.g0), Hd, K));
    HIPCHK(e, dgrad("temporal.0.conv1.weight", D3, 2 * Hd, Hd, K, Y, X));                      // d g0
    HIPCHK(e, launch_sd_mish_bwd(X, at(A.pre2), Z, dr[1], R * Hd, s));                         // d pre2
    HIPCHK(e, wb("spectral.3.weight", "spectral.3.bias", Z, Hd, at(A.h1), Hd, 1));
    HIPCHK(e, dgrad("spectral.3.weight", Z, Hd, Hd, 1, nullptr, Y));                           // d h1
    HIPCHK(e, launch_sd_mish_bwd(Y, at(A.pre1), Z, dr[0], R * Hd, s));                         // d pre1
    HIPCHK(e, wb("spectral.0.weight", "spectral.0.bias", Z, Hd, at(A.mel), I, 1));
    return ST_OK;
}

}  // extern "C"
