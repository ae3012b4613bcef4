// Vocos generator training behind the C ABI (st_vocos_train_forward / st_vocos_train_backward) on a vocoder handle:
// the fp32 forward of Vocos.forward (vocoders/vocos/models/model.py:17-20; backbone.py:50-56, module.py:33-46,
// head.py:39-72,93-117) that keeps its activations, and the backward from d audio to every parameter and the mel.
// The inference path (engine_vocos.cpp, 16-bit operands) is not involved: the parameters are read in place as fp32 from the
// tensors st_bind_param / st_load_param hold, the GEMMs are the fp32 MFMA tile kernels of style_dp_launch.h called on the
// channel-major (C, B * T) tensors as B = 1, T = B * T, and the row work is vocos_train_kernels.hip.  The k = 7 embed conv is
// the im2col form: cols (7 M, R) against backbone.embed.weight read as (C, 7 M).
// Kept per forward: the im2col of the mel, the embed conv output and its LayerNorm statistics, per block its input, the
// dwconv-LayerNorm statistics, the normalised h, the pre-GELU u and the pwconv2 output (d gamma needs it), the last block's
// output with the final LayerNorm statistics and output, and the head output rows.
#include "engine_internal.h"
#include "style_dp_launch.h"
#include "vocos_train_launch.h"

#include <algorithm>
#include <string>

using namespace st;
using namespace sthost;

namespace {

struct VtCfg {
    int C, F, M, L, NB;       // NB = n_fft + 2 head rows
    // accumulation chains of the GEMMs (SdConvArgs::chains).  dim 512 keeps the arithmetic it was released with; the wider generators
    // (the trainer's 768 / 2048 / 12) contract over up to 2048 terms through more blocks, and four chains hold their gradients
    // within the bar of the 512 preset against the reference module (tests/test_gpu_vocos_dims_training.py)
    int chains() const { return C > 512 ? 4 : 1; }
};

// the handle's configuration from its parameter table (st_create_vocoder built it from the st_vocos_config)
VtCfg vt_cfg(const st_engine* e) {
    VtCfg c{};
    const auto& ew = e->params.at("backbone.embed.weight").shape;
    c.C = (int)ew[0]; c.M = (int)ew[1];
    c.F = (int)e->params.at("backbone.convnext.0.pwconv1.weight").shape[0];
    c.NB = (int)e->params.at("head.out.weight").shape[0];
    while (e->params.count("backbone.convnext." + std::to_string(c.L) + ".gamma")) c.L += 1;
    return c;
}

std::string vblk(int i) { return "backbone.convnext." + std::to_string(i) + "."; }

struct VtActs {         // float offsets into SdTrain::act
    size_t cols, e0, st0, x, blk, blk_stride, b_st, b_h, b_u, b_y2, stf, hf, hrows, end;
};

VtActs vt_acts(const VtCfg& c, int64_t R) {
    VtActs a{};
    FloatArena ar;
    a.cols = ar.want((size_t)7 * c.M * R); a.e0 = ar.want((size_t)c.C * R); a.st0 = ar.want(2 * R);
    a.x = ar.want((size_t)(c.L + 1) * c.C * R);          // x_0 .. x_L, C * R apart
    a.blk = ar.off;
    a.b_st = ar.want(2 * R) - a.blk; a.b_h = ar.want((size_t)c.C * R) - a.blk; a.b_u = ar.want((size_t)c.F * R) - a.blk; a.b_y2 = ar.want((size_t)c.C * R) - a.blk;
    a.blk_stride = ar.off - a.blk;
    ar.off = a.blk + a.blk_stride * c.L;
    a.stf = ar.want(2 * R); a.hf = ar.want((size_t)c.C * R); a.hrows = ar.want((size_t)R * 2 * kVocHeadPlane);
    a.end = ar.off;
    return a;
}

int vt_check_shape(st_engine* e, const VtCfg& c, int B, int T) {
    const int64_t R = (int64_t)B * T;
    const int64_t widest = std::max({(int64_t)7 * c.M, (int64_t)c.C, (int64_t)c.F, (int64_t)2 * kVocHeadPlane, (int64_t)kVocNfft});
    if (R * widest >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "B*T too large for the vocoder's training path (32-bit tile indexing)");
    if (B > 65535) return e->fail(ST_ERR_INVALID, "B too large for the vocoder's training path (at most 65535 items)");
    return ST_OK;
}

// The training path keeps the preset's ISTFT (kVocNfft / kVocHop, kVocHeadPlane) and im2col rows of exactly 7 M columns, so it
// serves the handles st_create_vocoder admitted before the inference path took other n_fft and mel widths, and refuses the rest
// before any allocation or launch.
int vt_check_config(st_engine* e) {
    const st_vocos_config& c = vocos_config_of(e);
    if (c.n_fft != kVocNfft || c.hop_length != kVocHop || c.input_channels % 64 != 0)
        return e->fail(ST_ERR_UNSUPPORTED, "native Vocos training is built for n_fft == 2048, hop_length == 512 and input_channels 64, 128 or 192 "
                                           "(inference alone takes the other n_fft and mel widths)");
    return ST_OK;
}

}  // namespace

extern "C" {

int st_vocos_train_forward(st_engine* e, const float* mel, float* audio, int B, int T, void* stream) {
    int rc = check_handle(e, KIND_VOCODER); if (rc) return rc;
    if ((rc = vt_check_config(e))) return rc;
    if ((rc = check_finalized(e))) return rc;
    if (!mel || !audio) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if ((rc = check_sizes(e, B, T))) return rc;
    const VtCfg c = vt_cfg(e);
    if ((rc = vt_check_shape(e, c, B, T))) return rc;
    const int C = c.C, F = c.F, M = c.M, L = c.L;
    const int64_t R = (int64_t)B * T;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    SdTrain* st = state_of<HeldState>(e)->begin();
    const VtActs A = vt_acts(c, R);
    if ((rc = sd_train_grow(e, &st->act, &st->act_cap, A.end * 4))) return rc;
    float* act = (float*)st->act;
    auto at = [&](size_t o) { return act + o; };
    // transients: the dwconv output, the GELU output, the channel-major head output, the windowed frames
    FloatArena ar;
    const size_t o_z = ar.want((size_t)C * R), o_g = ar.want((size_t)F * R), o_o = ar.want((size_t)c.NB * R), o_fr = ar.want((size_t)R * kVocNfft);
    if ((rc = sd_train_grow(e, &st->scr, &st->scr_cap, ar.off * 4))) return rc;
    float* scr = (float*)st->scr;
    float* z = scr + o_z; float* g = scr + o_g; float* o = scr + o_o; float* frames = scr + o_fr;

    auto conv = [&](const float* in, int cin, const std::string& w, const std::string& b, int cout, float* out) {
        SdConvArgs a; a.in = in; a.Cin = cin; a.w = P(e, w); a.bias = P(e, b); a.out = out; a.Cout = cout;
        a.B = 1; a.T = (int)R; a.taps = 1; a.chains = c.chains();
        return launch_sd_conv(a, s);
    };
    auto ln = [&](const float* x, const std::string& p, float* stats, float* y) {
        return launch_sd_layernorm_train(x, y, stats, stats + R, P(e, p + "weight"), P(e, p + "bias"), 1e-6f, SdDrop{}, 1, C, (int)R, s);
    };
    // embed (backbone.py:51) + LayerNorm (:52)
    HIPCHK(e, launch_vt_im2col7(mel, at(A.cols), B, M, T, s));
    HIPCHK(e, conv(at(A.cols), 7 * M, "backbone.embed.weight", "backbone.embed.bias", C, at(A.e0)));
    HIPCHK(e, ln(at(A.e0), "backbone.norm.", at(A.st0), at(A.x)));
    for (int i = 0; i < L; ++i) {       // ConvNeXtBlock.forward (module.py:33-46)
        const std::string p = vblk(i);
        float* xi = at(A.x) + (size_t)i * C * R;
        float* bk = at(A.blk + A.blk_stride * i);
        HIPCHK(e, launch_vt_dwconv7(xi, P(e, p + "dwconv.weight"), P(e, p + "dwconv.bias"), z, C, B, T, s));
        HIPCHK(e, ln(z, p + "norm.", bk + A.b_st, bk + A.b_h));
        HIPCHK(e, conv(bk + A.b_h, C, p + "pwconv1.weight", p + "pwconv1.bias", F, bk + A.b_u));
        HIPCHK(e, launch_vt_gelu(bk + A.b_u, g, (int64_t)F * R, s));
        HIPCHK(e, conv(g, F, p + "pwconv2.weight", p + "pwconv2.bias", C, bk + A.b_y2));
        HIPCHK(e, launch_vt_scale_residual(xi, bk + A.b_y2, P(e, p + "gamma"), xi + (size_t)C * R, C, R, s));
    }
    // final LayerNorm (backbone.py:55), head projection (head.py:103), ISTFT (:104-116: the inference kernels, fp32 already)
    HIPCHK(e, ln(at(A.x) + (size_t)L * C * R, "backbone.final_layer_norm.", at(A.stf), at(A.hf)));
    HIPCHK(e, conv(at(A.hf), C, "head.out.weight", "head.out.bias", c.NB, o));
    const int bins = c.NB / 2;
    HIPCHK(e, launch_vt_transpose(o, bins, (int)R, R, at(A.hrows), 2 * kVocHeadPlane, s));
    HIPCHK(e, launch_vt_transpose(o + (size_t)bins * R, bins, (int)R, R, at(A.hrows) + kVocHeadPlane, 2 * kVocHeadPlane, s));
    HIPCHK(e, launch_voc_spec_ifft(at(A.hrows), P(e, "head.istft.window"), R, kVocNfft, frames, s));
    HIPCHK(e, launch_voc_overlap_add(frames, P(e, "head.istft.window"), B, T, kVocNfft, audio, s));
    sd_train_commit(st, B, T, 0.0f, 0, false);
    return ST_OK;
}

int st_vocos_train_backward(st_engine* e, const float* d_audio, float* d_mel, float* grad_flat, int B, int T, void* stream) {
    int rc = check_handle(e, KIND_VOCODER); if (rc) return rc;
    if ((rc = vt_check_config(e))) return rc;
    if (!d_audio || !grad_flat) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if ((rc = check_sizes(e, B, T))) return rc;
    SdTrain* st = &state_of<HeldState>(e)->held;
    if ((rc = sd_train_check(e, *st, "st_vocos_train", "T", -1, B, T))) return rc;
    const VtCfg c = vt_cfg(e);
    const int C = c.C, F = c.F, M = c.M, L = c.L, NB = c.NB;
    const int64_t R = (int64_t)B * T;
    const int Ri = (int)R;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const VtActs A = vt_acts(c, R);
    float* act = (float*)st->act;
    auto at = [&](size_t o) { return act + o; };

    size_t ws = 0;
    ws = std::max(ws, sd_wgrad_scratch_floats(1, C, NB, Ri, 1));
    ws = std::max(ws, sd_wgrad_scratch_floats(1, F, C, Ri, 1));
    ws = std::max(ws, sd_wgrad_scratch_floats(1, C, F, Ri, 1));
    ws = std::max(ws, sd_wgrad_scratch_floats(1, 7 * M, C, Ri, 1));
    FloatArena ar;
    // d head rows and (later) d cols share one region; d head output channel-major; GELU output; d u, which later takes the C-wide
    // d z as well (so max(F, C) rows: intermediate_dim may be below dim); three C-wide planes; the split-K planes
    const size_t big = std::max((size_t)R * 2 * kVocHeadPlane, d_mel ? (size_t)7 * M * R : 0);
    const size_t o_dh = ar.want(big), o_do = ar.want((size_t)NB * R), o_g = ar.want((size_t)F * R), o_du = ar.want((size_t)std::max(F, C) * R),
                 o_x = ar.want((size_t)C * R), o_y = ar.want((size_t)C * R), o_z = ar.want((size_t)C * R), o_ws = ar.want(ws);
    if ((rc = sd_train_grow(e, &st->scr, &st->scr_cap, ar.off * 4))) return rc;
    float* scr = (float*)st->scr;
    float* dH = scr + o_dh; float* dO = scr + o_do; float* g = scr + o_g; float* dU = scr + o_du;
    float* X = scr + o_x; float* Y = scr + o_y; float* Z = scr + o_z; float* wsp = scr + o_ws;

    std::map<std::string, int64_t> goff;
    train_grad_layout(e, &goff);
    auto G = [&](const std::string& n) { return grad_flat + goff.at(n); };
    auto wb = [&](const std::string& p, const float* dy, int cout, const float* x, int cin) {
        SdWgradArgs a; a.dy = dy; a.in = x; a.dw = G(p + "weight"); a.scratch = wsp; a.B = 1; a.Cin = cin; a.Cout = cout; a.T = Ri; a.taps = 1;
        hipError_t r = launch_sd_wgrad(a, s);
        if (r != hipSuccess) return r;
        return launch_sd_sum_frames(dy, G(p + "bias"), 1, cout, Ri, 0, s);
    };
    auto dgrad = [&](const std::string& w, const float* dy, int cout, int cin, float* out) {
        SdConvArgs a; a.in = dy; a.Cin = cout; a.w = P(e, w); a.out = out; a.Cout = cin; a.B = 1; a.T = Ri; a.taps = 1; a.chains = c.chains();
        return launch_sd_conv_dgrad(a, s);
    };
    auto ln_bwd = [&](const float* dy, const float* x, const float* stats, const std::string& p, float* dx) {
        return launch_sd_layernorm_bwd(dy, x, stats, stats + R, P(e, p + "weight"), dx, G(p + "weight"), G(p + "bias"), SdDrop{}, 0, 1, C, Ri, s);
    };
    // ISTFT head backward -> d head output (channel-major), head linear, final LayerNorm
    const int bins = NB / 2;
    HIPCHK(e, launch_vt_istft_bwd(d_audio, P(e, "head.istft.window"), at(A.hrows), dH, B, T, s));
    HIPCHK(e, launch_vt_transpose(dH, R, bins, 2 * kVocHeadPlane, dO, R, s));
    HIPCHK(e, launch_vt_transpose(dH + kVocHeadPlane, R, bins, 2 * kVocHeadPlane, dO + (size_t)bins * R, R, s));
    HIPCHK(e, wb("head.out.", dO, NB, at(A.hf), C));
    HIPCHK(e, dgrad("head.out.weight", dO, NB, C, Y));                                              // d hf
    HIPCHK(e, ln_bwd(Y, at(A.x) + (size_t)L * C * R, at(A.stf), "backbone.final_layer_norm.", X));      // X = d x_L
    for (int i = L - 1; i >= 0; --i) {
        const std::string p = vblk(i);
        const float* xi = at(A.x) + (size_t)i * C * R;
        const float* bk = at(A.blk + A.blk_stride * i);
        HIPCHK(e, launch_vt_scale_bwd(X, bk + A.b_y2, P(e, p + "gamma"), Y, G(p + "gamma"), C, R, s));      // Y = d y2
        HIPCHK(e, launch_vt_gelu(bk + A.b_u, g, (int64_t)F * R, s));
        HIPCHK(e, wb(p + "pwconv2.", Y, C, g, F));
        HIPCHK(e, dgrad(p + "pwconv2.weight", Y, C, F, dU));                                        // d g
        HIPCHK(e, launch_vt_gelu_bwd(dU, bk + A.b_u, dU, (int64_t)F * R, s));                       // d u
        HIPCHK(e, wb(p + "pwconv1.", dU, F, bk + A.b_h, C));
        HIPCHK(e, dgrad(p + "pwconv1.weight", dU, F, C, Y));                                        // d h
        HIPCHK(e, launch_vt_dwconv7(xi, P(e, p + "dwconv.weight"), P(e, p + "dwconv.bias"), Z, C, B, T, s));    // the LayerNorm's input again
        HIPCHK(e, ln_bwd(Y, Z, bk + A.b_st, p + "norm.", dU));                                      // d z (in d u's plane, free by now)
        HIPCHK(e, launch_vt_dwconv7_bwd(dU, xi, P(e, p + "dwconv.weight"), X, Z, G(p + "dwconv.weight"), G(p + "dwconv.bias"), C, B, T, s));
        std::swap(X, Z);                                                                            // X = d x_i
    }
    HIPCHK(e, ln_bwd(X, at(A.e0), at(A.st0), "backbone.norm.", Y));                                  // d e0
    HIPCHK(e, wb("backbone.embed.", Y, C, at(A.cols), 7 * M));
    if (d_mel) {
        HIPCHK(e, dgrad("backbone.embed.weight", Y, C, 7 * M, dH));                                 // d cols
        HIPCHK(e, launch_vt_col2im7(dH, d_mel, B, M, T, s));
    }
    return ST_OK;
}

}  // extern "C"
