// DiscriminatorR behind the C ABI (st_create_resolution_discriminator / st_resolution_disc_*): parameter table, the weight norm,
// and the launch sequences of the forward and the backward.  Reference: vocoders/vocos/models/discriminator.py:112-171, one handle
// per window length.  All fp32 (resolution_disc_kernels.hip); the parameters -- the weight norm's g (original0) and v (original1)
// and the biases of the 5 x 5 band convs and conv_post -- are read in place from the tensors st_load_param / st_bind_param hold,
// and the effective weights w = v g / ||v|| are engine-owned, recomputed by st_finalize (new tensors) and st_repack (an in-place
// update), not per call.  Kept per training forward: the spectrum and the post-activations of every band's layers 0-4; the leaky
// ReLU's backward reads their signs.
#include "engine_disc.h"
#include "audio_launch.h"
#include "resolution_disc_launch.h"
#include "style_dp_launch.h"

#include <algorithm>
#include <cmath>
#include <string>

using namespace st;
using namespace sthost;

namespace sthost {

constexpr int kRdLayers = 5;                                  // band_convs.c.0 .. band_convs.c.4, then conv_post
constexpr int kRdConvs = kRdBands * kRdLayers + 1;            // index c * 5 + i; the last is conv_post
constexpr int kRdPost = kRdConvs - 1;
constexpr int kRdMaps = kRdBands * (kRdLayers - 1) + 1;       // returned maps: band-major layers 1..4, then conv_post's output

struct RdState : DiscState {
    ~RdState() override { if (wbuf) hipFree(wbuf); if (window) hipFree(window); }
    st_resolution_disc_config cfg{};
    float* wbuf = nullptr;              // the effective weights of the 26 convs, back to back
    float* w[kRdConvs] = {};
    float* window = nullptr;            // hann window, cfg.window_length floats
};

static int rd_cin(int k) { return k == kRdPost ? kRdCh : (k % kRdLayers == 0 ? 2 : kRdCh); }
static int rd_cout(int k) { return k == kRdPost ? 1 : kRdCh; }
static int rd_taps_w(int k) { return k == kRdPost || k % kRdLayers == kRdLayers - 1 ? 3 : 9; }
static int rd_stride_w(int i) { return i >= 1 && i <= 3 ? 2 : 1; }
static int64_t rd_wnumel(int k) { return (int64_t)rd_cout(k) * rd_cin(k) * kRdRows * rd_taps_w(k); }
static std::string rd_name(int k) {
    return k == kRdPost ? std::string("conv_post.") : "band_convs." + std::to_string(k / kRdLayers) + "." + std::to_string(k % kRdLayers) + ".";
}

static void rd_build_params(st_engine* e) {
    for (int k = 0; k < kRdConvs; ++k) {
        expect(e, rd_name(k) + kWnG, {rd_cout(k), 1, 1, 1});
        expect(e, rd_name(k) + kWnV, {rd_cout(k), rd_cin(k), kRdRows, rd_taps_w(k)});
        expect(e, rd_name(k) + "bias", {rd_cout(k)});
    }
}

// frames and bins of the spectrum, the width of band c after layer i, the bands' columns in conv_post's input
struct RdGeom { int W, T, frames, bins, lo[kRdBands], Wd[kRdBands][kRdLayers], off[kRdBands + 1]; };

static RdGeom rd_geom(const st_resolution_disc_config& cfg, int T) {
    RdGeom g{};
    g.W = cfg.window_length; g.T = T;
    g.frames = 1 + T / (g.W / 4);
    g.bins = g.W / 2 + 1;
    for (int c = 0; c < kRdBands; ++c) {
        g.lo[c] = cfg.band_lo[c];
        g.Wd[c][0] = cfg.band_hi[c] - cfg.band_lo[c];
        for (int i = 1; i < kRdLayers; ++i) g.Wd[c][i] = rd_stride_w(i) == 2 ? (g.Wd[c][i - 1] - 1) / 2 + 1 : g.Wd[c][i - 1];
        g.off[c + 1] = g.off[c] + g.Wd[c][kRdLayers - 1];
    }
    return g;
}

// float offsets of what a forward writes besides the returned maps: the spectrum and the post-activations
struct RdActs { size_t spec, a[kRdBands][kRdLayers], end; };

static RdActs rd_acts(int B, const RdGeom& g, bool all_layers) {
    RdActs A{};
    FloatArena ar;
    A.spec = ar.want((size_t)B * 2 * g.frames * g.bins);
    for (int c = 0; c < kRdBands; ++c)
        for (int i = 0; i < (all_layers ? kRdLayers : 1); ++i) A.a[c][i] = ar.want((size_t)B * kRdCh * g.frames * g.Wd[c][i]);
    A.end = ar.off;
    return A;
}

static int rd_check(st_engine* e, int B, int T, RdGeom* g) {
    int rc = check_sizes(e, B, T); if (rc) return rc;
    const RdState* rd = state_of<RdState>(e);
    const int W = rd->cfg.window_length;
    if (T <= W / 2)
        return e->fail(ST_ERR_INVALID, "T = " + std::to_string(T) + " is too short for window_length " + std::to_string(W) + ": the reflect padding of " +
                       std::to_string(W / 2) + " samples needs T > " + std::to_string(W / 2));
    if (B > 65535) return e->fail(ST_ERR_INVALID, "B too large for the resolution discriminator (at most 65535 items)");
    *g = rd_geom(rd->cfg, T);
    if ((int64_t)B * g->frames * W >= ((int64_t)1 << 31) || (int64_t)g->frames * g->bins >= ((int64_t)1 << 30))
        return e->fail(ST_ERR_INVALID, "B * T too large for the resolution discriminator (32-bit frame indexing)");
    return ST_OK;
}

// The forward.  keep = nullptr: the spectrum and layer 0's activations live in the workspace arena and every other layer writes
// its feature map only.  keep != nullptr: the spectrum and all post-activations go to keep's activation buffer as well.
static int rd_forward(st_engine* e, const float* x, float* const* fmaps, int B, const RdGeom& g, SdTrain* keep, hipStream_t s) {
    const RdState* rd = state_of<RdState>(e);
    const float slope = rd->cfg.lrelu_slope;
    const RdActs A = rd_acts(B, g, keep != nullptr);
    int rc;
    float* base;
    if (keep) {
        if ((rc = sd_train_grow(e, &keep->act, &keep->act_cap, A.end * 4))) return rc;
        base = (float*)keep->act;
    } else {
        if ((rc = ensure_ws(e, A.end * 4))) return rc;
        base = (float*)e->ws;
    }
    float* spec = base + A.spec;
    float* a[kRdBands][kRdLayers];
    for (int c = 0; c < kRdBands; ++c) {
        a[c][0] = base + A.a[c][0];
        for (int i = 1; i < kRdLayers; ++i) a[c][i] = keep ? base + A.a[c][i] : fmaps[c * (kRdLayers - 1) + i - 1];
    }
    HIPCHK(e, launch_rd_stft(x, rd->window, spec, g.W, B, g.T, g.frames, s));
    for (int i = 0; i < kRdLayers; ++i) {
        RdConvArgs ca;
        ca.B = B; ca.Cin = i == 0 ? 2 : kRdCh; ca.Cout = kRdCh; ca.frames = g.frames; ca.taps_w = i == kRdLayers - 1 ? 3 : 9;
        ca.stride_w = rd_stride_w(i); ca.slope = slope;
        for (int c = 0; c < kRdBands; ++c) {
            RdBand& bd = ca.band[c];
            const int k = c * kRdLayers + i;
            bd.in = i == 0 ? spec + g.lo[c] : a[c][i - 1];
            bd.in_rs = i == 0 ? g.bins : g.Wd[c][i - 1];
            bd.Win = i == 0 ? g.Wd[c][0] : g.Wd[c][i - 1];
            bd.Wout = g.Wd[c][i];
            bd.w = rd->w[k]; bd.bias = P(e, rd_name(k) + "bias");
            bd.out = a[c][i];
            bd.out2 = keep && i >= 1 ? fmaps[c * (kRdLayers - 1) + i - 1] : nullptr;
        }
        HIPCHK(e, launch_rd_conv(ca, s));
    }
    if (e->capture) {       // st_debug_capture: what no feature map shows -- the spectrum and layer 0's post-activations (their signs)
        capture(e, "spec", spec, (int64_t)B * 2 * g.frames * g.bins, false, s);
        for (int c = 0; c < kRdBands; ++c)
            capture(e, "band_convs." + std::to_string(c) + ".0.act", a[c][0], (int64_t)B * kRdCh * g.frames * g.Wd[c][0], false, s);
    }
    RdPostArgs pa{};
    for (int c = 0; c < kRdBands; ++c) pa.in[c] = a[c][kRdLayers - 1];
    std::copy(g.off, g.off + kRdBands + 1, pa.off);
    pa.w = rd->w[kRdPost]; pa.bias = P(e, rd_name(kRdPost) + "bias"); pa.out = fmaps[kRdMaps - 1];
    pa.B = B; pa.frames = g.frames; pa.slope = slope;
    HIPCHK(e, launch_rd_post_fwd(pa, s));
    return ST_OK;
}

static const DiscKind<RdGeom> kRdKind = {KIND_RESOLUTION_DISC, kRdMaps, "st_resolution_disc_train", rd_check, rd_forward};

}  // namespace sthost

extern "C" {

int st_create_resolution_discriminator(const st_resolution_disc_config* cfg, int device, st_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ST_ERR_INVALID; }
    // the leaky ReLU's backward takes the pre-activation's sign from the kept post-activation: the slope must keep it
    if (!(cfg->lrelu_slope > 0.0f) || !(cfg->lrelu_slope < 1e30f)) { g_create_error = "lrelu_slope must be positive and finite"; return ST_ERR_INVALID; }
    const int W = cfg->window_length;
    if (W < kMelMinNfft || W > kMelMaxNfft || (W & (W - 1)) != 0) {
        g_create_error = "window_length must be a power of two in [32, 2048]";
        return ST_ERR_UNSUPPORTED;
    }
    for (int c = 0; c < kRdBands; ++c) {
        if (cfg->band_lo[c] < 0 || cfg->band_hi[c] > W / 2 + 1) { g_create_error = "a band reaches outside the window_length / 2 + 1 bins"; return ST_ERR_INVALID; }
        if (cfg->band_hi[c] <= cfg->band_lo[c]) { g_create_error = "every band must hold at least one bin"; return ST_ERR_UNSUPPORTED; }
    }
    st_engine* e = nullptr;
    if (int rc = new_handle(KIND_RESOLUTION_DISC, device, std::make_unique<RdState>(), &e)) return rc;
    RdState* rd = state_of<RdState>(e);
    rd->cfg = *cfg;
    rd_build_params(e);
    int64_t total = 0;
    for (int k = 0; k < kRdConvs; ++k) total += (rd_wnumel(k) + 63) / 64 * 64;
    std::vector<float> win(W);
    // torch.hann_window(W) as torch computes it in fp32 (periodic; the angle n * fl(2 pi / W) rounded to fp32 before the cosine):
    // the window of torchaudio's Spectrogram, whose distance from the exact one (~9e-8) would otherwise count as this engine's error
    const float step = (float)(2.0 * M_PI / W);
    for (int n = 0; n < W; ++n) win[n] = 0.5f - 0.5f * (float)std::cos((double)((float)n * step));
    if (hipMalloc((void**)&rd->wbuf, (size_t)total * 4) != hipSuccess || hipMalloc((void**)&rd->window, (size_t)W * 4) != hipSuccess ||
        hipMemcpy(rd->window, win.data(), (size_t)W * 4, hipMemcpyHostToDevice) != hipSuccess) {
        g_create_error = "hipMalloc failed";
        delete e;
        return ST_ERR_HIP;
    }
    int64_t off = 0;
    for (int k = 0; k < kRdConvs; ++k) {
        rd->w[k] = rd->wbuf + off; off += (rd_wnumel(k) + 63) / 64 * 64;
        rd->convs.push_back({rd_name(k), rd->w[k], rd_cout(k), rd_wnumel(k)});
    }
    e->weight_bytes += total * 4 + (int64_t)W * 4;
    *out = e;
    return ST_OK;
}

int st_resolution_disc_fmap_shape(const st_engine* e, int T, int index, int64_t* channels, int64_t* frames, int64_t* width) {
    const RdState* rd = state_if<RdState>(e, KIND_RESOLUTION_DISC);
    if (!rd || !channels || !frames || !width || T < 1 || index < 0 || index >= kRdMaps) return ST_ERR_INVALID;
    if (T <= rd->cfg.window_length / 2) return ST_ERR_INVALID;
    const RdGeom g = rd_geom(rd->cfg, T);
    *frames = g.frames;
    if (index == kRdMaps - 1) { *channels = 1; *width = g.off[kRdBands]; }
    else { *channels = kRdCh; *width = g.Wd[index / (kRdLayers - 1)][index % (kRdLayers - 1) + 1]; }
    return ST_OK;
}

int st_resolution_disc_wgrad_planes(const st_engine* e, int B, int T, int band, int layer) {
    const RdState* rd = state_if<RdState>(e, KIND_RESOLUTION_DISC);
    if (!rd || B < 1 || T <= rd->cfg.window_length / 2 || band < 0 || band >= kRdBands || layer < 0 || layer >= kRdLayers)
        return ST_ERR_INVALID;
    const RdGeom g = rd_geom(rd->cfg, T);
    return rd_wgrad_planes(B, layer == 0 ? 2 : kRdCh, g.frames, g.Wd[band][layer], layer == kRdLayers - 1 ? 3 : 9);
}

int st_resolution_disc_forward(st_engine* e, const float* x, float* const* fmaps, int B, int T, void* stream) {
    return disc_forward(kRdKind, e, x, fmaps, B, T, false, stream);
}

int st_resolution_disc_train_forward(st_engine* e, const float* x, float* const* fmaps, int B, int T, void* stream) {
    return disc_forward(kRdKind, e, x, fmaps, B, T, true, stream);
}

int st_resolution_disc_train_backward(st_engine* e, const float* const* d_fmaps, float* d_x, float* grad_flat, int B, int T, void* stream) {
    RdGeom g;
    DiscBackward bw;
    int rc = disc_backward_begin(kRdKind, e, d_fmaps, d_x, grad_flat, B, T, stream, &g, &bw);
    if (rc || !bw.st) return rc;
    const RdState* rd = state_of<RdState>(e);
    SdTrain* st = bw.st;
    hipStream_t s = bw.s;
    const float slope = rd->cfg.lrelu_slope;
    const int Fr = g.frames, L4 = kRdLayers - 1;

    const RdActs A = rd_acts(B, g, true);
    const float* act = (const float*)st->act;
    const float* spec = act + A.spec;
    const float* a[kRdBands][kRdLayers];
    for (int c = 0; c < kRdBands; ++c) for (int i = 0; i < kRdLayers; ++i) a[c][i] = act + A.a[c][i];
    // scratch: two gradient planes per band, the range sums of the bias / conv_post reductions (no band is wider than the spectrum),
    // one weight-shaped plane, the split-K planes, the spectrum's gradient and the frame rows
    size_t ws = 0;
    if (grad_flat)
        for (int c = 0; c < kRdBands; ++c)
            for (int i = 0; i < kRdLayers; ++i) ws = std::max(ws, rd_wgrad_scratch_floats(B, i == 0 ? 2 : kRdCh, Fr, g.Wd[c][i], i == L4 ? 3 : 9));
    FloatArena ar;
    size_t o_d[kRdBands][2];
    for (int c = 0; c < kRdBands; ++c) for (int j = 0; j < 2; ++j) o_d[c][j] = ar.want((size_t)B * kRdCh * Fr * g.Wd[c][0]);
    const size_t o_red = ar.want(grad_flat ? std::max(rd_bias_scratch_floats(B, Fr, g.bins),
                                                       rd_post_wgrad_scratch_floats(B, Fr, g.off[kRdBands])) : 0);
    const size_t o_dw = ar.want(bw.wmax), o_ws = ar.want(ws), o_dspec = ar.want(d_x ? (size_t)B * 2 * Fr * g.bins : 0),
                 o_rows = ar.want(d_x ? (size_t)B * Fr * g.W : 0);
    if ((rc = sd_train_grow(e, &st->scr, &st->scr_cap, ar.off * 4))) return rc;
    float* scr = (float*)st->scr;
    float* D[kRdBands]; float* Dn[kRdBands];
    for (int c = 0; c < kRdBands; ++c) { D[c] = scr + o_d[c][0]; Dn[c] = scr + o_d[c][1]; }
    float* dW = bw.dW = scr + o_dw; float* wsp = scr + o_ws; float* red = scr + o_red;      // red: the range sums of the O(N) reductions
    auto G = [&](const std::string& n) { return bw.G(n); };
    auto wn_bwd = [&](int k) { return bw.wn_bwd(e, k); };
    // conv_post: the logits' gradient d_fmaps[20] (B, 1, frames, Wc)
    RdPostArgs pa{};
    for (int c = 0; c < kRdBands; ++c) { pa.in[c] = a[c][L4]; pa.addg[c] = d_fmaps[c * L4 + L4 - 1]; pa.dpre[c] = D[c]; }
    std::copy(g.off, g.off + kRdBands + 1, pa.off);
    pa.w = rd->w[kRdPost]; pa.dy = d_fmaps[kRdMaps - 1]; pa.dw = dW; pa.part = red; pa.B = B; pa.frames = Fr; pa.slope = slope;
    if (grad_flat && pa.dy) {
        HIPCHK(e, launch_rd_post_wgrad(pa, s));
        HIPCHK(e, launch_sd_sum_frames(pa.dy, G(rd_name(kRdPost) + "bias"), B, 1, Fr * g.off[kRdBands], 0, s));
        HIPCHK(e, wn_bwd(kRdPost));
    }       // (no logits gradient: the three slices keep the caller's zeros)
    HIPCHK(e, launch_rd_post_dgrad(pa, s));      // D[c] = d pre-activation of band c's layer 4
    for (int i = L4; i >= 0; --i) {
        const int taps_w = i == L4 ? 3 : 9, sw = rd_stride_w(i), Cin = i == 0 ? 2 : kRdCh;
        if (grad_flat) {
            for (int c = 0; c < kRdBands; ++c) {
                const int k = c * kRdLayers + i;
                RdWgradArgs w;
                w.dy = D[c]; w.in = i == 0 ? spec + g.lo[c] : a[c][i - 1]; w.dw = dW; w.scratch = wsp;
                w.B = B; w.Cin = Cin; w.frames = Fr; w.in_rs = i == 0 ? g.bins : g.Wd[c][i - 1]; w.Win = i == 0 ? g.Wd[c][0] : g.Wd[c][i - 1];
                w.Wout = g.Wd[c][i]; w.taps_w = taps_w; w.stride_w = sw;
                HIPCHK(e, launch_rd_wgrad(w, s));
                HIPCHK(e, wn_bwd(k));
            }
            RdBiasArgs ba{};      // the layer's five bias gradients in one launch
            for (int c = 0; c < kRdBands; ++c) { ba.d[c] = D[c]; ba.db[c] = G(rd_name(c * kRdLayers + i) + "bias"); ba.width[c] = g.Wd[c][i]; }
            ba.part = red; ba.B = B; ba.frames = Fr;
            HIPCHK(e, launch_rd_bias_grad(ba, s));
        }
        if (i == 0) break;
        RdConvArgs ca;       // d pre-activation of layer i - 1; layer 0's activation is not returned, so nothing is added there
        ca.B = B; ca.Cin = kRdCh; ca.Cout = kRdCh; ca.frames = Fr; ca.taps_w = taps_w; ca.stride_w = sw; ca.slope = slope;
        for (int c = 0; c < kRdBands; ++c) {
            RdBand& bd = ca.band[c];
            bd.in = D[c]; bd.in_rs = g.Wd[c][i]; bd.Win = g.Wd[c][i]; bd.Wout = g.Wd[c][i - 1];
            bd.w = rd->w[c * kRdLayers + i]; bd.out = Dn[c]; bd.act = a[c][i - 1];
            bd.addg = i >= 2 ? d_fmaps[c * L4 + i - 2] : nullptr;
        }
        HIPCHK(e, launch_rd_conv_dgrad(ca, s));
        for (int c = 0; c < kRdBands; ++c) std::swap(D[c], Dn[c]);
    }
    if (d_x) {
        RdL0DgradArgs la{};
        for (int c = 0; c < kRdBands; ++c) { la.d0[c] = D[c]; la.w[c] = rd->w[c * kRdLayers]; la.lo[c] = g.lo[c]; la.hi[c] = g.lo[c] + g.Wd[c][0]; }
        la.dspec = scr + o_dspec; la.B = B; la.frames = Fr; la.bins = g.bins;
        HIPCHK(e, launch_rd_l0_dgrad(la, s));
        HIPCHK(e, launch_rd_stft_backward(la.dspec, rd->window, scr + o_rows, d_x, g.W, B, g.T, Fr, s));
    }
    return ST_OK;
}

}  // extern "C"
