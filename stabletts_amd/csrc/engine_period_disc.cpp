// DiscriminatorP behind the C ABI (st_create_period_discriminator / st_period_disc_*): parameter table, the weight norm, and the
// launch sequences of the forward and the backward.  Reference: vocoders/vocos/models/discriminator.py:32-75, one handle per
// period.  All fp32 (period_disc_kernels.hip); the parameters -- the weight norm's g (original0) and v (original1) and the
// biases -- are read in place from the tensors st_load_param / st_bind_param hold, and the effective weights w = v g / ||v|| are
// engine-owned buffers recomputed by st_finalize (new tensors) and st_repack (an in-place update), not per call.
// Kept per training forward: the waveform and the post-activations of layers 0-4; the leaky ReLU's backward reads their signs.
#include "engine_disc.h"
#include "style_dp_launch.h"

#include <algorithm>
#include <string>

using namespace st;
using namespace sthost;

namespace sthost {

constexpr int kPdLayers = 5;                                                  // convs.0 .. convs.4, then conv_post
constexpr int kPdCh[kPdLayers + 1] = {1, 32, 128, 512, 1024, 1024};           // channels before layer i / after layer i - 1
constexpr int kPdStride[kPdLayers] = {3, 3, 3, 3, 1};

struct PdState : DiscState {
    st_period_disc_config cfg{};
    float* w[kPdLayers + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};     // effective weights; [5] = conv_post
    ~PdState() override { for (float* p : w) if (p) hipFree(p); }
};

static std::string pd_name(int i) { return i < kPdLayers ? "convs." + std::to_string(i) + "." : std::string("conv_post."); }
static int64_t pd_wnumel(int i) { return i < kPdLayers ? (int64_t)kPdCh[i + 1] * kPdCh[i] * kPdTaps : (int64_t)kPdCh[kPdLayers] * kPdPostTaps; }

static void pd_build_params(st_engine* e) {
    for (int i = 0; i <= kPdLayers; ++i) {
        const int64_t co = i < kPdLayers ? kPdCh[i + 1] : 1, ci = i < kPdLayers ? kPdCh[i] : kPdCh[kPdLayers];
        const int64_t k = i < kPdLayers ? kPdTaps : kPdPostTaps;
        expect(e, pd_name(i) + kWnG, {co, 1, 1, 1});
        expect(e, pd_name(i) + kWnV, {co, ci, k, 1});
        expect(e, pd_name(i) + "bias", {co});
    }
}

// rows of the period view and of every layer's output: H[0] = Tp / p (the input), H[i + 1] after layer i, conv_post keeps H[5]
struct PdGeom { int p, T, Tp, H[kPdLayers + 1]; };

static PdGeom pd_geom(int p, int T) {
    PdGeom g{};
    g.p = p; g.T = T;
    g.Tp = T % p ? T + (p - T % p) : T;
    g.H[0] = g.Tp / p;
    for (int i = 0; i < kPdLayers; ++i) g.H[i + 1] = (g.H[i] - 1) / kPdStride[i] + 1;
    return g;
}

// float offsets into SdTrain::act of what a training forward keeps: the waveform and the post-activations a0 .. a4
struct PdActs { size_t x, a[kPdLayers], widest, end; };

static PdActs pd_acts(int B, const PdGeom& g) {
    PdActs A{};
    FloatArena ar;
    A.x = ar.want((size_t)B * g.T);
    for (int i = 0; i < kPdLayers; ++i) {
        const size_t n = (size_t)B * kPdCh[i + 1] * g.H[i + 1] * g.p;
        A.a[i] = ar.want(n);
        A.widest = std::max(A.widest, n);
    }
    A.end = ar.off;
    return A;
}

static int pd_check(st_engine* e, int B, int T, PdGeom* g) {
    int rc = check_sizes(e, B, T); if (rc) return rc;
    const int p = state_of<PdState>(e)->cfg.period;
    const int n_pad = T % p ? p - T % p : 0;
    if (T <= n_pad)
        return e->fail(ST_ERR_INVALID, "T = " + std::to_string(T) + " is too short for period " + std::to_string(p) + ": the reflect padding of " +
                       std::to_string(n_pad) + " samples needs T > " + std::to_string(n_pad));
    if (B > 65535) return e->fail(ST_ERR_INVALID, "B too large for the period discriminator (at most 65535 items)");
    if ((int64_t)T + p >= ((int64_t)1 << 30)) return e->fail(ST_ERR_INVALID, "T too large for the period discriminator (32-bit frame indexing)");
    *g = pd_geom(p, T);
    return ST_OK;
}

// The forward.  keep = nullptr: a0 lives in the workspace arena and every other layer writes its feature map only.
// keep != nullptr: x and the post-activations a0 .. a4 go to keep's activation buffer as well.
static int pd_forward(st_engine* e, const float* x, float* const* fmaps, int B, const PdGeom& g, SdTrain* keep, hipStream_t s) {
    const PdState* pd = state_of<PdState>(e);
    const int p = g.p;
    const float slope = pd->cfg.lrelu_slope;
    int rc;
    float* a[kPdLayers] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const float* xin = x;
    if (keep) {
        const PdActs A = pd_acts(B, g);
        if ((rc = sd_train_grow(e, &keep->act, &keep->act_cap, A.end * 4))) return rc;
        float* act = (float*)keep->act;
        HIPCHK(e, hipMemcpyAsync(act + A.x, x, (size_t)B * g.T * 4, hipMemcpyDeviceToDevice, s));
        xin = act + A.x;
        for (int i = 0; i < kPdLayers; ++i) a[i] = act + A.a[i];
    } else {
        if ((rc = ensure_ws(e, (size_t)B * kPdCh[1] * g.H[1] * p * 4))) return rc;
        a[0] = (float*)e->ws;
        for (int i = 1; i < kPdLayers; ++i) a[i] = fmaps[i - 1];
    }
    HIPCHK(e, launch_pd_l0_fwd(xin, pd->w[0], P(e, pd_name(0) + "bias"), a[0], B, g.T, g.Tp, g.H[1], p, slope, s));
    for (int i = 1; i < kPdLayers; ++i) {
        PdConvArgs c;
        c.in = a[i - 1]; c.w = pd->w[i]; c.bias = P(e, pd_name(i) + "bias"); c.out = a[i]; c.out2 = keep ? fmaps[i - 1] : nullptr;
        c.B = B; c.Cin = kPdCh[i]; c.Cout = kPdCh[i + 1]; c.Hin = g.H[i]; c.Hout = g.H[i + 1]; c.p = p; c.stride = kPdStride[i]; c.slope = slope;
        HIPCHK(e, launch_pd_conv(c, s));
    }
    HIPCHK(e, launch_pd_post_fwd(a[4], pd->w[kPdLayers], P(e, pd_name(kPdLayers) + "bias"), fmaps[4], nullptr, B, kPdCh[kPdLayers], g.H[kPdLayers], p, s));
    return ST_OK;
}

static const DiscKind<PdGeom> kPdKind = {KIND_PERIOD_DISC, kPdLayers, "st_period_disc_train", pd_check, pd_forward};

}  // namespace sthost

extern "C" {

int st_create_period_discriminator(const st_period_disc_config* cfg, int device, st_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ST_ERR_INVALID; }
    if (cfg->period < 1) { g_create_error = "period must be >= 1"; return ST_ERR_INVALID; }
    // the leaky ReLU's backward takes the pre-activation's sign from the kept post-activation: the slope must keep it
    if (!(cfg->lrelu_slope > 0.0f) || !(cfg->lrelu_slope < 1e30f)) { g_create_error = "lrelu_slope must be positive and finite"; return ST_ERR_INVALID; }
    st_engine* e = nullptr;
    if (int rc = new_handle(KIND_PERIOD_DISC, device, std::make_unique<PdState>(), &e)) return rc;
    PdState* pd = state_of<PdState>(e);
    pd->cfg = *cfg;
    pd_build_params(e);
    for (int i = 0; i <= kPdLayers; ++i) {
        if (hipMalloc((void**)&pd->w[i], (size_t)pd_wnumel(i) * 4) != hipSuccess) {
            g_create_error = "hipMalloc failed";
            delete e;
            return ST_ERR_HIP;
        }
        e->weight_bytes += pd_wnumel(i) * 4;
        pd->convs.push_back({pd_name(i), pd->w[i], i < kPdLayers ? kPdCh[i + 1] : 1, pd_wnumel(i)});
    }
    *out = e;
    return ST_OK;
}

int st_period_disc_fmap_shape(const st_engine* e, int T, int index, int64_t* channels, int64_t* rows) {
    const PdState* pd = state_if<PdState>(e, KIND_PERIOD_DISC);
    if (!pd || !channels || !rows || T < 1 || index < 0 || index >= kPdLayers) return ST_ERR_INVALID;
    const int p = pd->cfg.period;
    if (T <= (T % p ? p - T % p : 0)) return ST_ERR_INVALID;
    const PdGeom g = pd_geom(p, T);
    *channels = index < kPdLayers - 1 ? kPdCh[index + 2] : 1;
    *rows = index < kPdLayers - 1 ? g.H[index + 2] : g.H[kPdLayers];
    return ST_OK;
}

int st_period_disc_forward(st_engine* e, const float* x, float* const* fmaps, int B, int T, void* stream) {
    return disc_forward(kPdKind, e, x, fmaps, B, T, false, stream);
}

int st_period_disc_train_forward(st_engine* e, const float* x, float* const* fmaps, int B, int T, void* stream) {
    return disc_forward(kPdKind, e, x, fmaps, B, T, true, stream);
}

int st_period_disc_train_backward(st_engine* e, const float* const* d_fmaps, float* d_x, float* grad_flat, int B, int T, void* stream) {
    PdGeom g;
    DiscBackward bw;
    int rc = disc_backward_begin(kPdKind, e, d_fmaps, d_x, grad_flat, B, T, stream, &g, &bw);
    if (rc || !bw.st) return rc;
    const PdState* pd = state_of<PdState>(e);
    SdTrain* st = bw.st;
    hipStream_t s = bw.s;
    const int p = g.p;
    const float slope = pd->cfg.lrelu_slope;

    const PdActs A = pd_acts(B, g);
    const float* act = (const float*)st->act;
    const float* x = act + A.x;
    const float* a[kPdLayers];
    for (int i = 0; i < kPdLayers; ++i) a[i] = act + A.a[i];
    // scratch: two gradient planes, one weight-shaped plane, the split-K planes, layer 0's partial sums
    size_t ws = 0;
    if (grad_flat)
        for (int i = 1; i < kPdLayers; ++i) ws = std::max(ws, pd_wgrad_scratch_floats(B, kPdCh[i], kPdCh[i + 1], g.H[i + 1], p));
    FloatArena ar;
    const size_t o_d0 = ar.want(A.widest), o_d1 = ar.want(A.widest), o_dw = ar.want(bw.wmax), o_ws = ar.want(ws),
                 o_l0 = ar.want(grad_flat ? pd_l0_scratch_floats(B, g.H[1], p) : 0);
    if ((rc = sd_train_grow(e, &st->scr, &st->scr_cap, ar.off * 4))) return rc;
    float* scr = (float*)st->scr;
    float* D = scr + o_d0; float* Dn = scr + o_d1; float* dW = bw.dW = scr + o_dw; float* wsp = scr + o_ws; float* l0p = scr + o_l0;
    auto G = [&](const std::string& n) { return bw.G(n); };
    auto wn_bwd = [&](int i) { return bw.wn_bwd(e, i); };
    // conv_post: the logits' gradient d_fmaps[4] (B, 1, H, p)
    const int C4 = kPdCh[kPdLayers], H4 = g.H[kPdLayers];
    const float* dy = d_fmaps[4];
    if (grad_flat) {
        if (dy) {
            HIPCHK(e, launch_pd_post_wgrad(dy, a[4], dW, B, C4, H4, p, s));
            HIPCHK(e, launch_sd_sum_frames(dy, G(pd_name(kPdLayers) + "bias"), B, 1, H4 * p, 0, s));
            HIPCHK(e, wn_bwd(kPdLayers));
        }       // (no logits gradient: the three slices keep the caller's zeros)
    }
    HIPCHK(e, launch_pd_post_dgrad(dy, pd->w[kPdLayers], a[4], d_fmaps[3], D, B, C4, H4, p, slope, s));      // D = d pre-activation of layer 4
    for (int i = kPdLayers - 1; i >= 1; --i) {
        const int Cin = kPdCh[i], Cout = kPdCh[i + 1];
        if (grad_flat) {
            PdWgradArgs w;
            w.dy = D; w.in = a[i - 1]; w.dw = dW; w.scratch = wsp; w.B = B; w.Cin = Cin; w.Cout = Cout; w.Hin = g.H[i]; w.Hout = g.H[i + 1];
            w.p = p; w.stride = kPdStride[i];
            HIPCHK(e, launch_pd_wgrad(w, s));
            HIPCHK(e, launch_sd_sum_frames(D, G(pd_name(i) + "bias"), B, Cout, g.H[i + 1] * p, 0, s));
            HIPCHK(e, wn_bwd(i));
        }
        PdConvArgs c;       // d pre-activation of layer i - 1: the feature map below layer 1 is not returned, so nothing is added there
        c.in = D; c.w = pd->w[i]; c.out = Dn; c.act = a[i - 1]; c.addg = i >= 2 ? d_fmaps[i - 2] : nullptr;
        c.B = B; c.Cin = Cout; c.Cout = Cin; c.Hin = g.H[i + 1]; c.Hout = g.H[i]; c.p = p; c.stride = kPdStride[i]; c.slope = slope;
        HIPCHK(e, launch_pd_conv_dgrad(c, s));
        std::swap(D, Dn);
    }
    if (grad_flat) {
        HIPCHK(e, launch_pd_l0_wgrad(D, x, dW, G(pd_name(0) + "bias"), l0p, B, g.T, g.Tp, g.H[1], p, s));
        HIPCHK(e, wn_bwd(0));
    }
    if (d_x) HIPCHK(e, launch_pd_l0_dgrad(D, pd->w[0], d_x, B, g.T, g.Tp, g.H[1], p, s));
    return ST_OK;
}

}  // extern "C"
