// DurationPredictor behind the C ABI (st_create_duration_predictor / st_duration_predictor_forward): parameter table and
// launch sequence.  Reference: models/duration_predictor.py:5-37 (eval mode), built as models/model.py:39 does.  All fp32
// (style_dp_kernels.hip): logw feeds ceil(exp(logw)) (model.py:83-84), where a 16-bit error would move whole frames.
#include "engine_internal.h"
#include "style_dp_launch.h"

#include <algorithm>
#include <string>

using namespace st;
using namespace sthost;

namespace sthost {

// Reads the loaded parameters in place: nothing to pack
struct DurState : HeldState {
    st_duration_predictor_config cfg{};
    DurState() : HeldState("st_repack: style-encoder / duration-predictor handles read their parameters in place") {}
};

static void duration_build_params(st_engine* e, const st_duration_predictor_config& c) {
    const int64_t Ci = c.in_channels, F = c.filter_channels, K = c.kernel_size, G = c.gin_channels;
    expect(e, "conv1.weight", {F, Ci, K}); expect(e, "conv1.bias", {F});                // duration_predictor.py:16-21
    expect(e, "norm1.weight", {F}); expect(e, "norm1.bias", {F});
    expect(e, "conv2.weight", {F, F, K}); expect(e, "conv2.bias", {F});
    expect(e, "norm2.weight", {F}); expect(e, "norm2.bias", {F});
    expect(e, "proj.weight", {1, F, 1}); expect(e, "proj.bias", {1});
    expect(e, "cond.weight", {Ci, G, 1}); expect(e, "cond.bias", {Ci});                  // :22
}

}  // namespace sthost

extern "C" {

int st_create_duration_predictor(const st_duration_predictor_config* cfg, int device, st_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ST_ERR_INVALID; }
    auto bad = [&](const char* m, int code) { g_create_error = m; return code; };
    if (cfg->in_channels < 1 || cfg->filter_channels < 1 || cfg->kernel_size < 1 || cfg->gin_channels < 1)
        return bad("sizes must be positive", ST_ERR_INVALID);
    // limits of this native build
    if (cfg->filter_channels % 128 != 0) return bad("filter_channels must be a multiple of 128", ST_ERR_UNSUPPORTED);
    if (cfg->kernel_size != 1 && cfg->kernel_size != 3 && cfg->kernel_size != 5) return bad("native convolutions are built for kernel_size 1, 3 or 5", ST_ERR_UNSUPPORTED);
    auto state = std::make_unique<DurState>();
    state->cfg = *cfg;
    st_engine* e = nullptr;
    if (int rc = new_handle(KIND_DURATION_PREDICTOR, device, std::move(state), &e)) return rc;
    duration_build_params(e, *cfg);
    *out = e;
    return ST_OK;
}

int st_duration_predictor_forward(st_engine* e, const float* x, const float* x_mask, const float* g, float* logw_out,
                                  int B, int Tx, void* stream) {
    int rc = check_handle(e, KIND_DURATION_PREDICTOR); if (rc) return rc;
    if ((rc = check_finalized(e))) return rc;
    if (!x || !x_mask || !g || !logw_out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if ((rc = check_sizes(e, B, Tx, "Tx"))) return rc;
    const st_duration_predictor_config& c = state_of<DurState>(e)->cfg;
    const int Ci = c.in_channels, F = c.filter_channels, K = c.kernel_size, G = c.gin_channels;
    const int64_t R = (int64_t)B * Tx;
    if (R * F >= ((int64_t)1 << 31) || R * Ci >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "B*Tx too large");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;

    FloatArena ar;
    const size_t o_gb = ar.want((size_t)B * Ci), o_h1 = ar.want((size_t)R * F), o_h2 = ar.want((size_t)R * F);
    if ((rc = ensure_ws(e, ar.off * 4))) return rc;
    float* ws = (float*)e->ws;
    float* gb = ws + o_gb; float* h1 = ws + o_h1; float* h2 = ws + o_h2;

    {   // cond(g) (:26): a k = 1 conv over a one-frame input -> per-item bias of in_channels
        SdConvArgs a; a.in = g; a.Cin = G; a.w = P(e, "cond.weight"); a.bias = P(e, "cond.bias"); a.out = gb; a.Cout = Ci;
        a.B = B; a.T = 1; a.taps = 1;
        HIPCHK(e, launch_sd_conv(a, s));
    }
    {   // conv1((x + cond(g)) * x_mask) -> relu -> norm1 (:26-29)
        SdConvArgs a; a.in = x; a.addv = gb; a.imask = x_mask; a.Cin = Ci; a.w = P(e, "conv1.weight"); a.bias = P(e, "conv1.bias");
        a.out = h1; a.Cout = F; a.B = B; a.T = Tx; a.taps = K; a.epi = SD_EPI_RELU;
        HIPCHK(e, launch_sd_conv(a, s));
        HIPCHK(e, launch_sd_layernorm_channels(h1, P(e, "norm1.weight"), P(e, "norm1.bias"), 1e-5f, B, F, Tx, s));
    }
    {   // conv2(x * x_mask) -> relu -> norm2 (:31-33)
        SdConvArgs a; a.in = h1; a.imask = x_mask; a.Cin = F; a.w = P(e, "conv2.weight"); a.bias = P(e, "conv2.bias");
        a.out = h2; a.Cout = F; a.B = B; a.T = Tx; a.taps = K; a.epi = SD_EPI_RELU;
        HIPCHK(e, launch_sd_conv(a, s));
        HIPCHK(e, launch_sd_layernorm_channels(h2, P(e, "norm2.weight"), P(e, "norm2.bias"), 1e-5f, B, F, Tx, s));
    }
    {   // proj(x * x_mask) * x_mask (:35-36)
        SdConvArgs a; a.in = h2; a.imask = x_mask; a.omask = x_mask; a.Cin = F; a.w = P(e, "proj.weight"); a.bias = P(e, "proj.bias");
        a.out = logw_out; a.Cout = 1; a.B = B; a.T = Tx; a.taps = 1;
        HIPCHK(e, launch_sd_conv(a, s));
    }
    return ST_OK;
}

}  // extern "C"

// ---- training: the forward above with its activations kept and dropout after norm1 / norm2 (salts 72, 73), and the
// backward.  x and g get no gradient (the reference detaches them, :25-26); cond's gradient comes from conv1's data gradient.
namespace {

struct DurActs {        // float offsets into SdTrain::act; R = B * Tx
    size_t x, mask, g, gb, r1, m1, s1, d1, r2, m2, s2, d2, end;
};

DurActs dur_acts(const st_duration_predictor_config& c, int B, int T) {
    const size_t R = (size_t)B * T, F = c.filter_channels;
    DurActs a{};
    FloatArena ar;
    a.x = ar.want(R * c.in_channels); a.mask = ar.want(R); a.g = ar.want((size_t)B * c.gin_channels); a.gb = ar.want((size_t)B * c.in_channels);
    a.r1 = ar.want(R * F); a.m1 = ar.want(R); a.s1 = ar.want(R); a.d1 = ar.want(R * F);
    a.r2 = ar.want(R * F); a.m2 = ar.want(R); a.s2 = ar.want(R); a.d2 = ar.want(R * F);
    a.end = ar.off;
    return a;
}

}  // namespace

extern "C" {

int st_duration_predictor_train_forward(st_engine* e, const float* x, const float* x_mask, const float* g, float* logw_out,
                                        int B, int Tx, float p_dropout, uint64_t seed, void* stream) {
    int rc = check_handle(e, KIND_DURATION_PREDICTOR); if (rc) return rc;
    if ((rc = check_finalized(e))) return rc;
    if (!x || !x_mask || !g || !logw_out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if ((rc = check_sizes(e, B, Tx, "Tx"))) return rc;
    if ((rc = check_dropout(e, p_dropout))) return rc;
    const st_duration_predictor_config& c = state_of<DurState>(e)->cfg;
    const int Ci = c.in_channels, F = c.filter_channels, K = c.kernel_size, Gc = c.gin_channels;
    const int64_t R = (int64_t)B * Tx;
    if (R * F >= ((int64_t)1 << 31) || R * Ci >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "B*Tx too large");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    SdTrain* st = state_of<DurState>(e)->begin();
    const DurActs A = dur_acts(c, B, Tx);
    if ((rc = sd_train_grow(e, &st->act, &st->act_cap, A.end * 4))) return rc;
    float* act = (float*)st->act;
    auto at = [&](size_t o) { return act + o; };
    HIPCHK(e, hipMemcpyAsync(at(A.x), x, (size_t)R * Ci * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(at(A.mask), x_mask, (size_t)R * 4, hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(at(A.g), g, (size_t)B * Gc * 4, hipMemcpyDeviceToDevice, s));
    const float* mask = at(A.mask);
    const SdDrop d1 = sd_make_drop(p_dropout, seed, 72), d2 = sd_make_drop(p_dropout, seed, 73);
    {   // cond(g): per-item bias of in_channels
        SdConvArgs a; a.in = at(A.g); a.Cin = Gc; a.w = P(e, "cond.weight"); a.bias = P(e, "cond.bias"); a.out = at(A.gb); a.Cout = Ci;
        a.B = B; a.T = 1; a.taps = 1;
        HIPCHK(e, launch_sd_conv(a, s));
    }
    {   // relu(conv1((x + cond(g)) * x_mask)) -> norm1 -> dropout
        SdConvArgs a; a.in = at(A.x); a.addv = at(A.gb); a.imask = mask; a.Cin = Ci; a.w = P(e, "conv1.weight"); a.bias = P(e, "conv1.bias");
        a.out = at(A.r1); a.Cout = F; a.B = B; a.T = Tx; a.taps = K; a.epi = SD_EPI_RELU;
        HIPCHK(e, launch_sd_conv(a, s));
        HIPCHK(e, launch_sd_layernorm_train(at(A.r1), at(A.d1), at(A.m1), at(A.s1), P(e, "norm1.weight"), P(e, "norm1.bias"), 1e-5f, d1, B, F, Tx, s));
    }
    {   // relu(conv2(x * x_mask)) -> norm2 -> dropout
        SdConvArgs a; a.in = at(A.d1); a.imask = mask; a.Cin = F; a.w = P(e, "conv2.weight"); a.bias = P(e, "conv2.bias");
        a.out = at(A.r2); a.Cout = F; a.B = B; a.T = Tx; a.taps = K; a.epi = SD_EPI_RELU;
        HIPCHK(e, launch_sd_conv(a, s));
        HIPCHK(e, launch_sd_layernorm_train(at(A.r2), at(A.d2), at(A.m2), at(A.s2), P(e, "norm2.weight"), P(e, "norm2.bias"), 1e-5f, d2, B, F, Tx, s));
    }
    {   // proj(x * x_mask) * x_mask
        SdConvArgs a; a.in = at(A.d2); a.imask = mask; a.omask = mask; a.Cin = F; a.w = P(e, "proj.weight"); a.bias = P(e, "proj.bias");
        a.out = logw_out; a.Cout = 1; a.B = B; a.T = Tx; a.taps = 1;
        HIPCHK(e, launch_sd_conv(a, s));
    }
    sd_train_commit(st, B, Tx, p_dropout, seed, true);
    return ST_OK;
}

int st_duration_predictor_train_backward(st_engine* e, int64_t serial, int B, int Tx, const float* grad_logw, float* grad_flat,
                                         void* stream) {
    int rc = check_handle(e, KIND_DURATION_PREDICTOR); if (rc) return rc;
    if (!grad_logw || !grad_flat) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    DurState* dur = state_of<DurState>(e);
    SdTrain* st = &dur->held;
    if ((rc = sd_train_check(e, *st, "st_duration_predictor_train", "Tx", serial, B, Tx))) return rc;
    const st_duration_predictor_config& c = dur->cfg;
    const int Ci = c.in_channels, F = c.filter_channels, K = c.kernel_size, Gc = c.gin_channels;
    const int64_t R = (int64_t)B * Tx;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    const DurActs A = dur_acts(c, B, Tx);
    float* act = (float*)st->act;
    auto at = [&](size_t o) { return act + o; };
    const float* mask = at(A.mask);
    const SdDrop d1 = sd_make_drop(st->p, st->seed, 72), d2 = sd_make_drop(st->p, st->seed, 73);

    size_t ws = 0;
    ws = std::max(ws, sd_wgrad_scratch_floats(B, F, 1, Tx, 1));
    ws = std::max(ws, sd_wgrad_scratch_floats(B, F, F, Tx, K));
    ws = std::max(ws, sd_wgrad_scratch_floats(B, Ci, F, Tx, K));
    ws = std::max(ws, sd_wgrad_scratch_floats(B, Gc, Ci, 1, 1));
    FloatArena ar;
    const size_t o_dy = ar.want(R), o_a = ar.want(R * F), o_b = ar.want(R * F), o_dx = ar.want(R * Ci), o_dc = ar.want((size_t)B * Ci), o_ws = ar.want(ws);
    if ((rc = sd_train_grow(e, &st->scr, &st->scr_cap, ar.off * 4))) return rc;
    float* scr = (float*)st->scr;
    float* dY = scr + o_dy; float* Pa = scr + o_a; float* Pb = scr + o_b; float* dX = scr + o_dx; float* dC = scr + o_dc; float* wsp = scr + o_ws;

    std::map<std::string, int64_t> goff;
    train_grad_layout(e, &goff);
    auto G = [&](const std::string& n) { return grad_flat + goff.at(n); };
    auto wb = [&](const std::string& w, const std::string& b, const float* dy, int cout, const float* x, const float* addv, int cin, int taps, int T) {
        SdWgradArgs a; a.dy = dy; a.in = x; a.addv = addv; a.dw = G(w); a.scratch = wsp;
        a.imask = x == at(A.g) ? nullptr : mask;      // (cond: one frame per item, no mask)
        a.B = B; a.Cin = cin; a.Cout = cout; a.T = T; a.taps = taps;
        hipError_t r = launch_sd_wgrad(a, s);
        if (r != hipSuccess) return r;
        return launch_sd_sum_frames(dy, G(b), B, cout, T, 0, s);
    };
    auto dgrad = [&](const std::string& w, const float* dy, int cout, int cin, int taps, float* out) {     // masked: the input mask
        SdConvArgs a; a.in = dy; a.Cin = cout; a.w = P(e, w); a.out = out; a.Cout = cin; a.B = B; a.T = Tx; a.taps = taps; a.omask = mask;
        return launch_sd_conv_dgrad(a, s);
    };
    HIPCHK(e, launch_sd_mul_mask(grad_logw, mask, dY, B, 1, Tx, s));                      // logw = proj(.) * x_mask
    HIPCHK(e, wb("proj.weight", "proj.bias", dY, 1, at(A.d2), nullptr, F, 1, Tx));
    HIPCHK(e, dgrad("proj.weight", dY, 1, F, 1, Pa));                                      // d (dropped norm2 output)
    HIPCHK(e, launch_sd_layernorm_bwd(Pa, at(A.r2), at(A.m2), at(A.s2), P(e, "norm2.weight"), Pb, G("norm2.weight"), G("norm2.bias"), d2, 1, B, F, Tx, s));
    HIPCHK(e, wb("conv2.weight", "conv2.bias", Pb, F, at(A.d1), nullptr, F, K, Tx));
    HIPCHK(e, dgrad("conv2.weight", Pb, F, F, K, Pa));
    HIPCHK(e, launch_sd_layernorm_bwd(Pa, at(A.r1), at(A.m1), at(A.s1), P(e, "norm1.weight"), Pb, G("norm1.weight"), G("norm1.bias"), d1, 1, B, F, Tx, s));
    HIPCHK(e, wb("conv1.weight", "conv1.bias", Pb, F, at(A.x), at(A.gb), Ci, K, Tx));
    HIPCHK(e, dgrad("conv1.weight", Pb, F, Ci, K, dX));                                    // d (x + cond(g)), masked
    HIPCHK(e, launch_sd_sum_frames(dX, dC, B, Ci, Tx, 1, s));                              // d cond(g)[b] = sum over frames
    HIPCHK(e, wb("cond.weight", "cond.bias", dC, Ci, at(A.g), nullptr, Gc, 1, 1));
    return ST_OK;
}

}  // extern "C"
