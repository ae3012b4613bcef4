// DurationPredictor behind the C ABI (st_create_duration_predictor / st_duration_predictor_forward): parameter table and
// launch sequence.  Reference: models/duration_predictor.py:5-37 (eval mode), built as models/model.py:39 does.  All fp32
// (style_dp_kernels.hip): logw feeds ceil(exp(logw)) (model.py:83-84), where a 16-bit error would move whole frames.
#include "engine_internal.h"
#include "style_dp_launch.h"

#include <string>

using namespace st;
using namespace sthost;

namespace sthost {

struct DurState {
    st_duration_predictor_config cfg{};
};

static void duration_build_params(st_engine* e, const st_duration_predictor_config& c) {
    auto expect = [&](const std::string& n, std::vector<int64_t> shape) { Param p; p.shape = std::move(shape); e->params[n] = p; };
    const int64_t Ci = c.in_channels, F = c.filter_channels, K = c.kernel_size, G = c.gin_channels;
    expect("conv1.weight", {F, Ci, K}); expect("conv1.bias", {F});                // duration_predictor.py:16-21
    expect("norm1.weight", {F}); expect("norm1.bias", {F});
    expect("conv2.weight", {F, F, K}); expect("conv2.bias", {F});
    expect("norm2.weight", {F}); expect("norm2.bias", {F});
    expect("proj.weight", {1, F, 1}); expect("proj.bias", {1});
    expect("cond.weight", {Ci, G, 1}); expect("cond.bias", {Ci});                  // :22
}

void duration_destroy(st_engine* e) { delete e->dur; e->dur = nullptr; }

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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return bad("no such HIP device", ST_ERR_HIP);
    if (hipSetDevice(device) != hipSuccess) return bad("hipSetDevice failed", ST_ERR_HIP);
    st_engine* e = new st_engine();
    e->device = device; e->kind = 4;
    e->dur = new DurState();
    e->dur->cfg = *cfg;
    duration_build_params(e, *cfg);
    *out = e;
    return ST_OK;
}

int st_duration_predictor_forward(st_engine* e, const float* x, const float* x_mask, const float* g, float* logw_out,
                                  int B, int Tx, void* stream) {
    if (!e) return ST_ERR_INVALID;
    if (e->kind != 4) return e->fail(ST_ERR_STATE, "this handle is not a duration predictor (st_create_duration_predictor)");
    if (!e->finalized) return e->fail(ST_ERR_STATE, "st_finalize() has not been called after loading parameters");
    if (!x || !x_mask || !g || !logw_out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || Tx < 1) return e->fail(ST_ERR_INVALID, "B and Tx must be >= 1");
    const st_duration_predictor_config& c = e->dur->cfg;
    const int Ci = c.in_channels, F = c.filter_channels, K = c.kernel_size, G = c.gin_channels;
    const int64_t R = (int64_t)B * Tx;
    if (R * F >= ((int64_t)1 << 31) || R * Ci >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "B*Tx too large");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;

    size_t off = 0;
    auto want = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_gb = want((size_t)B * Ci * 4), o_h1 = want((size_t)R * F * 4), o_h2 = want((size_t)R * F * 4);
    int rc = ensure_ws(e, off); if (rc) return rc;
    float* gb = (float*)(e->ws + o_gb); float* h1 = (float*)(e->ws + o_h1); float* h2 = (float*)(e->ws + o_h2);

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
