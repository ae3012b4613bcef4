// MelStyleEncoder behind the C ABI (st_create_style_encoder / st_style_encoder_forward): parameter table and launch
// sequence.  Reference: models/reference_encoder.py:22-93 (eval mode), built as models/model.py:38 does.  All fp32
// (style_dp_kernels.hip); the parameters are read in place from the tensors st_load_param / st_bind_param hold.
#include "engine_internal.h"
#include "style_dp_launch.h"

#include <string>

using namespace st;
using namespace sthost;

namespace sthost {

struct StyleState {
    st_style_encoder_config cfg{};
};

static void style_build_params(st_engine* e, const st_style_encoder_config& c) {
    auto expect = [&](const std::string& n, std::vector<int64_t> shape) { Param p; p.shape = std::move(shape); e->params[n] = p; };
    const int64_t I = c.n_mel_channels, Hd = c.style_hidden, O = c.style_vector_dim, K = c.style_kernel_size;
    expect("spectral.0.weight", {Hd, I}); expect("spectral.0.bias", {Hd});             // reference_encoder.py:44-51
    expect("spectral.3.weight", {Hd, Hd}); expect("spectral.3.bias", {Hd});
    for (int i = 0; i < 2; ++i) {                                                      // :53-56, Conv1dGLU :13
        const std::string p = "temporal." + std::to_string(i) + ".conv1.";
        expect(p + "weight", {2 * Hd, Hd, K}); expect(p + "bias", {2 * Hd});
    }
    expect("slf_attn.in_proj_weight", {3 * Hd, Hd}); expect("slf_attn.in_proj_bias", {3 * Hd});     // :58-63
    expect("slf_attn.out_proj.weight", {Hd, Hd}); expect("slf_attn.out_proj.bias", {Hd});
    expect("fc.weight", {O, Hd}); expect("fc.bias", {O});                              // :65
}

void style_destroy(st_engine* e) { delete e->sty; e->sty = nullptr; }

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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return bad("no such HIP device", ST_ERR_HIP);
    if (hipSetDevice(device) != hipSuccess) return bad("hipSetDevice failed", ST_ERR_HIP);
    st_engine* e = new st_engine();
    e->device = device; e->kind = 3;
    e->sty = new StyleState();
    e->sty->cfg = *cfg;
    style_build_params(e, *cfg);
    *out = e;
    return ST_OK;
}

int st_style_encoder_forward(st_engine* e, const float* mel, const float* mask, float* c_out, int B, int T, void* stream) {
    if (!e) return ST_ERR_INVALID;
    if (e->kind != 3) return e->fail(ST_ERR_STATE, "this handle is not a style encoder (st_create_style_encoder)");
    if (!e->finalized) return e->fail(ST_ERR_STATE, "st_finalize() has not been called after loading parameters");
    if (!mel || !c_out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if (B < 1 || T < 1) return e->fail(ST_ERR_INVALID, "B and T must be >= 1");
    const st_style_encoder_config& c = e->sty->cfg;
    const int I = c.n_mel_channels, Hd = c.style_hidden, O = c.style_vector_dim, K = c.style_kernel_size, NH = c.style_head;
    const int64_t R = (int64_t)B * T;
    if (R * 3 * Hd >= ((int64_t)1 << 31) || R * O >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "B*T too large");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;

    // workspace: two hidden planes, the GLU / q-k-v plane, the fc output (all (B, C, T) fp32)
    size_t off = 0;
    auto want = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t o_h1 = want((size_t)R * Hd * 4), o_h2 = want((size_t)R * Hd * 4), o_u = want((size_t)R * 3 * Hd * 4), o_f = want((size_t)R * O * 4);
    int rc = ensure_ws(e, off); if (rc) return rc;
    float* h1 = (float*)(e->ws + o_h1); float* h2 = (float*)(e->ws + o_h2); float* u = (float*)(e->ws + o_u); float* f = (float*)(e->ws + o_f);

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
