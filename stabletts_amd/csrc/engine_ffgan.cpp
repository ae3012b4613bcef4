// FireflyGAN vocoder behind the C ABI (st_create_ffgan / st_ffgan_forward / st_ffgan_forward_ragged): parameter table, weight-norm fold and packing, and the
// launch sequence.  Reference: vocoders/ffgan/model.py:7-29,44-57, backbone.py:78-214, head.py:25-133,136-249 (use_template=False).
// The ConvNeXt encoder runs like the Vocos backbone (engine_vocos.cpp): its GEMMs on the implicit-GEMM kernels of the decoder over
// the flattened rows of the batch, the row kernels at a run-time width.  The HiFi-GAN head runs on the convolution family of
// ffgan_kernels.hip, every level a time-major [item][L][C] tensor.
// Split-precision handles (ST_OPERAND_*_SPLIT; FfganState::split): every MFMA operand is a hi + lo pair of the 16-bit format and every
// product three MFMAs (f16: lo * lo dropped) or, in the encoder, four (bf16: its lo * lo is as large as what the pair loses; the head
// goes further for bf16 and carries three parts, ffgan_launch.h).  An encoder operand is one
// pair tensor [row][hi | lo], the GEMM source a0 with c0 = 2 K, and c2 re-reads it: K = [a_hi | a_lo | a_hi] against
// [W_hi | W_hi | W_lo], or K = [a_hi | a_lo | a_hi | a_lo] against [W_hi | W_hi | W_lo | W_lo] (pwconv1 as an fp32-output GEMM, then the
// GELU row kernel that writes the pair); the head runs the SPLIT instantiations of its convolution family on fp32 tensors: c1
// stores its fp32 pre-activation and c2 applies the SiLU while it stages it.
#include "engine_vocoder.h"
#include "ffgan_launch.h"
#include "vocos_launch.h"

#include <algorithm>
#include <string>

using namespace st;
using namespace sthost;

namespace sthost {

struct FfConv {             // one convolution of the head: fragment-ordered 16-bit weights + fp32 bias
    void* wfrag = nullptr;
    const float* bias = nullptr;
    int cin = 0, cout = 0, taps = 0, dil = 1;
};

struct FfganState : KindState {
    FfganState() : KindState("st_repack: vocoder handles re-pack through st_finalize") {}
    ~FfganState() override { slots.destroy(); }
    int finalize(st_engine* e) override;
    st_ffgan_config cfg{};
    int hop = 1;
    bool split = false;                               // hi + lo operand pairs (e->dt names their 16-bit format)
    int parts() const { return !split ? 1 : cfg.operand_dtype == ST_OPERAND_BF16_SPLIT ? 4 : 3; }      // K slices of an encoder GEMM
    Conv stem;
    std::vector<Conv> down;                           // the k = 1 downsample convs of stages 1..
    std::vector<std::vector<Conv>> pw1, pw2;          // [stage][block]
    FfConv pre;
    std::vector<FfConv> ups;
    std::vector<std::vector<std::vector<FfConv>>> c1, c2;      // [level][resblock][pair]
    float* post_w = nullptr;                          // [taps][C] fp32
    UttSlots slots;                                   // ragged calls: the utterance tables (utt_slots.h)
};

static const std::string kWn0 = "parametrizations.weight.original0", kWn1 = "parametrizations.weight.original1";
static std::string ds(int i, int j) { return "backbone.downsample_layers." + std::to_string(i) + "." + std::to_string(j) + "."; }
static std::string blk(int i, int j) { return "backbone.stages." + std::to_string(i) + "." + std::to_string(j) + "."; }
static std::string rb(int i, int b, int which, int p) {
    return "head.resblocks." + std::to_string(i) + ".blocks." + std::to_string(b) + ".convs" + std::to_string(which) + "." + std::to_string(p) + ".";
}
static int head_width(const st_ffgan_config& c, int level) { return c.upsample_initial_channel >> level; }      // level 0: conv_pre's output

// The limits of the native kernels (include/stabletts_hip.h: st_ffgan_config); nullptr: supported
static const char* ffgan_unsupported(const st_ffgan_config& c) {
    if (c.operand_dtype != ST_OPERAND_BF16 && c.operand_dtype != ST_OPERAND_F16 && c.operand_dtype != ST_OPERAND_BF16_SPLIT &&
        c.operand_dtype != ST_OPERAND_F16_SPLIT)
        return "operand_dtype";
    if (c.use_template) return "use_template: the native head is built without the noise convolutions (use_template=False)";
    if (c.input_channels % 64 != 0 || c.input_channels < 64 || c.input_channels > 192) return "input_channels must be 64, 128 or 192";
    if (c.kernel_size != 7) return "the native encoder kernels are built for kernel_size == 7";
    if (c.n_stages < 1 || c.n_stages > ST_FFGAN_MAX_STAGES) return "the encoder has 1..8 stages";
    for (int i = 0; i < c.n_stages; ++i) {
        if (c.depths[i] < 1 || c.depths[i] > 64) return "encoder depths must be in [1, 64]";
        if (c.dims[i] < 128 || c.dims[i] % 128 != 0 || c.dims[i] > kFfgMaxDim) return "encoder widths must be multiples of 128 up to 1024 (the GEMM and row kernels)";
    }
    if (c.n_upsamples < 1 || c.n_upsamples > ST_FFGAN_MAX_UPSAMPLES) return "the head has 1..8 upsamples";
    const int c0 = c.upsample_initial_channel;
    if (c0 < 16 || c0 > 1024 || (c0 & (c0 - 1)) != 0) return "head widths must be 16 * 2^n: upsample_initial_channel is a power of two in [16, 1024]";
    if ((c0 >> c.n_upsamples) < 16) return "head widths must be 16 * 2^n: the last level has fewer than 16 channels";
    for (int i = 0; i < c.n_upsamples; ++i) {
        const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
        if (u < 2 || u > 16 || (u & 1)) return "upsample rates must be even, in [2, 16]";
        if (k != 2 * u) return "the native transposed convolution is built for upsample_kernel_size == 2 * upsample_rate";
    }
    if (c.n_resblocks < 1 || c.n_resblocks > ST_FFGAN_MAX_RESBLOCKS) return "a ParralelBlock has 1..4 resblocks";
    if (c.n_dilations < 1 || c.n_dilations > ST_FFGAN_MAX_DILATIONS) return "a resblock has 1..4 dilations";
    for (int b = 0; b < c.n_resblocks; ++b) {
        const int k = c.resblock_kernel_sizes[b];
        if (k < 1 || !(k & 1) || k > kFfgMaxTaps) return "resblock kernel sizes must be odd and <= 13";
        for (int p = 0; p < c.n_dilations; ++p) {
            const int d = c.resblock_dilation_sizes[b][p];
            if (d < 1) return "resblock dilations must be >= 1";
            if ((k / 2) * d > kFfgMaxHalo) return "resblock halo (kernel_size / 2) * dilation exceeds the 25 rows of the convolution kernel's LDS patch";
        }
    }
    for (int k : {c.pre_conv_kernel_size, c.post_conv_kernel_size})
        if (k < 1 || !(k & 1) || k > kFfgMaxTaps) return "pre / post conv kernel sizes must be odd and <= 13";
    return nullptr;
}

static void wn_expect(st_engine* e, const std::string& p, int64_t d0, int64_t d1, int64_t k, int64_t nbias) {
    expect(e, p + "bias", {nbias});
    expect(e, p + kWn0, {d0, 1, 1});
    expect(e, p + kWn1, {d0, d1, k});
}

static void ffgan_build_params(st_engine* e, const st_ffgan_config& c) {
    const int64_t M = c.input_channels;
    for (int i = 0; i < c.n_stages; ++i) {
        const int64_t C = c.dims[i];
        if (i == 0) {                                                                               // backbone.py:160-169
            expect(e, ds(0, 0) + "weight", {C, M, 7}); expect(e, ds(0, 0) + "bias", {C});
            expect(e, ds(0, 1) + "weight", {C}); expect(e, ds(0, 1) + "bias", {C});
        } else {                                                                                    // :173-176
            const int64_t Cp = c.dims[i - 1];
            expect(e, ds(i, 0) + "weight", {Cp}); expect(e, ds(i, 0) + "bias", {Cp});
            expect(e, ds(i, 1) + "weight", {C, Cp, 1}); expect(e, ds(i, 1) + "bias", {C});
        }
        for (int j = 0; j < c.depths[i]; ++j) {                                                     // :104-121
            const std::string p = blk(i, j);
            expect(e, p + "dwconv.weight", {C, 1, 7}); expect(e, p + "dwconv.bias", {C});
            expect(e, p + "norm.weight", {C}); expect(e, p + "norm.bias", {C});
            expect(e, p + "pwconv1.weight", {4 * C, C}); expect(e, p + "pwconv1.bias", {4 * C});
            expect(e, p + "pwconv2.weight", {C, 4 * C}); expect(e, p + "pwconv2.bias", {C});
            expect(e, p + "gamma", {C});
        }
    }
    const int64_t D = c.dims[c.n_stages - 1];
    expect(e, "backbone.norm.weight", {D}); expect(e, "backbone.norm.bias", {D});                 // :198
    const int64_t C0 = c.upsample_initial_channel;
    wn_expect(e, "head.conv_pre.", C0, D, c.pre_conv_kernel_size, C0);                             // head.py:158-166
    for (int i = 0; i < c.n_upsamples; ++i) {
        const int64_t ci = head_width(c, i), co = head_width(c, i + 1);
        wn_expect(e, "head.ups." + std::to_string(i) + ".", ci, co, c.upsample_kernel_sizes[i], co);      // :177-187: (in, out, k), g over dim 0
        for (int b = 0; b < c.n_resblocks; ++b)
            for (int p = 0; p < c.n_dilations; ++p)
                for (int which = 1; which <= 2; ++which) wn_expect(e, rb(i, b, which, p), co, co, c.resblock_kernel_sizes[b], co);      // :29-99
    }
    wn_expect(e, "head.conv_post.", 1, head_width(c, c.n_upsamples), c.post_conv_kernel_size, 1);  // :214-222
}

// st_finalize of an ffgan handle: 16-bit GEMM weights of the encoder, w = g v / ||v|| of the head's convs in fragment order
int FfganState::finalize(st_engine* e) {
    free_owned(e);
    FfganState* v = this;
    const st_ffgan_config& c = v->cfg;
    hipStream_t s = nullptr;
    const bool split = v->split;
    const int parts = v->parts();
    auto pack = [&](Conv& cv, const std::string& wname, const std::string& bname, int cout, int cin, int taps) -> int {
        cv.cout = cout; cv.cin = cin * taps * parts; cv.taps = 1; cv.split = false;      // consumed as a k = 1 GEMM (the stem over im2col rows)
        int rc = dev_alloc(e, &cv.w, (size_t)cout * cv.cin * 2); if (rc) return rc;
        if (split && taps == 1) {        // [W_hi | W_hi | W_lo (| W_lo)] against K = [a_hi | a_lo | a_hi (| a_lo)]
            for (int k = 0; k < parts; ++k)
                HIPCHK(e, launch_pack_weight(e->dt, P(e, wname), cout, cin, 1, 0, cin, cv.w, 0, parts * cin, k * cin, cin, k >= 2, s));
        } else if (split) {              // the stem: the same slices, each in the (tap, channel) order of the im2col rows
            HIPCHK(e, launch_ffg_pack_rows_split(e->dt, P(e, wname), cout, cin, taps, parts, cv.w, s));
        } else {
            HIPCHK(e, launch_pack_weight(e->dt, P(e, wname), cout, cin, taps, 0, cin, cv.w, 0, cin, 0, cin, 0, s));
        }
        cv.bias = const_cast<float*>(P(e, bname));
        return ST_OK;
    };
    int rc;
    v->down.assign(c.n_stages, Conv()); v->pw1.assign(c.n_stages, {}); v->pw2.assign(c.n_stages, {});
    for (int i = 0; i < c.n_stages; ++i) {
        const int C = c.dims[i];
        if (i == 0) { if ((rc = pack(v->stem, ds(0, 0) + "weight", ds(0, 0) + "bias", C, c.input_channels, 7))) return rc; }
        else if ((rc = pack(v->down[i], ds(i, 1) + "weight", ds(i, 1) + "bias", C, c.dims[i - 1], 1))) return rc;
        v->pw1[i].assign(c.depths[i], Conv()); v->pw2[i].assign(c.depths[i], Conv());
        for (int j = 0; j < c.depths[i]; ++j) {
            if ((rc = pack(v->pw1[i][j], blk(i, j) + "pwconv1.weight", blk(i, j) + "pwconv1.bias", 4 * C, C, 1))) return rc;
            if ((rc = pack(v->pw2[i][j], blk(i, j) + "pwconv2.weight", blk(i, j) + "pwconv2.bias", C, 4 * C, 1))) return rc;
        }
    }
    // weight norm: one scale per row of dim 0, then the fold inside the packing kernel
    auto wn_scale = [&](const std::string& p, int rows, int inner, float** scale) -> int {
        int rc2 = dev_alloc(e, (void**)scale, (size_t)rows * 4); if (rc2) return rc2;
        HIPCHK(e, launch_ffg_wn_scale(P(e, p + kWn1), P(e, p + kWn0), rows, inner, *scale, s));
        return ST_OK;
    };
    auto conv = [&](FfConv& cv, const std::string& p, int cout, int cin, int taps, int dil) -> int {
        float* scale = nullptr;
        int rc2 = wn_scale(p, cout, cin * taps, &scale); if (rc2) return rc2;
        cv.cin = cin; cv.cout = cout; cv.taps = taps; cv.dil = dil; cv.bias = P(e, p + "bias");
        if ((rc2 = dev_alloc(e, &cv.wfrag, ffg_frag_bytes(cout, cin, taps, split ? ffg_split_planes(e->dt) : 1)))) return rc2;
        HIPCHK(e, launch_ffg_pack_conv(e->dt, P(e, p + kWn1), scale, cout, cin, taps, 0, cv.wfrag, s, split));
        return ST_OK;
    };
    const int D = c.dims[c.n_stages - 1];
    if ((rc = conv(v->pre, "head.conv_pre.", c.upsample_initial_channel, D, c.pre_conv_kernel_size, 1))) return rc;
    v->ups.assign(c.n_upsamples, FfConv()); v->c1.assign(c.n_upsamples, {}); v->c2.assign(c.n_upsamples, {});
    for (int i = 0; i < c.n_upsamples; ++i) {
        const int ci = head_width(c, i), co = head_width(c, i + 1), u = c.upsample_rates[i];
        const std::string p = "head.ups." + std::to_string(i) + ".";
        FfConv& up = v->ups[i];
        float *scale = nullptr, *bias = nullptr;
        if ((rc = wn_scale(p, ci, co * 2 * u, &scale))) return rc;
        up.cin = ci; up.cout = u * co; up.taps = 3; up.dil = 1;
        if ((rc = dev_alloc(e, &up.wfrag, ffg_frag_bytes(up.cout, ci, 3, split ? ffg_split_planes(e->dt) : 1)))) return rc;
        HIPCHK(e, launch_ffg_pack_conv(e->dt, P(e, p + kWn1), scale, up.cout, ci, 3, u, up.wfrag, s, split));
        if ((rc = dev_alloc(e, (void**)&bias, (size_t)up.cout * 4))) return rc;
        HIPCHK(e, launch_ffg_tile_bias(P(e, p + "bias"), co, u, bias, s));
        up.bias = bias;
        v->c1[i].assign(c.n_resblocks, std::vector<FfConv>(c.n_dilations)); v->c2[i].assign(c.n_resblocks, std::vector<FfConv>(c.n_dilations));
        for (int b = 0; b < c.n_resblocks; ++b)
            for (int q = 0; q < c.n_dilations; ++q) {
                if ((rc = conv(v->c1[i][b][q], rb(i, b, 1, q), co, co, c.resblock_kernel_sizes[b], c.resblock_dilation_sizes[b][q]))) return rc;
                if ((rc = conv(v->c2[i][b][q], rb(i, b, 2, q), co, co, c.resblock_kernel_sizes[b], 1))) return rc;
            }
    }
    {
        const int cl = head_width(c, c.n_upsamples), k = c.post_conv_kernel_size;
        float* scale = nullptr;
        if ((rc = wn_scale("head.conv_post.", 1, cl * k, &scale))) return rc;
        if ((rc = dev_alloc(e, (void**)&v->post_w, (size_t)cl * k * 4))) return rc;
        HIPCHK(e, launch_ffg_pack_post(P(e, "head.conv_post." + kWn1), scale, cl, k, v->post_w, s));
    }
    HIPCHK(e, hipDeviceSynchronize());
    return ST_OK;
}

// widest level of one utterance, in channel-samples per mel frame: max over the levels of (product of the rates so far) * width
static int64_t ffgan_level_elems(const st_ffgan_config& c) {
    int64_t up = 1, widest = head_width(c, 0);
    for (int i = 0; i < c.n_upsamples; ++i) { up *= c.upsample_rates[i]; widest = std::max(widest, up * head_width(c, i + 1)); }
    return widest;
}
static int ffgan_max_dim(const st_ffgan_config& c) { return *std::max_element(c.dims, c.dims + c.n_stages); }
// rows per chunk: 32-bit operand offsets of the encoder's GEMMs (widest operand row: the im2col rows or 4 * dim)
static int64_t ffgan_max_rows(const st_ffgan_config& c) {
    const bool split = c.operand_dtype == ST_OPERAND_BF16_SPLIT || c.operand_dtype == ST_OPERAND_F16_SPLIT;      // a pair row is twice as wide
    const int64_t widest = std::max<int64_t>(7 * (int64_t)c.input_channels, 4 * (int64_t)ffgan_max_dim(c)) * (split ? 2 : 1);
    return (((int64_t)1 << 31) - 1) / (widest * 2);
}
constexpr int64_t kFfganHeadBytes = (int64_t)1 << 30;      // bound of the head's level tensors per chunk (stabletts_hip.h: st_ffgan_forward)
// bytes of head workspace per channel-sample of the widest level: three fp32 level tensors and c1's output, 16-bit or (split) fp32
static int64_t ffgan_head_sample_bytes(const FfganState* v) { return v->split ? 16 : 14; }
constexpr int kFfganMaxT = 1 << 20;

// One chunk of whole utterances: the encoder's GEMMs and LayerNorms run over its R flattened rows, R = B * T, or the packed rows of a
// ragged chunk (rg: mel and audio stay padded to T; the im2col, the depthwise conv, the head's convolutions and the post kernel know
// utterances and take their ragged form -- every level tensor of the head then holds R * up packed rows).
static int ffgan_forward_chunk(st_engine* e, const float* mel, float* audio, int B, int T, const RaggedChunk* rg, hipStream_t s) {
    FfganState* v = state_of<FfganState>(e);
    const st_ffgan_config& c = v->cfg;
    const int M = c.input_channels, Dmax = ffgan_max_dim(c), D = c.dims[c.n_stages - 1], C0 = c.upsample_initial_channel;
    const int64_t R = rg ? rg->rows : (int64_t)B * T, lvl = ffgan_level_elems(c) * R;
    const bool cap = e->capture, split = v->split;

    size_t off = 0;
    auto want = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t pr = split ? 2 : 1;       // split: a16, h16 and u16 are pair tensors [row][hi | lo]
    const size_t o_a16 = want((size_t)R * 7 * M * 2 * pr), o_xa = want((size_t)R * Dmax * 4), o_xb = want((size_t)R * Dmax * 4), o_h16 = want((size_t)R * Dmax * 2 * pr);
    const size_t o_u16 = want((size_t)R * 4 * Dmax * 2 * pr), o_enc32 = want((size_t)R * D * 4), o_enc16 = split ? 0 : want((size_t)R * D * 2), o_pre = want((size_t)R * C0 * 4);
    const size_t o_X = want((size_t)lvl * 4), o_Y = want((size_t)lvl * 4), o_Mn = want((size_t)lvl * 4), o_U = want((size_t)lvl * (split ? 4 : 2));
    const size_t o_u32 = split ? want((size_t)R * 4 * Dmax * 4) : 0;      // split: pwconv1's fp32 output (and no enc16: conv_pre reads enc32)
    const size_t o_pt = cap ? want((size_t)R * v->hop * 4) : 0;
    const size_t o_tiles = rg ? want((size_t)rg->n_tiles * sizeof(VocSeg)) : 0, o_frames = rg ? want((size_t)rg->n_groups * sizeof(VocSeg)) : 0;
    int rc = ensure_ws(e, off); if (rc) return rc;
    VocSeg* tiles = (VocSeg*)(e->ws + o_tiles); VocSeg* frames = (VocSeg*)(e->ws + o_frames);      // im2col tiles; one entry per packed row
    void* a16 = e->ws + o_a16; float* x = (float*)(e->ws + o_xa); float* xn = (float*)(e->ws + o_xb); void* h16 = e->ws + o_h16; void* u16 = e->ws + o_u16;
    float* enc32 = (float*)(e->ws + o_enc32); void* enc16 = split ? nullptr : e->ws + o_enc16; float* pre32 = (float*)(e->ws + o_pre);
    float* X = (float*)(e->ws + o_X); float* Y = (float*)(e->ws + o_Y); float* Mn = (float*)(e->ws + o_Mn); void* U = e->ws + o_U;
    float* pretanh = cap ? (float*)(e->ws + o_pt) : nullptr;
    float* u32 = (float*)(e->ws + o_u32);
    // a split GEMM over the pair tensor `pair` of K values per half: c0 = both halves, c2 = the re-read (hi, or hi and lo)
    const int parts = v->parts();
    auto pair_src = [&](ConvGemmArgs& a, const void* pair, int K) { a.a0 = pair; a.c0 = 2 * K; a.c2 = (parts - 2) * K; };

    auto args = [&](const Conv& cv) { return flat_gemm_args(e, cv, R); };
    // ---- ConvNeXtEncoder.forward (backbone.py:206-214)
    for (int i = 0; i < c.n_stages; ++i) {
        const int C = c.dims[i];
        if (i == 0) {       // stem: k = 7 conv as an im2col GEMM, then the per-frame LayerNorm
            if (rg) HIPCHK(e, launch_voc_segments(rg->utt, B, 1, tiles, frames, s));
            if (split)   HIPCHK(e, launch_ffg_im2col7_split(e->dt, mel, B, M, T, rg ? tiles : nullptr, rg ? rg->n_tiles : 0, a16, s));
            else if (rg) HIPCHK(e, launch_voc_im2col7_ragged(e->dt, mel, tiles, rg->n_tiles, M, T, a16, s));
            else         HIPCHK(e, launch_voc_im2col7(e->dt, mel, B, M, T, a16, s));
            ConvGemmArgs a = args(v->stem); a.a0 = a16; a.c0 = 7 * M; a.out32 = x;
            if (split) pair_src(a, a16, 7 * M);
            HIPCHK(e, gemm(e, 1, EPI_F32, a, s));
            HIPCHK(e, launch_ffg_ln(e->dt, x, P(e, ds(0, 1) + "weight"), P(e, ds(0, 1) + "bias"), R, C, x, nullptr, s));
        } else {            // LayerNorm, then the k = 1 conv to the next width
            const int Cp = c.dims[i - 1];
            if (split) HIPCHK(e, launch_ffg_ln_split(e->dt, x, P(e, ds(i, 0) + "weight"), P(e, ds(i, 0) + "bias"), R, Cp, nullptr, h16, s));
            else       HIPCHK(e, launch_ffg_ln(e->dt, x, P(e, ds(i, 0) + "weight"), P(e, ds(i, 0) + "bias"), R, Cp, nullptr, h16, s));
            ConvGemmArgs a = args(v->down[i]); a.a0 = h16; a.c0 = Cp; a.out32 = xn;
            if (split) pair_src(a, h16, Cp);
            HIPCHK(e, gemm(e, 1, EPI_F32, a, s));
            std::swap(x, xn);
        }
        for (int j = 0; j < c.depths[i]; ++j) {      // ConvNeXtBlock.forward (backbone.py:124-143); DropPath is the identity in eval
            const std::string p = blk(i, j);
            const float *dw = P(e, p + "dwconv.weight"), *db = P(e, p + "dwconv.bias"), *nw = P(e, p + "norm.weight"), *nb = P(e, p + "norm.bias");
            if (split)   HIPCHK(e, launch_ffg_dwconv_ln_split(e->dt, x, dw, db, nw, nb, B, T, rg ? frames : nullptr, R, C, h16, s));
            else if (rg) HIPCHK(e, launch_ffg_dwconv_ln_ragged(e->dt, x, dw, db, nw, nb, frames, R, C, h16, s));
            else         HIPCHK(e, launch_ffg_dwconv_ln(e->dt, x, dw, db, nw, nb, B, T, C, h16, s));
            if (split) {     // pwconv1 to fp32, the GELU pair, then x += gamma * (W u + b) over the pair of u
                ConvGemmArgs a = args(v->pw1[i][j]); pair_src(a, h16, C); a.out32 = u32;
                HIPCHK(e, gemm(e, 1, EPI_F32, a, s));
                HIPCHK(e, launch_ffg_gelu_split(e->dt, u32, R, 4 * C, u16, s));
                ConvGemmArgs b2 = args(v->pw2[i][j]); pair_src(b2, u16, 4 * C); b2.out32 = x;
                b2.gate = P(e, p + "gamma"); b2.gate_stride = 0;
                HIPCHK(e, gemm(e, 1, EPI_RESGATE, b2, s));
                continue;
            }
            {
                ConvGemmArgs a = args(v->pw1[i][j]); a.a0 = h16; a.c0 = C; a.out16 = u16;
                HIPCHK(e, gemm(e, 1, EPI_GELU16, a, s));
            }
            {       // x += gamma * (W u + b)
                ConvGemmArgs a = args(v->pw2[i][j]); a.a0 = u16; a.c0 = 4 * C; a.out32 = x; a.gate = P(e, p + "gamma"); a.gate_stride = 0;
                HIPCHK(e, gemm(e, 1, EPI_RESGATE, a, s));
            }
        }
    }
    // (split: conv_pre stages enc32 itself and splits it there, so no 16-bit copy is written)
    HIPCHK(e, launch_ffg_ln(e->dt, x, P(e, "backbone.norm.weight"), P(e, "backbone.norm.bias"), R, D, enc32, enc16, s));
    if (cap) capture(e, "ffgan.encoder", enc32, R * D, false, s);

    // ---- HiFiGANGenerator.forward (head.py:226-249)
    // L: the level length of the chunk's longest utterance (ragged: it sizes the grid; up = L / its frames scales the utterance table)
    const int Tmax = rg ? rg->t_max : T;
    auto run = [&](const FfConv& cv, int L, FfgConvArgs a) -> hipError_t {
        a.wfrag = cv.wfrag; a.bias = cv.bias; a.cin = cv.cin; a.cout = cv.cout; a.taps = cv.taps; a.dil = cv.dil; a.L = L; a.n_items = B;
        if (rg) { a.utt = rg->utt; a.up = L / Tmax; }
        return split ? launch_ffg_conv_split(e->dt, a, s) : launch_ffg_conv(e->dt, a, s);
    };
    {
        FfgConvArgs a{}; a.epi = FFG_F32; a.out32 = pre32;
        if (split) { a.in32 = enc32; a.in_raw = 1; } else a.in16 = enc16;
        HIPCHK(e, run(v->pre, Tmax, a));
    }
    const float* cur = pre32;
    int L = Tmax;
    const int nb = c.n_resblocks, np = c.n_dilations;
    for (int i = 0; i < c.n_upsamples; ++i) {
        {       // silu + ConvTranspose1d: [L][u * C] rows = the upsampled [L * u][C]
            FfgConvArgs a{}; a.in32 = cur; a.epi = FFG_F32; a.out32 = X;
            HIPCHK(e, run(v->ups[i], L, a));
        }
        L *= c.upsample_rates[i];
        for (int b = 0; b < nb; ++b)             // ParralelBlock (head.py:132-133): every ResBlock1 starts from X
            for (int p = 0; p < np; ++p) {       // ResBlock1.forward (head.py:101-108)
                const float* xin = p == 0 ? X : Y;
                {
                    FfgConvArgs a{}; a.in32 = xin;
                    if (split) { a.epi = FFG_F32; a.out32 = (float*)U; } else { a.epi = FFG_SILU16; a.out16 = U; }
                    HIPCHK(e, run(v->c1[i][b][p], L, a));
                }
                FfgConvArgs a{}; a.epi = FFG_RES; a.res32 = xin;
                if (split) a.in32 = (const float*)U; else a.in16 = U;
                if (p + 1 < np) a.out32 = Y;
                else { a.mean = Mn; a.mean_first = b == 0; a.mean_scale = b + 1 == nb ? 1.0f / (float)nb : 1.0f; }
                HIPCHK(e, run(v->c2[i][b][p], L, a));
            }
        cur = Mn;
    }
    const int Cl = head_width(c, c.n_upsamples), kpost = c.post_conv_kernel_size;
    if (rg) HIPCHK(e, launch_ffg_post_ragged(cur, v->post_w, P(e, "head.conv_post.bias"), rg->utt, v->hop, B, T * v->hop, Cl, kpost, pretanh, audio, s));
    else    HIPCHK(e, launch_ffg_post(cur, v->post_w, P(e, "head.conv_post.bias"), B, L, Cl, kpost, pretanh, audio, s));
    if (cap) capture(e, "ffgan.pre_tanh", pretanh, R * v->hop, false, s);
    return ST_OK;
}

// Chunks keep the packed rows within max_rows, the head's level tensors of those rows within kFfganHeadBytes (one utterance
// always runs) and the grid within 65535 items; dense and ragged batches alike
static VocoderGeom ffgan_geom(st_engine* e) {
    FfganState* v = state_of<FfganState>(e);
    const int64_t head_rows = std::max<int64_t>(1, kFfganHeadBytes / (ffgan_level_elems(v->cfg) * ffgan_head_sample_bytes(v)));
    const ChunkLimits lim = {ffgan_max_rows(v->cfg), 65535, 0, head_rows};
    return {lim, lim, v->cfg.input_channels, v->hop, &v->slots};
}
static int ffgan_dw_frames(int64_t) { return 1; }      // one depthwise group per packed row
static const VocoderKind kFfganKind = {KIND_FFGAN, "the vocoder's row indexing", kFfganMaxT, ffgan_geom, ffgan_dw_frames, ffgan_forward_chunk};

}  // namespace sthost

extern "C" {

int st_create_ffgan(const st_ffgan_config* cfg, int device, st_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ST_ERR_INVALID; }
    if (const char* why = ffgan_unsupported(*cfg)) { g_create_error = why; return ST_ERR_INVALID; }
    auto state = std::make_unique<FfganState>();
    state->cfg = *cfg;
    state->split = cfg->operand_dtype == ST_OPERAND_BF16_SPLIT || cfg->operand_dtype == ST_OPERAND_F16_SPLIT;
    for (int i = 0; i < cfg->n_upsamples; ++i) state->hop *= cfg->upsample_rates[i];
    st_engine* e = nullptr;
    if (int rc = new_handle(KIND_FFGAN, device, std::move(state), &e)) return rc;
    e->dt = (cfg->operand_dtype == ST_OPERAND_BF16 || cfg->operand_dtype == ST_OPERAND_BF16_SPLIT) ? DT_BF16 : DT_F16;
    e->tile.splitk_target = 0;      // no split-K convs: the encoder's GEMMs run over the flattened rows of the whole batch
    ffgan_build_params(e, *cfg);
    if (hipMalloc(&e->zeros, 256) != hipSuccess || hipMemset(e->zeros, 0, 256) != hipSuccess) {
        delete e;
        g_create_error = "hipMalloc failed";
        return ST_ERR_HIP;
    }
    *out = e;
    return ST_OK;
}

int st_ffgan_forward(st_engine* e, const float* mel, float* audio, int B, int T, void* stream) {
    return vocoder_forward(kFfganKind, e, mel, audio, B, T, stream);
}

int st_ffgan_forward_ragged(st_engine* e, const float* mel, const int64_t* lengths, float* audio, int B, int T, void* stream) {
    return vocoder_forward_ragged(kFfganKind, e, mel, lengths, audio, B, T, stream);
}

}  // extern "C"
