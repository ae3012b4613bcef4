// Feature front end behind the C ABI (st_create_mel_extractor / st_mel_forward / st_mel_forward_ragged / st_mel_backward):
// handle kind KIND_MEL_EXTRACTOR.
// Reference: utils/audio.py:6-52 (LinearSpectrogram, LogMelSpectrogram), config.py:4-19.  The window and the filter bank
// are the module's buffers ("spectrogram.window", "mel_scale.fb"), loaded like parameters; st_finalize derives each
// filter's nonzero bin range from the loaded fb and packs those weights, and the same table bin-major for the backward.  The
// kernels are in audio_kernels.hip.
#include "engine_internal.h"
#include "audio_launch.h"

#include <string>
#include <vector>

using namespace st;
using namespace sthost;

namespace sthost {

struct MelState : KindState {
    MelState() : KindState("st_repack: mel-extractor handles re-read their filter bank through st_finalize") {}
    ~MelState() override;
    int finalize(st_engine* e) override;
    st_mel_config cfg{};
    int* band = nullptr;          // [n_mels][3]: lo, hi, offset into wband
    float* wband = nullptr;
    int* bandT = nullptr;         // [n_fft / 2 + 1][3]: mlo, mhi, offset into wbandT (the backward's dmag = fb dmel)
    float* wbandT = nullptr;
    // ragged launches: utterance tables in pinned host memory, copied to device slots; a slot is refilled only after the
    // event of its previous launch, so a call never waits for the one before it
    static constexpr int kSlots = 4;
    MelUtt* host[kSlots] = {};
    MelUtt* dev[kSlots] = {};
    hipEvent_t ev[kSlots] = {};
    bool used[kSlots] = {};
    int cap = 0, next = 0;
};

MelState::~MelState() {
    for (int i = 0; i < kSlots; ++i) {
        if (host[i]) hipHostFree(host[i]);
        if (dev[i]) hipFree(dev[i]);
        if (ev[i]) hipEventDestroy(ev[i]);
    }
    if (band) hipFree(band);
    if (wband) hipFree(wband);
    if (bandT) hipFree(bandT);
    if (wbandT) hipFree(wbandT);
}

// st_finalize of a mel handle: every filter's nonzero range [lo, hi) of bins, and its weights packed in bin order.  A filter
// without a nonzero weight gets an empty range (its sum is 0, log(1e-5) after the clamp), as in the dense product.  The
// transposed table gives every bin its range of mels with nonzero weights and those weights in mel order; a bin that no filter
// reaches gets an empty range (dmag = 0), and an all-zero filter appears in no bin's range.
int MelState::finalize(st_engine* e) {
    MelState* m = this;
    const st_mel_config& c = m->cfg;
    if (c.n_mels > 0) {
        const int bins = c.n_fft / 2 + 1, M = c.n_mels;
        std::vector<float> fb((size_t)bins * M);
        HIPCHK(e, hipMemcpy(fb.data(), P(e, "mel_scale.fb"), fb.size() * 4, hipMemcpyDeviceToHost));
        std::vector<int> band((size_t)3 * M);
        std::vector<float> w;
        for (int j = 0; j < M; ++j) {
            int lo = bins, hi = 0;
            for (int k = 0; k < bins; ++k)
                if (fb[(size_t)k * M + j] != 0.0f) { if (k < lo) lo = k; hi = k + 1; }
            if (hi == 0) lo = 0;
            band[3 * j] = lo; band[3 * j + 1] = hi; band[3 * j + 2] = (int)w.size();
            for (int k = lo; k < hi; ++k) w.push_back(fb[(size_t)k * M + j]);     // (zeros inside the range kept: same terms)
        }
        if (w.empty()) w.push_back(0.0f);
        std::vector<int> bandT((size_t)3 * bins);
        std::vector<float> wT;
        for (int k = 0; k < bins; ++k) {
            int lo = M, hi = 0;
            for (int j = 0; j < M; ++j)
                if (fb[(size_t)k * M + j] != 0.0f) { if (j < lo) lo = j; hi = j + 1; }
            if (hi == 0) lo = 0;
            bandT[3 * k] = lo; bandT[3 * k + 1] = hi; bandT[3 * k + 2] = (int)wT.size();
            for (int j = lo; j < hi; ++j) wT.push_back(fb[(size_t)k * M + j]);
        }
        if (wT.empty()) wT.push_back(0.0f);
        if (m->band) { hipFree(m->band); m->band = nullptr; }
        if (m->wband) { hipFree(m->wband); m->wband = nullptr; }
        if (m->bandT) { hipFree(m->bandT); m->bandT = nullptr; }
        if (m->wbandT) { hipFree(m->wbandT); m->wbandT = nullptr; }
        HIPCHK(e, hipMalloc((void**)&m->band, band.size() * 4));
        HIPCHK(e, hipMalloc((void**)&m->wband, w.size() * 4));
        HIPCHK(e, hipMalloc((void**)&m->bandT, bandT.size() * 4));
        HIPCHK(e, hipMalloc((void**)&m->wbandT, wT.size() * 4));
        HIPCHK(e, hipMemcpy(m->band, band.data(), band.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(m->wband, w.data(), w.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(m->bandT, bandT.data(), bandT.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(e, hipMemcpy(m->wbandT, wT.data(), wT.size() * 4, hipMemcpyHostToDevice));
    }
    return ST_OK;
}

static int64_t frames_of(const st_mel_config& c, int64_t L) {
    if (L <= c.pad || L + 2 * (int64_t)c.pad < c.n_fft) return ST_ERR_INVALID;
    return 1 + (L + 2 * (int64_t)c.pad - c.n_fft) / c.hop_length;
}

static int mel_check(st_engine* e, const float* wave, float* out) {
    int rc = check_handle(e, KIND_MEL_EXTRACTOR); if (rc) return rc;
    if (!e->finalized) return e->fail(ST_ERR_STATE, "st_finalize() has not been called after loading the window / filter bank");
    if (!wave || !out) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    return ST_OK;
}

static MelArgs mel_args(st_engine* e, const float* wave, float* out, bool log_mel) {
    const MelState* m = state_of<MelState>(e);
    const st_mel_config& c = m->cfg;
    MelArgs a{};
    a.wave = wave; a.window = P(e, "spectrogram.window"); a.wband = m->wband; a.band = m->band; a.out = out;
    a.n_fft = c.n_fft; a.hop = c.hop_length; a.pad = c.pad;
    a.rows = log_mel ? c.n_mels : c.n_fft / 2 + 1; a.log_mel = log_mel ? 1 : 0;
    return a;
}

}  // namespace sthost

extern "C" {

int st_create_mel_extractor(const st_mel_config* cfg, int device, st_engine** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return ST_ERR_INVALID; }
    auto bad = [&](const char* m, int code) { g_create_error = m; return code; };
    if (cfg->n_fft < 1 || cfg->win_length < 1 || cfg->hop_length < 1) return bad("n_fft, win_length and hop_length must be positive", ST_ERR_INVALID);
    if (cfg->pad < 0 || cfg->n_mels < 0) return bad("pad and n_mels must not be negative", ST_ERR_INVALID);
    if (cfg->hop_length > cfg->n_fft) return bad("hop_length must not exceed n_fft", ST_ERR_INVALID);
    if (cfg->win_length > cfg->n_fft) return bad("win_length must not exceed n_fft (torch.stft)", ST_ERR_INVALID);
    if (cfg->pad_mode < ST_PAD_REFLECT || cfg->pad_mode > ST_PAD_CIRCULAR) return bad("pad_mode must be an ST_PAD_* value", ST_ERR_INVALID);
    // limits of this native build
    if (cfg->center != 0) return bad("native kernels are built for center=False", ST_ERR_UNSUPPORTED);
    if (cfg->pad_mode != ST_PAD_REFLECT) return bad("native kernels are built for pad_mode 'reflect'", ST_ERR_UNSUPPORTED);
    if (cfg->win_length != cfg->n_fft) return bad("native kernels are built for win_length == n_fft", ST_ERR_UNSUPPORTED);
    if (cfg->n_fft < kMelMinNfft || cfg->n_fft > kMelMaxNfft || (cfg->n_fft & (cfg->n_fft - 1)))
        return bad("native kernels are built for n_fft a power of two in [32, 2048]", ST_ERR_UNSUPPORTED);
    auto state = std::make_unique<MelState>();
    state->cfg = *cfg;
    st_engine* e = nullptr;
    if (int rc = new_handle(KIND_MEL_EXTRACTOR, device, std::move(state), &e)) return rc;
    expect(e, "spectrogram.window", {cfg->win_length});                                        // utils/audio.py:17
    if (cfg->n_mels > 0) expect(e, "mel_scale.fb", {cfg->n_fft / 2 + 1, cfg->n_mels});         // :45 (MelScale's buffer)
    *out = e;
    return ST_OK;
}

int64_t st_mel_frames(const st_engine* e, int64_t L) {
    const MelState* m = state_if<MelState>(e, KIND_MEL_EXTRACTOR);
    return m ? frames_of(m->cfg, L) : ST_ERR_INVALID;
}

int st_mel_forward(st_engine* e, const float* wave, int B, int64_t L, float* out, void* stream) {
    int rc = mel_check(e, wave, out); if (rc) return rc;
    const st_mel_config& c = state_of<MelState>(e)->cfg;
    if (c.n_mels < 1) return e->fail(ST_ERR_STATE, "a linear-spectrogram extractor (n_mels = 0) has no mel output: st_mel_forward_ragged with ST_MEL_LINEAR");
    if (B < 1) return e->fail(ST_ERR_INVALID, "B must be >= 1");
    const int64_t T = frames_of(c, L);
    if (T < 0) return e->fail(ST_ERR_INVALID, "L must exceed pad (reflect padding) and L + 2 pad must be >= n_fft");
    const int FR = mel_tile_frames(c.n_fft);
    const int64_t per = (T + FR - 1) / FR;
    if (L >= ((int64_t)1 << 31) || (int64_t)B * per >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "batch too large");
    HIPCHK(e, hipSetDevice(e->device));
    MelArgs a = mel_args(e, wave, out, true);
    a.utt = nullptr; a.B = B; a.L = L; a.frames = (int)T; a.tiles_per = (int)per; a.total_tiles = (int)(B * per);
    HIPCHK(e, launch_mel(a, (hipStream_t)stream));
    return ST_OK;
}

int st_mel_forward_ragged(st_engine* e, const float* wave, const int64_t* sample_offsets, const int64_t* frame_offsets, int B,
                          int output, float* out, void* stream) {
    int rc = mel_check(e, wave, out); if (rc) return rc;
    if (!sample_offsets || !frame_offsets) return e->fail(ST_ERR_INVALID, "null offsets");
    if (B < 1) return e->fail(ST_ERR_INVALID, "B must be >= 1");
    if (output != ST_MEL_LOG && output != ST_MEL_LINEAR) return e->fail(ST_ERR_INVALID, "output must be ST_MEL_LOG or ST_MEL_LINEAR");
    MelState* m = state_of<MelState>(e);
    const st_mel_config& c = m->cfg;
    if (output == ST_MEL_LOG && c.n_mels < 1) return e->fail(ST_ERR_STATE, "a linear-spectrogram extractor (n_mels = 0) has no mel output");
    const int FR = mel_tile_frames(c.n_fft);
    // validate everything before touching the device
    int64_t tiles = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t L = sample_offsets[b + 1] - sample_offsets[b], T = frames_of(c, L);
        if (sample_offsets[b] < 0 || frame_offsets[b] < 0) return e->fail(ST_ERR_INVALID, "negative offset");
        if (T < 0) return e->fail(ST_ERR_INVALID, "utterance " + std::to_string(b) + ": L must exceed pad and L + 2 pad must be >= n_fft");
        if (L >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "utterance " + std::to_string(b) + " too long");
        if (frame_offsets[b + 1] - frame_offsets[b] != T)
            return e->fail(ST_ERR_INVALID, "frame_offsets[" + std::to_string(b + 1) + "] - frame_offsets[" + std::to_string(b) +
                           "] must be st_mel_frames(L) = " + std::to_string(T));
        tiles += (T + FR - 1) / FR;
    }
    if (tiles >= ((int64_t)1 << 31)) return e->fail(ST_ERR_INVALID, "batch too large");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t s = (hipStream_t)stream;
    if (B + 1 > m->cap) {       // grow every slot (after their launches)
        for (int i = 0; i < MelState::kSlots; ++i) {
            if (m->used[i]) HIPCHK(e, hipEventSynchronize(m->ev[i]));
            if (m->host[i]) { hipHostFree(m->host[i]); m->host[i] = nullptr; }
            if (m->dev[i]) { hipFree(m->dev[i]); m->dev[i] = nullptr; }
        }
        const int cap = B + 1 > 64 ? B + 1 : 64;
        for (int i = 0; i < MelState::kSlots; ++i) {
            HIPCHK(e, hipHostMalloc((void**)&m->host[i], (size_t)cap * sizeof(MelUtt)));
            HIPCHK(e, hipMalloc((void**)&m->dev[i], (size_t)cap * sizeof(MelUtt)));
            if (!m->ev[i]) HIPCHK(e, hipEventCreateWithFlags(&m->ev[i], hipEventDisableTiming));
            m->used[i] = false;
        }
        m->cap = cap;
    }
    const int slot = m->next;
    m->next = (m->next + 1) % MelState::kSlots;
    if (m->used[slot]) HIPCHK(e, hipEventSynchronize(m->ev[slot]));
    MelUtt* u = m->host[slot];
    int tile0 = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t L = sample_offsets[b + 1] - sample_offsets[b], T = frame_offsets[b + 1] - frame_offsets[b];
        u[b].s_off = sample_offsets[b]; u[b].f_off = frame_offsets[b]; u[b].L = (int)L; u[b].frames = (int)T; u[b].tile0 = tile0; u[b].pad_ = 0;
        tile0 += (int)((T + FR - 1) / FR);
    }
    u[B] = MelUtt{0, 0, 0, 0, tile0, 0};
    HIPCHK(e, hipMemcpyAsync(m->dev[slot], u, (size_t)(B + 1) * sizeof(MelUtt), hipMemcpyHostToDevice, s));
    MelArgs a = mel_args(e, wave, out, output == ST_MEL_LOG);
    a.utt = m->dev[slot]; a.B = B; a.total_tiles = tile0;
    HIPCHK(e, launch_mel(a, s));
    HIPCHK(e, hipEventRecord(m->ev[slot], s));
    m->used[slot] = true;
    return ST_OK;
}

int64_t st_mel_backward_workspace_bytes(const st_engine* e, int B, int64_t L) {
    const MelState* m = state_if<MelState>(e, KIND_MEL_EXTRACTOR);
    if (!m || B < 1) return ST_ERR_INVALID;
    const st_mel_config& c = m->cfg;
    const int64_t T = frames_of(c, L);
    if (T < 0) return ST_ERR_INVALID;
    return (int64_t)B * T * c.n_fft * (int64_t)sizeof(float);
}

int st_mel_backward(st_engine* e, const float* wave, const float* grad_out, int B, int64_t L, int output, float* grad_wave,
                    void* workspace, void* stream) {
    int rc = mel_check(e, wave, grad_wave); if (rc) return rc;
    if (!grad_out || !workspace) return e->fail(ST_ERR_INVALID, "null tensor pointer");
    if (output != ST_MEL_LOG && output != ST_MEL_LINEAR) return e->fail(ST_ERR_INVALID, "output must be ST_MEL_LOG or ST_MEL_LINEAR");
    MelState* m = state_of<MelState>(e);
    const st_mel_config& c = m->cfg;
    if (output == ST_MEL_LOG && c.n_mels < 1) return e->fail(ST_ERR_STATE, "a linear-spectrogram extractor (n_mels = 0) has no mel output");
    if (output == ST_MEL_LOG && c.n_mels > 2 * c.n_fft)
        return e->fail(ST_ERR_UNSUPPORTED, "the native backward is built for n_mels <= 2 n_fft");
    if (B < 1) return e->fail(ST_ERR_INVALID, "B must be >= 1");
    const int64_t T = frames_of(c, L);
    if (T < 0) return e->fail(ST_ERR_INVALID, "L must exceed pad (reflect padding) and L + 2 pad must be >= n_fft");
    const int FR = mel_tile_frames(c.n_fft);
    const int64_t per = (T + FR - 1) / FR;
    if (L >= ((int64_t)1 << 31) || (int64_t)B * per >= ((int64_t)1 << 31) || (int64_t)B * L >= ((int64_t)1 << 39))
        return e->fail(ST_ERR_INVALID, "batch too large");
    HIPCHK(e, hipSetDevice(e->device));
    MelBwdArgs a{};
    a.wave = wave; a.window = P(e, "spectrogram.window"); a.grad = grad_out;
    a.wband = m->wband; a.band = m->band; a.wbandT = m->wbandT; a.bandT = m->bandT;
    a.ws = (float*)workspace; a.out = grad_wave;
    a.n_fft = c.n_fft; a.hop = c.hop_length; a.pad = c.pad;
    a.rows = output == ST_MEL_LOG ? c.n_mels : c.n_fft / 2 + 1; a.log_mel = output == ST_MEL_LOG ? 1 : 0;
    a.B = B; a.L = L; a.frames = (int)T; a.tiles_per = (int)per; a.total_tiles = (int)(B * per);
    HIPCHK(e, launch_mel_backward(a, (hipStream_t)stream));
    return ST_OK;
}

}  // extern "C"
