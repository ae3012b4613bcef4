// Host-side internals shared by every engine_*.cpp: the handle (st_engine), the per-kind state it owns (KindState), the parameter
// table, the workspace arena, gemm() and the entry checks.  What only the DiT kinds use is in engine_dit.h.  Not part of the C ABI.
#pragma once
#include "../../include/stabletts_hip.h"
#include "launch.h"

#include <map>
#include <memory>
#include <string>
#include <vector>

namespace sthost {

enum ProfClass {
    PC_PREP = 0, PC_PRENET, PC_INPROJ, PC_FILM_LN1, PC_QKV, PC_ATTN, PC_OPROJ, PC_LN2, PC_FFN1, PC_FFN2,
    PC_LSC, PC_FINAL, PC_ODE, PC_TRAIN_FWD, PC_TRAIN_BWD, PC_COUNT
};

struct Param {
    std::vector<int64_t> shape;
    float* dev = nullptr;
    bool loaded = false;
    bool borrowed = false;     // st_bind_param: dev is the caller's tensor, never freed here
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct Conv {            // packed 16-bit weights [cout][taps][cin] + fp32 bias
    void* w = nullptr;
    float* bias = nullptr;
    int cout = 0, cin = 0, taps = 0;
    bool split = false;  // cin = 3 x the reference's: [W_hi | W_hi | W_lo] for a split-precision operand [x_hi | x_lo | x_hi]
};

struct Captured { void* dev = nullptr; int64_t n = 0; bool is16 = false; };

struct ProfEvent { int cls; hipEvent_t a, b; double flops; };

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Float offsets into one device buffer, handed out in order, each on a 64-float (256-byte) boundary; off: the floats used so far
struct FloatArena {
    size_t off = 0;
    size_t want(size_t n) { const size_t o = off; off += (n + 63) / 64 * 64; return o; }
};

// What a handle is (st_engine::kind), in the order the creators were added.  kKinds names each for the message of an entry
// point that is handed another kind's handle (check_handle).
enum Kind { KIND_DECODER = 0, KIND_TEXT_ENCODER, KIND_VOCODER, KIND_STYLE_ENCODER, KIND_DURATION_PREDICTOR, KIND_MEL_EXTRACTOR, KIND_PERIOD_DISC, KIND_RESOLUTION_DISC,
            KIND_FFGAN, KIND_COUNT };
struct KindName { const char* what; const char* creator; };
constexpr KindName kKinds[KIND_COUNT] = {
    {"CFM decoder", "st_create"},                                     // the estimator of the CFM decoder
    {"text encoder", "st_create_text_encoder"},                       // TextEncoder: the decoder's DiT block kernels
    {"vocoder", "st_create_vocoder"},                                 // Vocos
    {"style encoder", "st_create_style_encoder"},                     // MelStyleEncoder
    {"duration predictor", "st_create_duration_predictor"},           // DurationPredictor
    {"mel extractor", "st_create_mel_extractor"},                     // the feature front end (utils/audio.py)
    {"period discriminator", "st_create_period_discriminator"},       // DiscriminatorP of the Vocos training step
    {"resolution discriminator", "st_create_resolution_discriminator"},      // DiscriminatorR of the Vocos training step
    {"FireflyGAN vocoder", "st_create_ffgan"},                        // FireflyGANBase (vocoders/ffgan)
};
// The activations of ONE grad-enabled forward (serial, B, T; inputs copied in) and the backward's scratch, in two device buffers
// that grow on demand and are then reused: what the style encoder, the duration predictor, the Vocos generator and both
// discriminators hold between a training forward and its backward.
struct SdTrain {
    char* act = nullptr; size_t act_cap = 0;
    char* scr = nullptr; size_t scr_cap = 0;
    int64_t serial = 0;            // counts the training forwards of this handle
    bool have = false;             // the activations of forward #serial are held
    int B = 0, T = 0;
    float p = 0.0f; unsigned long long seed = 0;
    bool masked = false;           // style encoder: the forward had a mask
};
int sd_train_grow(st_engine* e, char** buf, size_t* cap, size_t bytes);     // engine_style.cpp
// The protocol around a training forward / backward of those kinds.  `entry`: "st_<kind>_train", the common stem of the two entry
// points' names; `t_name`: what they call the length ("T" / "Tx").
void sd_train_commit(SdTrain* st, int B, int T, float p_dropout, unsigned long long seed, bool masked);      // forward #serial + 1 is held
// The backward of the held forward?  serial < 0: an entry point without serials, which compares B and T alone.
int sd_train_check(st_engine* e, const SdTrain& st, const char* entry, const char* t_name, int64_t serial, int B, int T);

// What a handle of one kind holds beyond the parameter table and the arena: exactly one per st_engine, installed by new_handle.
// The destructor frees every device allocation of the kind (the device is current and idle: st_destroy, or a creator's error path).
struct KindState {
    const char* const repack_refusal;      // st_repack's message for a kind that has nothing to re-pack on a stream
    explicit KindState(const char* refusal = nullptr) : repack_refusal(refusal) {}
    virtual ~KindState() {}
    virtual int finalize(st_engine* e) = 0;                       // st_finalize: every parameter is loaded, the device is idle
    virtual int repack(st_engine* e, hipStream_t s);              // st_repack; the base refuses with repack_refusal
    virtual int64_t device_bytes() const { return 0; }            // st_device_bytes: what the state holds beside weights, arena and parameters
    virtual int64_t train_serial() const { return 0; }            // st_train_serial
    virtual void params_moved() {}                                // st_load_param / st_bind_param gave a parameter another device pointer
    virtual void arena_moved() {}                                 // ensure_ws is about to free the arena
};

// The kinds that train through SdTrain.  finalize(): the held activations are of the weights before this re-bind / re-load.
struct HeldState : KindState {
    SdTrain held;
    using KindState::KindState;
    ~HeldState() override;
    SdTrain* begin() { held.have = false; return &held; }      // a training forward starts: what was held is stale from here on
    int finalize(st_engine* e) override;
    int64_t device_bytes() const override { return (int64_t)(held.act_cap + held.scr_cap); }
    int64_t train_serial() const override { return held.have ? held.serial : 0; }
};

}  // namespace sthost

constexpr int kSplitKMax = 16;
// The launch policy gemm() reads for every caller
struct st_tile_policy {
    int big_min_blocks = 192;           // 256x256 tiles only when the launch has at least this many of them (~3/4 block per CU); read once
                                        // from ST_BIG_MIN_BLOCKS at st_create (tests force either tile family with it)
    int phased = 1;                     // k = 3 convs on 256-wide tiles use the phased K loop (conv_gemm_phased.h); ST_PHASED=0: A/B runs
    int ragged_skip = 1;                // conv / attention launches skip frame tiles past an utterance's last needed frame (ST_RAGGED_SKIP=0: A/B)
    int small_tiles = 256;              // conv launches of <= this many 128x128 tiles use the 64-frame tile variants (0: never)
    int splitk_max = kSplitKMax, splitk_min_stages = 4;
    int splitk_target = 256;            // split-K: blocks a small conv launch is brought up to (gemm()); 0: never
    float* kpart = nullptr;             // split-K partial planes [ks][items][T][256] fp32
    size_t kpart_bytes = 0;
};

struct st_engine {
    int device = 0;
    sthost::Kind kind = sthost::KIND_DECODER;
    int dt = st::DT_BF16;
    std::string err;
    std::unique_ptr<sthost::KindState> state;      // never null (new_handle)

    std::map<std::string, sthost::Param> params;
    bool finalized = false;
    std::vector<void*> owned;           // device allocations to free (dev_alloc: the packed weights)
    int64_t weight_bytes = 0;
    void* zeros = nullptr;              // 256 zero bytes: halo source of the LDS-DMA conv path

    // workspace arena
    char* ws = nullptr; size_t ws_cap = 0;
    uint64_t ws_sig = 0;                // layout signature of what the arena last held (see arena_fresh)

    // debug / profile
    bool capture = false;
    std::map<std::string, sthost::Captured> caps;
    bool prof = false;
    uint64_t prof_mask = ~0ull;
    int prof_stride = 1;
    int64_t prof_seen[sthost::PC_COUNT] = {0};
    std::vector<sthost::ProfEvent> evs;
    std::vector<hipEvent_t> ev_pool;
    int64_t prof_launches[sthost::PC_COUNT] = {0};
    double prof_ms[sthost::PC_COUNT] = {0};
    double prof_flops[sthost::PC_COUNT] = {0};

    st_tile_policy tile;

    ~st_engine();      // the state, then parameters, packed weights, captures, profile events, arena (the device is current and idle)
    int fail(int code, const std::string& msg) { err = msg; return code; }
};


namespace sthost {

// A handle's state as its kind's type: valid after check_handle (or a creator's new_handle) of that kind
template <class S> S* state_of(st_engine* e) { return static_cast<S*>(e->state.get()); }
template <class S> const S* state_of(const st_engine* e) { return static_cast<const S*>(e->state.get()); }
// The entry points that take a const handle and set no message: the state, or nullptr for a null handle or one of another kind
template <class S> const S* state_if(const st_engine* e, Kind kind) { return e && e->kind == kind ? state_of<S>(e) : nullptr; }

#define HIPCHK(e, call)                                                                         \
    do {                                                                                        \
        hipError_t _err = (call);                                                               \
        if (_err != hipSuccess)                                                                 \
            return (e)->fail(ST_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_err));  \
    } while (0)

int dev_alloc(st_engine* e, void** p, size_t bytes);     // a packed-weight buffer: freed with e->owned, counted in e->weight_bytes
void free_owned(st_engine* e);                             // a finalize that packs anew: frees them all, weight_bytes = 0
const float* P(st_engine* e, const std::string& name);
hipError_t gemm(st_engine* e, int taps, int epi, const st::ConvGemmArgs& a, hipStream_t s);
bool gemm_is_phased(const st_engine* e, int taps, const st::ConvGemmArgs& a);   // gemm() would run the 256 x 254 phased kernel (the tile that has EPI_SILU)
void prof_collect(st_engine* e);
void capture(st_engine* e, const std::string& name, const void* dev, int64_t n, bool is16, hipStream_t s);
int ensure_ws(st_engine* e, size_t bytes);
// Entry checks, each with ONE message.  check_handle: ST_ERR_INVALID for a null handle, ST_ERR_STATE for a handle of another kind.
int check_handle(st_engine* e, Kind kind);
int check_finalized(st_engine* e);
int check_sizes(st_engine* e, int B, int T, const char* t_name = "T");      // B and T >= 1
int check_dropout(st_engine* e, float p_dropout);
extern std::string g_create_error;
// The end of every st_create*: validates `device`, makes it current and returns a new handle of `kind` that owns `state`
// (code + g_create_error otherwise).  A creator that fails later deletes the handle.
int new_handle(Kind kind, int device, std::unique_ptr<KindState> state, st_engine** out);
void expect(st_engine* e, const std::string& name, std::vector<int64_t> shape);      // one row of the parameter table
const st_vocos_config& vocos_config_of(const st_engine* e);      // the st_vocos_config of a KIND_VOCODER handle
int64_t train_grad_layout(const st_engine* e, std::map<std::string, int64_t>* offs);   // flat parameter-gradient layout (64-byte aligned slices); returns the total

// HIP-event bracket around the launches of one kernel class (st_profile_*)
struct ProfScope {
    st_engine* e; hipStream_t s; int idx = -1;
    ProfScope(st_engine* e_, hipStream_t s_, int cls, double flops);
    ~ProfScope();
};

}  // namespace sthost
