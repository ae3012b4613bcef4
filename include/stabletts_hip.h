/*
 * stabletts_hip.h -- C ABI of libstabletts_hip.so: the MI355X (gfx950) native
 * conditional-flow-matching mel decoder of StableTTS.
 *
 * The reference (KdaiP/StableTTS) has no FFI layer; its boundary for this path is the
 * Python class models/flow_matching.py:11 `CFMDecoder`.  Each entry point below names the
 * reference interface it replaces.  Conventions:
 *   - every function returns 0 on success, a negative ST_ERR_* code on failure, and never
 *     throws across the ABI; st_last_error() returns the message of the last failure.
 *   - tensor pointers are BORROWED DEVICE pointers (fp32, contiguous, the reference's own
 *     layouts: (B, C, T) row-major), owned by the caller (torch).  The engine owns its packed
 *     16-bit weight copies and its workspace.
 *   - work is enqueued on the caller's HIP stream (`stream` = hipStream_t, e.g.
 *     torch.cuda.current_stream().cuda_stream) with no implicit device synchronisation.
 *   - a handle is one of nine kinds, each with its own creator: the CFM decoder, the text encoder, the Vocos vocoder, the style
 *     encoder, the duration predictor, the mel extractor, the period and resolution discriminators of the Vocos training step and the
 *     FireflyGAN vocoder; an
 *     entry point handed a handle of another kind returns ST_ERR_STATE.
 *   - one engine per device per process; an engine is not thread-safe (the reference is
 *     single-threaded per process: train.py:101-102, webui.py:128).
 */
#ifndef STABLETTS_HIP_H
#define STABLETTS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ST_ABI_VERSION 4

enum {
    ST_OK = 0,
    ST_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    ST_ERR_HIP = -2,          /* a HIP runtime call failed */
    ST_ERR_STATE = -3,        /* e.g. solve before all parameters were loaded */
    ST_ERR_UNSUPPORTED = -4   /* valid in the reference, not implemented natively (caller may fall back) */
};

/* MFMA operand type of the dense contractions (accumulation, residual stream, LayerNorm,
 * softmax statistics and the ODE state are always fp32). */
enum { ST_OPERAND_BF16 = 0, ST_OPERAND_F16 = 1,
       /* split-precision operands, st_create_ffgan only (every other st_create_* answers ST_ERR_INVALID): each MFMA operand x is the
        * pair hi = fl16(x), lo = fl16(x - hi) of the named format and each product w_hi x_hi + w_hi x_lo + w_lo x_hi -- about 22 bits
        * of the fp32 operand at three times the MFMA work.  A bf16 pair carries 16 bits, so ST_OPERAND_BF16_SPLIT keeps the fourth product
        * w_lo x_lo in the encoder, and its head (about 40 sequential convolutions) carries three bf16 parts per operand and six products */
       ST_OPERAND_BF16_SPLIT = 2, ST_OPERAND_F16_SPLIT = 3 };

/* Fixed-grid solvers of torchdiffeq.odeint as used at models/flow_matching.py:54. */
enum { ST_SOLVER_EULER = 0, ST_SOLVER_MIDPOINT = 1, ST_SOLVER_RK4 = 2,
       ST_SOLVER_DOPRI5 = 3,  /* adaptive Dormand-Prince 5(4), rtol = atol = 1e-5: the reference default (solver=None) */
       /* the other explicit adaptive pairs of torchdiffeq offered by webui.py:110, same controller and tolerances */
       ST_SOLVER_BOSH3 = 4, ST_SOLVER_FEHLBERG2 = 5, ST_SOLVER_ADAPTIVE_HEUN = 6,
       ST_SOLVER_IMPLICIT_ADAMS = 7 };  /* torchdiffeq 'implicit_adams' (webui.py:110): Adams-Bashforth-Moulton on the fixed grid of n_steps,
                                           functional iteration of the corrector (<= 4 evaluations per step, rtol = atol = 1e-5) */

/* Constructor arguments of reference CFMDecoder.__init__ (models/flow_matching.py:12). */
typedef struct st_config {
    int32_t noise_channels;   /* = cond_channels = out_channels = n_mels (config.py:12: 128) */
    int32_t hidden_channels;  /* 256 (config.py:23) */
    int32_t filter_channels;  /* 1024 */
    int32_t n_heads;          /* 4 */
    int32_t n_layers;         /* 6 (n_dec_layers) */
    int32_t kernel_size;      /* 3 */
    int32_t gin_channels;     /* 256 */
    int32_t operand_dtype;    /* ST_OPERAND_* */
} st_config;

typedef struct st_engine st_engine;

/* ABI version of the loaded library (compare with ST_ABI_VERSION). */
int st_abi_version(void);

/* Replaces CFMDecoder.__init__ / Decoder.__init__ (models/flow_matching.py:12-22,
 * models/estimator.py:66-96): validates the architecture (same assertions: n_layers even,
 * hidden % n_heads == 0, even time-embedding dim) and creates an engine on HIP device `device`. */
int st_create(const st_config* cfg, int device, st_engine** out);

void st_destroy(st_engine* e);

/* Message of the last failure on this engine (e == NULL: last st_create failure). */
const char* st_last_error(const st_engine* e);

/* Replaces nn.Module.load_state_dict for `decoder.estimator.*` (api.py:49, utils/load.py:31-41):
 * uploads one tensor by its reference state_dict name, fp32,
 * reference shapes (Conv1d weights (Cout, Cin, K)).  `data` may be a host or a device pointer. */
int st_load_param(st_engine* e, const char* name, const float* data, const int64_t* shape, int ndim);

/* Number of state_dict tensors the configured architecture expects (116 for the 31M model). */
int st_num_params(const st_engine* e);

/* Enumerates the expected tensors (index in [0, st_num_params), name order): reference state_dict name and
 * shape, so that a host without the Python module tree can discover what to load.  Returns the number of
 * dimensions (<= 4) and writes them to shape[0..ndim) if shape != NULL; *name points into the engine. */
int st_param_info(const st_engine* e, int index, const char** name, int64_t* shape);

/* Packs the uploaded fp32 parameters into the engine's 16-bit MFMA operand layouts.  Must be
 * called after loading (and again after any parameter update).  Synchronises the device. */
int st_finalize(st_engine* e);

/* The training-loop form of the two calls above (nn.Parameter semantics: train.py:78-82 updates the weights in place
 * every iteration).  st_bind_param makes the engine READ the fp32 tensor at the caller's device pointer instead of
 * keeping a copy: `data` (device memory, reference shape) stays owned by the caller and must outlive the binding
 * (re-bind after the storage moves).  After an in-place update of bound tensors (optimizer.step()), st_repack
 * re-packs the 16-bit operand copies INTO THE EXISTING BUFFERS as kernels on `stream` -- no allocation, no host
 * copy, no device synchronisation; it needs one earlier st_finalize (which allocates them). */
int st_bind_param(st_engine* e, const char* name, const float* data, const int64_t* shape, int ndim);
int st_repack(st_engine* e, void* stream);

/* Replaces Decoder.forward(t, x, mask, mu, c) (models/estimator.py:103-138): ONE vector-field
 * evaluation.  t: device fp32, t_len = 1 (inference, 0-dim t) or B (training, flow_matching.py:99).
 * x, mu, out: (B, n_feats, T); mask: (B, 1, T) float 0/1; c: (B, gin). */
int st_estimator_forward(st_engine* e, const float* t, int t_len, const float* x, const float* mu,
                         const float* mask, const float* c, float* out, int B, int T, void* stream);

/* Replaces CFMDecoder.forward (models/flow_matching.py:25-55) + cfg_wrapper (:58-67) +
 * torchdiffeq.odeint fixed-grid stepping (:54): the whole ODE solve.
 *   z            : initial noise (B, n_feats, T), ALREADY multiplied by the temperature (:45).
 *   n_steps      : n_timesteps; the grid is linspace(0, 1, n_steps + 1) (:46).
 *   solver       : ST_SOLVER_*.  For the adaptive solvers (>= ST_SOLVER_DOPRI5) n_steps only names the output grid of the reference
 *                  call (flow_matching.py:46,54) and does not influence the steps taken.
 *   use_cfg != 0 : classifier-free guidance with fake_speaker (gin,), fake_content (n_feats,)
 *                  and cfg_strength (models/model.py:43-44,102); cond and uncond branches run as
 *                  one 2B batch.
 *   out          : trajectory[-1], (B, n_feats, T).
 * Environment: ST_HIP_GRAPH=1 replays the fixed-grid solve body (everything between the boundary layout
 * conversions) from a HIP graph captured at the second call with the same (B, T, n_steps, solver, CFG) signature. */
int st_cfm_solve(st_engine* e, const float* mu, const float* mask, const float* z, const float* c,
                 int n_steps, int solver, int use_cfg, float cfg_strength,
                 const float* fake_speaker, const float* fake_content,
                 float* out, int B, int T, void* stream);

/* ---- TextEncoder: the caller side of the path, on the same DiT block kernels ---------------- */

/* Replaces TextEncoder.__init__ (models/text_encoder.py:9-28).  cfg fields are read as: noise_channels =
 * out_channels (n_mels), hidden / filter / n_heads / kernel_size / gin_channels / operand_dtype as for the
 * decoder, n_layers = n_enc_layers (any 1..16).  Parameters are loaded with st_load_param under the reference
 * names ("emb.weight", "encoder.<i>.attn.conv_q.weight", ..., "proj.bias") and packed by st_finalize; the handle
 * is destroyed with st_destroy.  The decoder entry points reject such a handle and vice versa. */
int st_create_text_encoder(const st_config* cfg, int n_vocab, int device, st_engine** out);

/* Replaces TextEncoder.forward(x, c, x_lengths) (models/text_encoder.py:34-44).
 *   tokens  : (B, T) int64 phoneme ids (ids outside [0, n_vocab) are clamped; nn.Embedding would raise)
 *   lengths : (B,) int64 valid lengths;  c: (B, gin) fp32 speaker vectors          -- all device pointers
 *   x_out   : (B, hidden, T) fp32 encoder states;  mu_out: (B, n_mels, T) fp32 = proj(x) * mask;
 *   mask_out: (B, 1, T) fp32 sequence mask (utils/mask.py). */
int st_text_encoder_forward(st_engine* e, const int64_t* tokens, const int64_t* lengths, const float* c,
                            float* x_out, float* mu_out, float* mask_out, int B, int T, void* stream);

/* ---- duration -> alignment -> mu_y: the caller side between TextEncoder and CFMDecoder ------------ */
/* Stateless (no engine handle; a failure's message is st_last_error(NULL)); all pointers are device pointers.       */

/* Replaces models/model.py:85-87 (synthesise): w = exp(logw) * x_mask; w_ceil = ceil(w) * length_scale;
 * y_lengths = clamp_min(sum(w_ceil), 1).long().  logw, x_mask: (B, 1, Tx) fp32.  Outputs: w_ceil (B, Tx),
 * cum (B, Tx) = cumsum(w_ceil) (generate_path's first step, :19; sequential fp32), y_lengths (B) int64.  The host
 * reads y_lengths.max() to size the mel tensors, exactly as the reference does at :88. */
int st_durations(const float* logw, const float* x_mask, float length_scale, int B, int Tx, float* w_ceil, float* cum,
                 int64_t* y_lengths, void* stream);

/* Replaces generate_path(duration, mask) (models/model.py:17-27): duration (B, Tx), mask (B, Tx, Ty) -> path (B, Tx, Ty)
 * 0/1 monotonic alignment.  cum_scratch: (B, Tx) fp32 workspace. */
int st_generate_path(const float* duration, const float* mask, int B, int Tx, int Ty, float* cum_scratch, float* path, void* stream);

/* Replaces models/model.py:91-95: y_mask = sequence_mask(y_lengths, Ty); attn = generate_path(w_ceil, x_mask x y_mask);
 * mu_y = attn^T mu_x -- as ONE gather (every mel frame copies the text position its 0/1 alignment column selects).
 * cum (B, Tx) from st_durations; mu_x (B, M, Tx); outputs mu_y (B, M, Ty), y_mask (B, 1, Ty) (optional) and the
 * alignment attn (B, Tx, Ty) (optional, NULL to skip: synthesise returns it, the decoder does not need it). */
int st_align(const float* cum, const float* x_mask, const int64_t* y_lengths, const float* mu_x, int B, int M, int Tx, int Ty,
             float* attn, float* mu_y, float* y_mask, void* stream);

/* ---- monotonic alignment search of training (models/model.py:148-158), stateless like the alignment helpers above ------ */

/* Replaces monotonic_align.maximum_path (monotonic_align/core.py:14-46) without the host round trip: bit-exact for every
 * item with t_x >= 1 and t_y >= 1 (t_x > t_y included).
 *   neg_cent  : (B, Ty, Tx) fp32, rows = mel frames; read only.
 *   t_y, t_x  : (B) int32, the reference's mask.sum(1)[:, 0] and mask.sum(2)[:, 0] truncated (clamped to [0, Ty] / [0, Tx]).
 *   path      : (B, Ty, Tx) fp32 0/1, every cell written; an item with t_x == 0 or t_y == 0 gets an all-zero path (the
 *               reference writes the last column through a negative index there; models/model.py never makes that case).
 *   durations : (B, Tx) int32 frames per token (= path.sum(1)), or NULL.
 *   workspace : st_maximum_path_workspace_bytes(B, Ty, Tx) bytes of device memory, NULL when that is 0.
 * Tx <= 4096 (one wave holds a row in registers); a wider Tx returns ST_ERR_UNSUPPORTED before any launch.  Any Ty. */
int st_maximum_path(const float* neg_cent, const int32_t* t_y, const int32_t* t_x, int B, int Ty, int Tx, float* path,
                    int32_t* durations, void* workspace, void* stream);
/* 0 when each utterance's decision bits (Ty x ceil(Tx / 64) x 8 bytes) fit the kernel's LDS budget (64 KiB). */
int64_t st_maximum_path_workspace_bytes(int B, int Ty, int Tx);

/* models/model.py:150-155 with s_p_sq_r = 1, all four terms:
 * neg_cent[b][t][s] = D (-1/2 log 2 pi) - 1/2 sum_d y[b][d][t]^2 + sum_d y[b][d][t] mu_x[b][d][s] - 1/2 sum_d mu_x[b][d][s]^2
 *   mu_x (B, D, Tx), y (B, D, Ty) fp32 -> neg_cent (B, Ty, Tx) fp32 (the cross term on the fp32-input MFMA). */
int st_mas_neg_cent(const float* mu_x, const float* y, int B, int D, int Tx, int Ty, float* neg_cent, void* stream);

/* ---- the step between the alignment search and the decoder in training (models/model.py:160-176), stateless ------------ */
/* The alignment has one token per frame and contiguous frames per token, so these take the per-token frame counts
 * st_maximum_path writes and never a dense (B, Ty, Tx) tensor.  fp32 tensors; the sums behind a loss or a gradient accumulate
 * in fp64 in one fixed order (no atomics): results do not depend on the batch, the grid or the neighbouring tokens.
 *
 * st_align_train_forward replaces model.py:166-168, :171-172 and :175-176.
 *   durations    : (B, Tx) int32.  A token counts only where x_mask != 0, a negative count is 0, and the running sum is
 *                  clipped to [0, Ty] before use: no durations tensor can index outside a buffer.
 *   x_mask, y_mask : (B, 1, Tx), (B, 1, Ty);  mu_x (B, M, Tx);  y (B, M, Ty).
 *   fake_content : (M) or NULL (= 0);  keep: (B), the cfg_mask of :138 as 0 / non-zero, or NULL (every item kept).
 *   frame_token  : (B, Ty) int32, the token of each frame, -1 where no token covers it.
 *   mu_y         : (B, M, Ty) or NULL: mu_x gathered by frame_token, 0 where frame_token < 0 (= attn^T mu_x, exactly).
 *   mu_y_masked  : (B, M, Ty): mu_y * keep + (1 - keep) * fake_content; a dropped item holds fake_content in every frame.
 *   scratch      : st_align_train_scratch_floats(B, M, Ty) floats; keeps the denominator sum(y_mask) * M for the backward.
 *   prior_loss   : device scalar, sum(0.5 ((y - mu_y)^2 + log 2 pi) y_mask) / (sum(y_mask) * M).
 * Tx <= 4096; a wider Tx returns ST_ERR_UNSUPPORTED before any launch.
 *
 * st_align_train_backward: for token i of item b with frames [s, s + d), ascending t,
 *   grad_mu_x[b][m][i] = sum_t keep_b g_masked[b][m][t] + g_mu_y[b][m][t] + g_prior y_mask[b][t] (mu_x[b][m][i] - y[b][m][t]) / denom
 *   (every element written; 0 for a token without frames);  grad_fake_content[m] = sum over items with keep == 0 and every
 *   frame t in [0, Ty) of g_masked[b][m][t] (NULL to skip).  grad_mu_y_masked, grad_mu_y (B, M, Ty) and grad_prior (device
 *   scalar) may each be NULL: that term is 0.  y, y_mask and scratch are read only with grad_prior. */
int st_align_train_scratch_floats(int B, int M, int Ty);
int st_align_train_forward(const int32_t* durations, const float* x_mask, const float* y_mask, const float* mu_x, const float* y,
                           const float* fake_content, const float* keep, int B, int M, int Tx, int Ty, int32_t* frame_token,
                           float* mu_y, float* mu_y_masked, float* scratch, float* prior_loss, void* stream);
int st_align_train_backward(const int32_t* durations, const float* x_mask, const float* y_mask, const float* mu_x, const float* y,
                            const float* keep, const float* scratch, const float* grad_mu_y_masked, const float* grad_mu_y,
                            const float* grad_prior, int B, int M, int Tx, int Ty, float* grad_mu_x, float* grad_fake_content,
                            void* stream);

/* Replaces model.py:162-163 and duration_loss (models/duration_predictor.py:38-40).
 * st_duration_loss: logw_ = log(1e-8 + durations) * x_mask -> logw_target (B, 1, Tx), or NULL to skip;
 *   loss = sum((logw - logw_)^2) / sum(x_lengths) -> *loss (device), over every element as the reference sums it.
 *   logw, x_mask: (B, 1, Tx); durations (B, Tx) int32 (a negative count is 0); x_lengths (B) int64;
 *   scratch: st_duration_loss_scratch_floats() floats, keeps the denominator for the backward.
 *   The difference logw - logw_ is formed in fp64: it cancels where the prediction is good.
 * st_duration_loss_backward: grad_logw = grad_loss[0] * 2 (logw - logw_) / sum(x_lengths)  (grad_loss: device scalar). */
int st_duration_loss(const float* logw, const int32_t* durations, const float* x_mask, const int64_t* x_lengths, int B, int Tx,
                     float* logw_target, float* scratch, float* loss, void* stream);
int st_duration_loss_backward(const float* logw, const int32_t* durations, const float* x_mask, const float* scratch,
                              const float* grad_loss, int B, int Tx, float* grad_logw, void* stream);
int st_duration_loss_scratch_floats(void);

/* ---- CFMDecoder.compute_loss's own arithmetic (models/flow_matching.py:86-100), stateless like the alignment helpers ------
 * st_cfm_loss_prep: t = 1 - cos(t_rand pi / 2) (:88), y = (1 - (1 - sigma) t) z + t x1 (:93), u = x1 - (1 - sigma) z (:96).
 *   x1, z, y, u: (B, M, T); t_rand, t: (B).
 * st_cfm_loss: loss = sum((pred - u)^2) / (sum(mask) * M) (:100; u is NOT masked, as in the reference) -> *loss (device);
 *   scratch: st_cfm_loss_scratch_floats() floats, keeps the denominator for the backward; deterministic summation order.
 * st_cfm_loss_backward: grad_pred = grad_loss[0] * 2 (pred - u) / (sum(mask) * M)  (grad_loss: device scalar). */
int st_cfm_loss_prep(const float* x1, const float* z, const float* t_rand, float sigma_min, int B, int M, int T, float* t, float* y,
                     float* u, void* stream);
int st_cfm_loss(const float* pred, const float* u, const float* mask, int B, int M, int T, float* scratch, float* loss, void* stream);
int st_cfm_loss_backward(const float* pred, const float* u, const float* scratch, const float* grad_loss, int B, int M, int T,
                         float* grad_pred, void* stream);
int st_cfm_loss_scratch_floats(void);

/* ---- Vocos vocoder: mel -> waveform, the step after the decoder (api.py:76) ------------------------ */

/* Replaces Vocos.__init__(VocosConfig(), MelConfig()) (vocoders/vocos/models/model.py:11-15, config.py:4-19,46-50). */
typedef struct st_vocos_config {
    int32_t input_channels;    /* n_mels, config.py:47; native kernels: a multiple of 16 up to 192 (e.g. 80, 96, 128) */
    int32_t dim;               /* config.py:48; native kernels: 512, 768 (the Vocos trainer's, vocoders/vocos/config.py:23) or 1024 */
    int32_t intermediate_dim;  /* config.py:49 (multiple of 256) */
    int32_t num_layers;        /* config.py:50 (1..32) */
    int32_t n_fft;             /* MelConfig.n_fft, config.py:6; native kernels: 256, 512, 1024 or 2048 */
    int32_t hop_length;        /* MelConfig.hop_length, config.py:8; native kernels: n_fft / 4 */
    int32_t operand_dtype;     /* ST_OPERAND_* of the GEMM operands (accumulation, LayerNorms, residual stream, ISTFT: fp32) */
} st_vocos_config;

/* The handle takes the parameters of Vocos.state_dict() under their reference names ("backbone.embed.weight", ...,
 * "backbone.convnext.<i>.gamma", ..., "head.out.bias", "head.istft.window") through st_load_param / st_finalize and
 * is destroyed with st_destroy.  The decoder / text-encoder entry points reject it and vice versa.
 * Accepted: n_fft 256, 512, 1024 or 2048 with hop_length == n_fft / 4 (44.1 kHz: 2048 / 512; 22.05-24 kHz: 1024 / 256; 16 kHz:
 * 512 / 128), input_channels a multiple of 16 up to 192, dim 512, 768 or 1024, intermediate_dim a multiple of 256.  Anything else
 * -- another n_fft, hop_length != n_fft / 4, a width such as Vocos-24k's 100 -- is ST_ERR_UNSUPPORTED before a device is touched,
 * with a message that states the rule. */
int st_create_vocoder(const st_vocos_config* cfg, int device, st_engine** out);

/* Replaces Vocos.forward(x) (model.py:17-20) = ISTFTHead(VocosBackbone(x)) (backbone.py:50-56, head.py:93-117 with
 * padding="same"):  mel (B, input_channels, T) fp32 -> audio (B, T * hop_length) fp32, device pointers.  Like the
 * reference there is no mask: every utterance is vocoded at the padded length T (a batch of different lengths:
 * st_vocos_forward_ragged).  Large batches run in chunks of whole utterances (32-bit row offsets inside the GEMMs, the
 * device's grid-y limit); only a T that exceeds the row bound on its own is rejected (ST_ERR_INVALID), as is a batch that
 * needs more than one chunk while debug capture is on. */
int st_vocos_forward(st_engine* e, const float* mel, float* audio, int B, int T, void* stream);

/* st_vocos_forward on a ragged batch: utterance b has lengths[b] frames, and its audio equals that utterance vocoded alone
 * (the padded frames of st_vocos_forward are not zero activations: they reach back through the k = 7 convolutions and the
 * ISTFT overlap into the last ~12 frames of every shorter utterance).
 *   mel     : (B, input_channels, T) fp32, device; frames from lengths[b] on are never read
 *   lengths : B entries in HOST memory, each in [1, T]  (e.g. length_regulate's y_lengths)
 *   audio   : (B, T * hop_length) fp32, device; every sample is written, those from lengths[b] * hop_length on as 0.0
 * Every activation between the two is packed: the GEMMs run over sum(lengths) rows, not B * T.  With every length equal to
 * T the audio is bitwise st_vocos_forward's (same kernels' arithmetic, same row count).  Everything is validated before the
 * device is touched (a null pointer or a length outside [1, T]: ST_ERR_INVALID naming the index).  Chunks are whole
 * utterances bounded by their PACKED rows (the 32-bit row bound of st_vocos_forward) and by 2^23 padded frames; an
 * utterance that exceeds the row bound on its own is rejected, as is a multi-chunk batch while debug capture is on (a
 * single-chunk call captures packed (sum(lengths), .) tensors).  Enqueued on `stream`; the length table travels through
 * one of four pinned slots guarded by events, so back-to-back calls do not wait on each other. */
int st_vocos_forward_ragged(st_engine* e, const float* mel, const int64_t* lengths, float* audio, int B, int T, void* stream);

/* ---- Vocos generator training: autograd counterpart of Vocos.forward on a vocoder handle (the generator step of
 * vocoders/vocos/train.py:94,115,128).  fp32 values and accumulation throughout (fp32-input MFMA): the parameters are read
 * IN PLACE from the tensors st_bind_param holds (or st_load_param's copies), so an optimizer step needs no re-pack for these two
 * entries; "head.istft.window" is a buffer and gets no gradient.  The waveform is therefore not bitwise st_vocos_forward's
 * (16-bit GEMM operands); it is closer to the fp32 reference.
 * st_vocos_train_forward: mel (B, input_channels, T) -> audio (B, T * hop_length), keeping the activations of this ONE forward in the
 * handle (st_train_serial counts the forwards; st_finalize drops them).
 * st_vocos_train_backward: d_audio (B, T * hop_length) = d loss / d audio -> EVERY parameter gradient into grad_flat
 * (st_train_grad_numel() floats in the layout of st_train_grad_offset: 64-byte aligned slices, the gaps and the window's slice are
 * not written) and, unless d_mel is NULL, d loss / d mel (B, input_channels, T).  B and T must be the forward's; without a held
 * forward the call fails with ST_ERR_STATE.  No atomics, every reduction in a fixed order: gradients are bitwise repeatable.
 * One batch per call (no chunking): B * T * max(7 input_channels, intermediate_dim, 2304) < 2^31 and B <= 65535, else ST_ERR_INVALID.
 * Training is built for n_fft == 2048, hop_length == 512 and input_channels 64, 128 or 192: on a handle of any other configuration
 * (which st_create_vocoder accepts for inference) both entries return ST_ERR_UNSUPPORTED before any allocation or launch. */
int st_vocos_train_forward(st_engine* e, const float* mel, float* audio, int B, int T, void* stream);
int st_vocos_train_backward(st_engine* e, const float* d_audio, float* d_mel /* nullable */, float* grad_flat, int B, int T, void* stream);

/* ---- FireflyGAN vocoder (vocoders/ffgan, the default vocoder of api.py:19-24,39): mel -> waveform, inference only -------- */

#define ST_FFGAN_MAX_STAGES 8
#define ST_FFGAN_MAX_UPSAMPLES 8
#define ST_FFGAN_MAX_RESBLOCKS 4
#define ST_FFGAN_MAX_DILATIONS 4

/* Replaces FireflyGANBase.__init__ (vocoders/ffgan/model.py:7-29,44-50): ConvNeXtEncoder(**config_dict["backbone"]) and
 * HiFiGANGenerator(**config_dict["head"]).  The head's num_mels is the encoder's last width.
 * What the native kernels implement -- anything else is ST_ERR_INVALID with a message from st_create_ffgan, before the device is touched:
 *   - use_template == 0 (no noise convolutions);
 *   - input_channels 64, 128 or 192; encoder kernel_size 7; 1..8 stages of depth >= 1 whose widths are multiples of 128 up to 1024;
 *   - 1..8 upsamples, each with an even rate u in [2, 16] and kernel size 2u; the head's widths upsample_initial_channel / 2^i are
 *     16 * 2^n with the last one >= 16, and upsample_initial_channel is 16, 32, 64 or a multiple of 128;
 *   - 1..4 resblocks with odd kernel sizes <= 13 and 1..4 dilations each (one conv pair per dilation), every halo
 *     (kernel / 2) * dilation <= 25 rows (the LDS patch of the convolution kernel holds 128 + 2 * 25 rows);
 *   - odd pre / post conv kernel sizes <= 13. */
typedef struct st_ffgan_config {
    int32_t input_channels;                                   /* mel channels, model.py:10 */
    int32_t n_stages;
    int32_t depths[ST_FFGAN_MAX_STAGES];                      /* model.py:11 */
    int32_t dims[ST_FFGAN_MAX_STAGES];                        /* model.py:12 */
    int32_t kernel_size;                                      /* model.py:14 */
    int32_t n_upsamples;
    int32_t upsample_rates[ST_FFGAN_MAX_UPSAMPLES];           /* model.py:19; their product is the hop length */
    int32_t upsample_kernel_sizes[ST_FFGAN_MAX_UPSAMPLES];    /* model.py:20 */
    int32_t n_resblocks;
    int32_t resblock_kernel_sizes[ST_FFGAN_MAX_RESBLOCKS];    /* model.py:21 */
    int32_t n_dilations;
    int32_t resblock_dilation_sizes[ST_FFGAN_MAX_RESBLOCKS][ST_FFGAN_MAX_DILATIONS];      /* model.py:22 */
    int32_t upsample_initial_channel;                         /* model.py:24 */
    int32_t pre_conv_kernel_size, post_conv_kernel_size;      /* model.py:26-27 */
    int32_t use_template;                                     /* model.py:25; native: 0 */
    int32_t operand_dtype;     /* ST_OPERAND_* of the MFMA operands, the two _SPLIT values included (accumulation, LayerNorms, residual streams,
                                  conv_post, tanh: fp32) */
} st_ffgan_config;

/* The handle takes the parameters of FireflyGANBase.state_dict() under their reference names ("backbone.downsample_layers.0.0.weight",
 * ..., "head.conv_pre.parametrizations.weight.original0" / "original1" (the g and v of a weight-normed conv), ...,
 * "head.resblocks.<i>.blocks.<b>.convs1.<p>.bias", ...) through st_load_param / st_finalize, which folds w = g v / ||v|| (the norm over
 * all dims but 0: the input channel of a ConvTranspose1d) and packs the 16-bit weights.  The other entry points reject the handle
 * and vice versa.  A split-precision handle (ST_OPERAND_*_SPLIT) takes the same parameters and serves the same two forward calls with
 * the same guarantees; its weights are packed as hi / lo pairs and its head keeps the tensor between the two convs of a ResBlock pair
 * in fp32, which makes the head's workspace 16 bytes per channel-sample of the widest level in place of 14. */
int st_create_ffgan(const st_ffgan_config* cfg, int device, st_engine** out);

/* Replaces FireflyGANBase.forward(x) (model.py:52-57): mel (B, input_channels, T) fp32 -> audio (B, T * hop) fp32, device pointers,
 * hop = the product of the upsample rates.  No mask, as in the reference: every utterance is vocoded at the padded length T (a batch of
 * different lengths: st_ffgan_forward_ragged), and no kernel reads a neighbouring utterance.  The ParralelBlock mean is accumulated in block order on one stream, without atomics: two
 * calls agree bit for bit.  Every tensor offset in the head kernels is 64-bit; large batches run in chunks of whole utterances so that
 * the head's workspace (three fp32 tensors and one 16-bit tensor of the widest level, 14 bytes per channel-sample; a split-precision
 * handle: four fp32 tensors, 16 bytes) stays below
 * 1 GiB (one utterance if that alone is more) and the encoder's GEMM rows within 32-bit offsets.  T up to 2^20; a T whose encoder rows
 * exceed the row bound on its own, and a batch that needs more than one chunk while debug capture is on, are ST_ERR_INVALID. */
int st_ffgan_forward(st_engine* e, const float* mel, float* audio, int B, int T, void* stream);

/* st_ffgan_forward on a ragged batch: utterance b has lengths[b] frames, and its audio equals that utterance vocoded alone (the
 * padded frames of st_ffgan_forward are not zero activations: they reach back through the encoder's k = 7 convolutions and the
 * head's dilated ones into the end of every shorter utterance).
 *   mel     : (B, input_channels, T) fp32, device; frames from lengths[b] on are never read
 *   lengths : B entries in HOST memory, each in [1, T]  (e.g. length_regulate's y_lengths)
 *   audio   : (B, T * hop) fp32, device; every sample is written, those from lengths[b] * hop on as 0.0
 * Every activation between the two is packed: sum(lengths) rows in the encoder and sum(lengths) * up rows at a head level, not
 * B * T.  A head tile runs the arithmetic of st_ffgan_forward on its utterance alone, so with every length equal to T the audio is
 * bitwise st_ffgan_forward's, and an utterance's audio does not depend on its neighbours' mel, lengths or order as long as the
 * encoder's GEMMs select the same tile for the row count.  Everything is validated before the device is touched (a null pointer or
 * a length outside [1, T]: ST_ERR_INVALID naming the index).  Chunks are whole utterances bounded by their PACKED rows -- the 1 GiB
 * head workspace at 14 bytes (split-precision handle: 16) per channel-sample of the widest level (one utterance if that alone is more), the encoder's 32-bit row
 * bound -- and by 65535 utterances; an utterance that exceeds the row bound on its own is rejected, as is a multi-chunk batch while
 * debug capture is on (a single-chunk call captures packed tensors: "ffgan.encoder" (sum(lengths), D), "ffgan.pre_tanh"
 * (sum(lengths) * hop)).  Enqueued on `stream`; the length table travels through one of four pinned slots guarded by events, as
 * for st_vocos_forward_ragged, so back-to-back calls do not wait on each other. */
int st_ffgan_forward_ragged(st_engine* e, const float* mel, const int64_t* lengths, float* audio, int B, int T, void* stream);

/* ---- period discriminator of the Vocos training step (vocoders/vocos/models/discriminator.py:32-75, train.py:98-128) ---- */
/* One handle serves one DiscriminatorP(period, in_channels = 1, kernel_size = 5, stride = 3, lrelu_slope); the five of a
 * MultiPeriodDiscriminator are five handles.  fp32 throughout, the reference's (B, C, H, period) layout, no atomics: every value
 * and gradient is bitwise repeatable, and an item's values do not depend on the rest of the batch.  Layers 1-4 are GEMMs on the
 * fp32-input MFMA (forward, data gradient, weight gradient); layer 0, conv_post and the weight norm are vector kernels. */
typedef struct st_period_disc_config {
    int32_t period;       /* >= 1 */
    float lrelu_slope;    /* > 0: the backward takes the pre-activation's sign from the kept post-activation */
} st_period_disc_config;

/* The handle takes the reference's state-dict entries through st_load_param / st_bind_param / st_finalize:
 * "convs.{i}.parametrizations.weight.original0" (g: Cout, 1, 1, 1), "...original1" (v: Cout, Cin, 5, 1), "convs.{i}.bias" for
 * i = 0..4 and the same three under "conv_post." (v: 1, 1024, 3, 1).  st_finalize computes the effective weights v g / ||v||
 * once; after an in-place update of bound tensors st_repack(e, stream) computes them again as kernels on `stream`.  Either
 * drops the activations a training forward left.  Destroyed with st_destroy. */
int st_create_period_discriminator(const st_period_disc_config* cfg, int device, st_engine** out);

/* Feature map `index` (0..3: after convs.1..4, 4: conv_post's output, the logits) of a T-sample input is (B, *channels, *rows,
 * period).  ST_ERR_INVALID for a bad index or a T the forward rejects. */
int st_period_disc_fmap_shape(const st_engine* e, int T, int index, int64_t* channels, int64_t* rows);

/* Replaces DiscriminatorP.forward:  x (B, 1, T) -> the five feature maps, fp32 device pointers in fmaps[0..4] (shapes above); the
 * module's first return value is fmaps[4] flattened.  T % period != 0 pads the tail by reflection as the reference does, which
 * needs T > period - T % period (ST_ERR_INVALID otherwise, where F.pad raises).  st_period_disc_forward keeps nothing.
 * st_period_disc_train_forward keeps x and the post-activations of this ONE forward in the handle (st_train_serial counts it). */
int st_period_disc_forward(st_engine* e, const float* x, float* const* fmaps, int B, int T, void* stream);
int st_period_disc_train_forward(st_engine* e, const float* x, float* const* fmaps, int B, int T, void* stream);

/* Backward of the held forward.  d_fmaps[0..4]: d loss / d feature map, each entry may be NULL (no gradient reaches that map).
 * d_x (nullable): receives d loss / d x (B, 1, T), the padded samples' share folded onto the samples they mirror; NULL skips
 * layer 0's data gradient.  grad_flat (nullable): st_train_grad_numel() floats that receive every parameter gradient at
 * st_train_grad_offset(name) (the gaps are not written; with d_fmaps[4] == NULL neither are conv_post's slices); NULL skips every
 * weight-gradient and weight-norm kernel.  B and T must be the forward's: ST_ERR_STATE without a held forward or with another
 * shape, before any caller memory is touched. */
int st_period_disc_train_backward(st_engine* e, const float* const* d_fmaps, float* d_x /* nullable */, float* grad_flat /* nullable */,
                                  int B, int T, void* stream);

/* ---- resolution discriminator of the Vocos training step (vocoders/vocos/models/discriminator.py:112-171, train.py:98-128) ---- */
/* One handle serves one DiscriminatorR(window_length, channels = 32, hop_factor = 0.25, bands); the three of a
 * MultiResolutionDiscriminator are three handles.  fp32 throughout, the reference's (B, C, frames, F) layout, no atomics: every
 * value and gradient is bitwise repeatable, and an item's values do not depend on the rest of the batch.  The complex STFT
 * (hann window, hop window_length / 4, reflect padding) is written as the two input channels of layer 0; a band is the column range
 * [band_lo, band_hi) of its window_length / 2 + 1 bins.  The band convs are GEMMs on the fp32-input MFMA (forward, data gradient of
 * the 32 -> 32 layers, weight gradient); the STFT, layer 0's data gradient, conv_post and the weight norm are vector kernels. */
typedef struct st_resolution_disc_config {
    int32_t window_length;    /* a power of two in [32, 2048] (ST_ERR_UNSUPPORTED otherwise) */
    int32_t band_lo[5];       /* the bands as bin ranges, int(b * (window_length / 2 + 1)) of the reference's fractions; */
    int32_t band_hi[5];       /* an empty one is ST_ERR_UNSUPPORTED (the reference fails there), one outside the bins ST_ERR_INVALID */
    float lrelu_slope;        /* > 0 (the reference: 0.1): the backward takes the pre-activation's sign from the kept post-activation */
} st_resolution_disc_config;

/* The handle takes the reference's state-dict entries through st_load_param / st_bind_param / st_finalize:
 * "band_convs.{c}.{i}.parametrizations.weight.original0" (g: 32, 1, 1, 1), "...original1" (v: 32, 2 or 32, 3, 9; i = 4: 32, 32, 3, 3),
 * "band_convs.{c}.{i}.bias" for c, i = 0..4 and the same three under "conv_post." (v: 1, 32, 3, 3).  st_finalize computes the
 * effective weights v g / ||v|| once; after an in-place update of bound tensors st_repack(e, stream) computes them again as kernels
 * on `stream`.  Either drops the activations a training forward left.  Destroyed with st_destroy. */
int st_create_resolution_discriminator(const st_resolution_disc_config* cfg, int device, st_engine** out);

/* Feature map `index` (band-major: 4 c + i - 1 after band_convs.c.i, i = 1..4; 20: conv_post's output, the logits) of a T-sample
 * input is (B, *channels, *frames, *width), frames = 1 + T / (window_length / 4).  ST_ERR_INVALID for a bad index or a T the
 * forward rejects. */
int st_resolution_disc_fmap_shape(const st_engine* e, int T, int index, int64_t* channels, int64_t* frames, int64_t* width);

/* Split-K planes of the weight-gradient launch of band_convs.{band}.{layer} at (B, T): a figure for tests and tools (>= 1), or
 * ST_ERR_INVALID. */
int st_resolution_disc_wgrad_planes(const st_engine* e, int B, int T, int band, int layer);

/* Replaces DiscriminatorR.forward:  x (B, 1, T) -> the 21 feature maps, fp32 device pointers in fmaps[0..20] (shapes above); the
 * module's first return value is fmaps[20] itself.  The reflect padding needs T > window_length / 2 (ST_ERR_INVALID otherwise, where
 * torch.stft raises).  st_resolution_disc_forward keeps nothing.  st_resolution_disc_train_forward keeps the spectrum and the
 * post-activations of this ONE forward in the handle (st_train_serial counts it). */
int st_resolution_disc_forward(st_engine* e, const float* x, float* const* fmaps, int B, int T, void* stream);
int st_resolution_disc_train_forward(st_engine* e, const float* x, float* const* fmaps, int B, int T, void* stream);

/* Backward of the held forward.  d_fmaps[0..20]: d loss / d feature map, each entry may be NULL (no gradient reaches that map).
 * d_x (nullable): receives d loss / d x (B, 1, T), the reflected samples' share folded onto the samples they mirror; NULL skips
 * layer 0's data gradient and the whole STFT backward.  grad_flat (nullable): st_train_grad_numel floats, each parameter's gradient
 * at st_train_grad_offset(name) (the gaps are not written; with d_fmaps[20] == NULL neither are conv_post's slices); NULL skips
 * every weight-gradient and weight-norm kernel.  B and T must be the forward's: ST_ERR_STATE without a held forward or with another
 * shape, before any caller memory is touched. */
int st_resolution_disc_train_backward(st_engine* e, const float* const* d_fmaps, float* d_x /* nullable */, float* grad_flat /* nullable */,
                                      int B, int T, void* stream);

/* ---- the three scalar GAN losses of a Vocos step (vocoders/vocos/models/loss.py:37-66), stateless ------------------------- */
/* Each loss is a sum over a LIST of tensors of per-tensor means.  The list is given as host arrays of n_pairs fp32 device
 * pointers (4-byte aligned: an entry may start anywhere inside a larger tensor) and element counts (each >= 1); a launch covers
 * up to st_gan_loss_max_pairs() entries, whose table travels as a kernel argument, and a block sums st_gan_loss_chunk() elements.
 * Every sum is fp64 in one fixed order without atomics: an entry's mean is the same bits alone, at any list position and at any
 * address, and two runs agree bit for bit.
 *   out     : 1 + n_pairs floats (device).  out[0] = the loss, out[1 + i] = the mean of entry i.
 *   scratch : st_gan_loss_scratch_bytes(numels, n_pairs) bytes (device, 8-byte aligned), not needed after the call; the function
 *             returns a negative ST_ERR_* for a bad list.  scratch_bytes: what the caller provides.
 * st_feature_loss_forward (:37-43): out[1 + i] = mean|real_i - fake_i|, out[0] = 2 sum_i out[1 + i].
 * st_lsgan_loss_forward, by mode: ST_LSGAN_REAL mean((1 - x_i)^2) (generator_loss, :58-66); ST_LSGAN_FAKE mean(x_i^2);
 *   ST_LSGAN_REAL_FAKE the first for the even entries and the second for the odd ones, for discriminator_loss's (:45-56) list
 *   r_0, g_0, r_1, g_1, ...;  out[0] = sum_i out[1 + i].
 * Backward, elementwise from the same inputs; grad_loss: device scalar (d / d out[0]), read on the device:
 *   st_feature_loss_backward: grad_fake_i = -grad_loss 2 / numel_i sign(real_i - fake_i), grad_real_i = -grad_fake_i (sign(0) = 0);
 *     each entry of grad_real / grad_fake may be NULL (that tensor gets no gradient).
 *   st_lsgan_loss_backward: grad_x_i = grad_loss 2 (x_i - 1) / numel_i, or grad_loss 2 x_i / numel_i; entries may be NULL.
 * A null array or required pointer, n_pairs < 0, a count < 1, a misaligned pointer, an unknown mode or a scratch that is too small
 * is ST_ERR_INVALID before anything touches the device.  n_pairs == 0 writes out[0] = 0. */
enum { ST_LSGAN_REAL = 0, ST_LSGAN_FAKE = 1, ST_LSGAN_REAL_FAKE = 2 };
int st_gan_loss_chunk(void);
int st_gan_loss_max_pairs(void);
int64_t st_gan_loss_scratch_bytes(const int64_t* numels, int n_pairs);
int st_feature_loss_forward(const void* const* real, const void* const* fake, const int64_t* numels, int n_pairs, float* out,
                            void* scratch, int64_t scratch_bytes, void* stream);
int st_feature_loss_backward(const void* const* real, const void* const* fake, const int64_t* numels, int n_pairs,
                             const float* grad_loss, void* const* grad_real, void* const* grad_fake, void* stream);
int st_lsgan_loss_forward(const void* const* x, const int64_t* numels, int n_pairs, int mode, float* out, void* scratch,
                          int64_t scratch_bytes, void* stream);
int st_lsgan_loss_backward(const void* const* x, const int64_t* numels, int n_pairs, int mode, const float* grad_loss,
                           void* const* grad_x, void* stream);

/* ---- the optimizer step of both training loops (torch.optim.AdamW, torch.nn.utils.clip_grad_norm_), stateless -------------- */
/* Each call works on a LIST of fp32 tensors, given as host arrays of n device pointers (4-byte aligned: an entry may start
 * anywhere inside a flat buffer) and element counts (each >= 1).  A launch covers up to st_optim_max_tensors() entries, whose
 * table travels as a kernel argument, and a block works on st_optim_chunk() elements of one entry; longer lists run as several
 * launches inside the one call.  No device allocation, no copy, no host synchronisation.
 * st_adamw_step: the decoupled-weight-decay Adam update (non-amsgrad, non-maximize), per element in fp32, each operation rounded
 *   once:  p *= 1 - lr wd;  m += (g - m)(1 - beta1);  v = v beta2 + (1 - beta2) g g;  p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
 *   with step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) evaluated in double per tensor.  steps: n int64
 *   step numbers, ALREADY incremented (each >= 1).  An element's new p, m, v are the same bits alone, at any list position and at
 *   any address (16-byte accesses where an entry's four pointers are 16-byte aligned, 4-byte ones otherwise).
 * st_grad_norm: total_norm_out[0] (device float) = (float)sqrt(sum of squares over the list), squares and sums in fp64 in one
 *   fixed order without atomics: two runs agree bit for bit and an entry's contribution does not change with its address.
 *   scratch: st_grad_norm_scratch_bytes(numels, n) bytes (device, 8-byte aligned), not needed after the call; that function
 *   returns a negative ST_ERR_* for a bad list.  n == 0 writes 0.
 * st_grad_clip: every gradient times coef = min(max_norm / (total_norm[0] + 1e-6f), 1.0f), formed in fp32 on the device
 *   (total_norm: device float, e.g. st_grad_norm's).  A coef of exactly 1.0f loads and stores nothing; a NaN coef multiplies.
 * A null array or required pointer, n < 0, a count < 1, a pointer that is not 4-byte aligned, a step < 1 or a scratch that is
 * too small is ST_ERR_INVALID before anything touches the device. */
int st_optim_chunk(void);
int st_optim_max_tensors(void);
int64_t st_grad_norm_scratch_bytes(const int64_t* numels, int n);
int st_grad_norm(const void* const* grads, const int64_t* numels, int n, float* total_norm_out, void* scratch, int64_t scratch_bytes,
                 void* stream);
int st_grad_clip(void* const* grads, const int64_t* numels, int n, const float* total_norm, float max_norm, void* stream);
int st_adamw_step(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numels,
                  const int64_t* steps, int n, double lr, double beta1, double beta2, double eps, double weight_decay, void* stream);

/* ---- sinc resampling (torchaudio.functional.resample's polyphase filter over a list of waveforms), stateless ---------------- */
/* x, y: host arrays of n device pointers (fp32, 4-byte aligned: an entry may start anywhere inside a flat buffer), in_len and
 * out_len their lengths in samples, out_len[b] == ceil(new_ * in_len[b] / orig).  orig and new_ are the two rates divided by
 * their greatest common divisor.  The filter is the caller's COMPACT table, on the device: of phase i (0 <= i < new_) only the
 * taps inside the window, first[i] the signed offset of its first tap from j * orig, padded with zero taps to the longest
 * phase's S and stored tap-major, taps[s * new_ + i].  Output sample q = j * new_ + i is
 *     y[q] = sum over s = 0 .. S-1, ascending, of taps[s * new_ + i] * x[j * orig + first[i] + s]
 * in fp32, one fused multiply-add per tap; a tap whose input index is outside [0, in_len) contributes exactly zero and is never
 * read.  A sample's bits depend on its own inputs alone: not on the entry's position in the list, its address or alignment,
 * its neighbours, or the launch it landed in.  A launch covers up to st_resample_max_tensors() non-empty entries, whose table
 * travels as a kernel argument, and a block produces st_resample_chunk() consecutive output samples of one entry; longer
 * lists run as several launches inside the one call.  No device allocation, no copy, no host synchronisation, no atomics.
 * n == 0 launches nothing, and so does an entry of length 0 (its two pointers are not looked at).
 * A null array, table or pointer of a non-empty entry, n < 0, orig, new_ or S < 1, a negative length, an out_len other than
 * the one above or a pointer that is not 4-byte aligned is ST_ERR_INVALID, and new_ * S > 2^22 ST_ERR_UNSUPPORTED, for any
 * entry of the list before anything touches the device. */
int st_resample_chunk(void);
int st_resample_max_tensors(void);
int st_resample(const void* const* x, void* const* y, const int64_t* in_len, const int64_t* out_len, int n, int orig, int new_,
                const float* taps, const int32_t* first, int S, void* stream);

/* ---- MelStyleEncoder and DurationPredictor: stages 1 and 3 of StableTTS.synthesise (models/model.py:79-81) ------- */
/* Both run in fp32 (fp32-input MFMA for every convolution and linear): the durations they feed are ceil()ed
 * (model.py:83-84), so a 16-bit logw error would add or drop whole frames.  Inference only (eval mode: no dropout). */

/* Replaces MelStyleEncoder.__init__ (models/reference_encoder.py:25-62) as StableTTS builds it (model.py:38). */
typedef struct st_style_encoder_config {
    int32_t n_mel_channels;    /* in_dim */
    int32_t style_hidden;      /* hidden_dim; native kernels: style_head * 64 */
    int32_t style_vector_dim;  /* out_dim = gin_channels */
    int32_t style_kernel_size; /* Conv1dGLU kernel; native kernels: 1, 3 or 5 */
    int32_t style_head;        /* heads of slf_attn; native kernels: head_dim style_hidden / style_head == 64 */
} st_style_encoder_config;

/* The handle takes MelStyleEncoder.state_dict() under the reference names ("spectral.0.weight", "spectral.3.bias",
 * "temporal.<i>.conv1.weight", "slf_attn.in_proj_weight", "slf_attn.out_proj.bias", "fc.weight", ...) through
 * st_load_param / st_finalize and is destroyed with st_destroy.  Entry points of the other kinds reject it and vice versa. */
int st_create_style_encoder(const st_style_encoder_config* cfg, int device, st_engine** out);

/* Replaces MelStyleEncoder.forward(x, x_mask) (reference_encoder.py:74-93) in eval mode.
 *   mel   : (B, n_mel_channels, T) fp32 reference mel spectrogram
 *   mask  : (B, 1, T) fp32 frame mask, or NULL (synthesise passes None, model.py:79).  Frames with mask == 0 are left out
 *           of the attention keys (key_padding_mask) and of the temporal mean; like the reference, the convolutions see
 *           them unmasked.  An item without any valid frame yields NaN in c_out, as the reference's 0 / 0 does.
 *   c_out : (B, style_vector_dim) fp32 style vectors                                  -- all device pointers
 * Enqueued on `stream`; the host is not synchronised. */
int st_style_encoder_forward(st_engine* e, const float* mel, const float* mask, float* c_out, int B, int T, void* stream);

/* Replaces DurationPredictor.__init__ (models/duration_predictor.py:6-22) as StableTTS builds it (model.py:39). */
typedef struct st_duration_predictor_config {
    int32_t in_channels;       /* hidden_channels of the text encoder */
    int32_t filter_channels;   /* native kernels: a multiple of 128 */
    int32_t kernel_size;       /* native kernels: 1, 3 or 5 */
    int32_t gin_channels;      /* width of g */
} st_duration_predictor_config;

/* The handle takes DurationPredictor.state_dict() under the reference names ("conv1.weight", "norm1.weight", "conv2.bias",
 * "norm2.bias", "proj.weight", "cond.weight", "cond.bias", ...) through st_load_param / st_finalize and is destroyed with
 * st_destroy.  Entry points of the other kinds reject it and vice versa. */
int st_create_duration_predictor(const st_duration_predictor_config* cfg, int device, st_engine** out);

/* Replaces DurationPredictor.forward(x, x_mask, g) (duration_predictor.py:24-37) in eval mode.
 *   x        : (B, in_channels, Tx) fp32 text-encoder states (st_text_encoder_forward's x_out)
 *   x_mask   : (B, 1, Tx) fp32 token mask (st_text_encoder_forward's mask_out); multiplied in where the reference does
 *   g        : (B, gin_channels) fp32 speaker vectors (st_style_encoder_forward's c_out)
 *   logw_out : (B, 1, Tx) fp32 log-durations, exactly 0 where x_mask is 0              -- all device pointers
 * Enqueued on `stream`; the host is not synchronised. */
int st_duration_predictor_forward(st_engine* e, const float* x, const float* x_mask, const float* g, float* logw_out,
                                  int B, int Tx, void* stream);

/* ---- style-encoder / duration-predictor training: autograd counterparts of the two forwards above, fp32 like them.
 * The *_train_forward calls compute what the inference forwards compute (bit for bit when p_dropout == 0) and keep the
 * activations of this ONE call in the engine (buffers that grow on demand, then are reused; the inputs are copied in).
 * Train-mode dropout is counter-based with the hash and seed words of st_train_forward and the salts
 *     style encoder: 64 spectral.2, 65 spectral.5, 66 temporal.0, 67 temporal.1 (the GLU product, before the residual add),
 *                    68 the attention probabilities;      duration predictor: 72 after norm1, 73 after norm2;
 * the backward re-evaluates the masks.  st_train_serial reports the forward held (0: none; a re-bind / st_finalize drops it).
 * The backward takes d loss / d c (B, style_vector_dim) resp. d loss / d logw (B, 1, Tx) and writes EVERY parameter gradient
 * into grad_flat: st_train_grad_numel() floats in the layout of st_train_grad_offset (parameter-name order, 64-byte aligned
 * slices; the gaps are not written).  Neither module has an input gradient (the reference detaches x and g, duration_predictor.py
 * :25-26; the mel is data).  (serial, B, T) must be those of the held forward (ST_ERR_STATE otherwise).  No atomics: the
 * gradients are bitwise repeatable. */
int st_style_encoder_train_forward(st_engine* e, const float* mel, const float* mask, float* c_out, int B, int T,
                                   float p_dropout, uint64_t seed, void* stream);
int st_style_encoder_train_backward(st_engine* e, int64_t serial, int B, int T, const float* grad_c, float* grad_flat, void* stream);
int st_duration_predictor_train_forward(st_engine* e, const float* x, const float* x_mask, const float* g, float* logw_out,
                                        int B, int Tx, float p_dropout, uint64_t seed, void* stream);
int st_duration_predictor_train_backward(st_engine* e, int64_t serial, int B, int Tx, const float* grad_logw, float* grad_flat,
                                         void* stream);

/* ---- feature front end: waveform -> (log-mel) spectrogram (utils/audio.py:6-52) ----------------------------------- */
/* fp32 throughout: reflect padding by index arithmetic, the window, a real FFT of length n_fft (one complex FFT of n_fft / 2
 * plus a split pass), sqrt(re^2 + im^2 + 1e-6), the banded mel projection and log(clamp(x, 1e-5)).  No atomics: the output is
 * bitwise repeatable and an utterance's values do not depend on the rest of the batch.  The backward of a padded batch
 * (st_mel_backward) recomputes the forward and writes the waveform's gradient. */

enum { ST_PAD_REFLECT = 0, ST_PAD_CONSTANT = 1, ST_PAD_REPLICATE = 2, ST_PAD_CIRCULAR = 3 };   /* F.pad modes */
enum { ST_MEL_LOG = 0, ST_MEL_LINEAR = 1 };   /* output of st_mel_forward_ragged: log-mel, or the linear magnitude */

/* Replaces LogMelSpectrogram.__init__ / LinearSpectrogram.__init__ (utils/audio.py:7-17,30-45).  sample_rate, f_min,
 * f_max and mel_scale only shape the filter bank, which the caller loads. */
typedef struct st_mel_config {
    int32_t n_fft;        /* native kernels: a power of two in [32, 2048] */
    int32_t win_length;   /* native kernels: == n_fft */
    int32_t hop_length;   /* 1 .. n_fft */
    int32_t pad;          /* reflect padding on both sides, >= 0 */
    int32_t n_mels;       /* >= 1; 0 makes a linear-spectrogram extractor, which has no filter bank */
    int32_t center;       /* native kernels: 0 (config.py: center=False) */
    int32_t pad_mode;     /* native kernels: ST_PAD_REFLECT */
} st_mel_config;

/* The handle takes "spectrogram.window" (win_length) and, when n_mels > 0, "mel_scale.fb" (n_fft / 2 + 1, n_mels) through
 * st_load_param / st_finalize; st_finalize derives each filter's nonzero bin range from the loaded fb.  Unsupported
 * configurations return ST_ERR_UNSUPPORTED and invalid ones ST_ERR_INVALID before any device is touched.  Entry points of the
 * other kinds reject this handle and vice versa.  Destroyed with st_destroy. */
int st_create_mel_extractor(const st_mel_config* cfg, int device, st_engine** out);

/* Frames of an utterance of L samples: 1 + (L + 2 pad - n_fft) / hop.  ST_ERR_INVALID when L <= pad (reflect padding needs
 * pad < L) or L + 2 pad < n_fft (no frame), where the reference's F.pad / torch.stft raise. */
int64_t st_mel_frames(const st_engine* e, int64_t L);

/* Replaces LogMelSpectrogram.forward (utils/audio.py:50-52) on a padded batch:  wave (B, L) -> out (B, n_mels, frames), fp32
 * device pointers.  Enqueued on `stream`; the host is not synchronised. */
int st_mel_forward(st_engine* e, const float* wave, int B, int64_t L, float* out, void* stream);

/* The ragged form, in one launch.  Utterance b is wave[sample_offsets[b] .. sample_offsets[b + 1]) and its result is the
 * (rows, frames_b) block at out + rows * frame_offsets[b], where rows = n_mels (ST_MEL_LOG) or n_fft / 2 + 1 (ST_MEL_LINEAR:
 * the magnitude of LinearSpectrogram.forward, :19-26) and frames_b = frame_offsets[b + 1] - frame_offsets[b] must equal
 * st_mel_frames(e, L_b).  Both offset arrays have B + 1 entries in HOST memory; wave and out are device pointers. */
int st_mel_forward_ragged(st_engine* e, const float* wave, const int64_t* sample_offsets, const int64_t* frame_offsets, int B,
                          int output, float* out, void* stream);

/* Backward of st_mel_forward (output ST_MEL_LOG) or of the linear spectrogram (ST_MEL_LINEAR) on a padded batch, for the Vocos
 * multi-scale mel loss (vocoders/vocos/models/loss.py):  wave (B, L) and grad_out, the gradient of the output ((B, n_mels, frames)
 * or (B, n_fft / 2 + 1, frames)) -> grad_wave (B, L), overwritten; fp32 device pointers.  The spectrum and the mel sums are
 * recomputed exactly as the forward computes them, so torch.clamp's mask (mel >= 1e-5) is the forward's.  workspace is a
 * caller-owned device buffer of st_mel_backward_workspace_bytes(e, B, L) bytes; no state is kept between calls.  No atomics: the
 * result is bitwise repeatable.  Validates every argument before touching the device (the checks of st_mel_forward); a log-mel
 * backward needs n_mels <= 2 n_fft (ST_ERR_UNSUPPORTED otherwise).  The window and the filter bank get no gradient. */
int64_t st_mel_backward_workspace_bytes(const st_engine* e, int B, int64_t L);
int st_mel_backward(st_engine* e, const float* wave, const float* grad_out, int B, int64_t L, int output, float* grad_wave,
                    void* workspace, void* stream);

/* ---- training: autograd counterpart of Decoder.forward ------------------------------------------- */

/* Replaces Decoder.forward(t, x, mask, mu, c) UNDER AUTOGRAD as CFMDecoder.compute_loss calls it (models/flow_matching.py:99,
 * train.py:78-81): one vector-field evaluation with a per-item t (B values) that keeps every activation the backward
 * pass needs in the engine.  Train-mode dropout of the reference (p_dropout on the FFN activations and on the attention
 * probabilities, models/diffusion_transformer.py:22,52,77) is counter-based: the same (seed, element) hash is
 * re-evaluated by the backward kernels, nothing is stored.  Pointers as for st_estimator_forward. */
int st_train_forward(st_engine* e, const float* t, const float* x, const float* mu, const float* mask, const float* c,
                     float* out, int B, int T, float p_dropout, uint64_t seed, void* stream);

/* Serial number of the st_train_forward (or of the text-encoder / style-encoder / duration-predictor training forward, on
 * those handles) whose activations the engine holds now (monotonically increasing from 1;
 * 0 = none: never run, or invalidated by a parameter update).  The engine keeps the activations of ONE forward. */
int64_t st_train_serial(const st_engine* e);

/* Replaces torch.autograd's backward of that call.  grad_out: d loss / d out (B, n_feats, T).  Writes d loss / d x,
 * d loss / d mu (B, n_feats, T) and d loss / d c (B, gin) where the pointer is not NULL, and the gradient of every
 * parameter into engine-owned fp32 buffers in the reference shapes (fetch with st_param_grad).
 * `serial`, B, T identify the forward this is the backward OF (st_train_serial right after that st_train_forward):
 * if another forward has replaced its activations, or the parameters were re-packed, or the shape differs, the
 * call fails with ST_ERR_STATE before touching any caller memory. */
int st_train_backward(st_engine* e, int64_t serial, int B, int T, const float* grad_out, float* grad_x, float* grad_mu,
                      float* grad_c, void* stream);

/* The same backward in three PARTS, so that a data-parallel wrapper (DDP, train.py:49-51) can reduce the gradients of finished
 * layers while the remaining ones are still being computed -- torch's autograd delivers them layer by layer, a single native call
 * would deliver all 116 at once:
 *     part 0: final_proj, blocks L-1 .. L/2, the long-skip convs      part 1: blocks L/2-1 .. 0
 *     part 2: in_proj, the cond prenet, the time MLP; writes d x, d mu, d c (grad_x / grad_mu / grad_c, each may be NULL)
 * st_train_param_part(name) says which part finishes a parameter's gradient.  Parts run in order 0, 1, 2 (ST_ERR_STATE otherwise);
 * grad_out is read by part 0 only.  grad_flat (part 0; may be NULL = the engine's own buffers, fetch with st_param_grad): a
 * caller-owned device buffer of st_train_grad_numel() floats that receives EVERY parameter gradient of this backward directly
 * -- no staging copy -- at st_train_grad_offset(name) (reference shape, 64-byte aligned slices, st_param_info's order); it must stay
 * valid until part 2 has run.  The legacy call above = the three parts with the engine's own buffers. */
int st_train_backward_part(st_engine* e, int64_t serial, int B, int T, int part, const float* grad_out, float* grad_flat,
                           int64_t grad_numel, float* grad_x, float* grad_mu, float* grad_c, void* stream);
int st_train_param_part(const st_engine* e, const char* name);        /* 0, 1, 2; < 0: unknown name */
int64_t st_train_grad_offset(const st_engine* e, const char* name);   /* element offset in the flat gradient layout; < 0: unknown */
int64_t st_train_grad_numel(const st_engine* e);                      /* floats of the flat layout (alignment gaps included) */

/* ---- text-encoder training: autograd counterpart of TextEncoder.forward (models/text_encoder.py:34-44) on a handle of
 * st_create_text_encoder.  The forward is st_text_encoder_forward that keeps the activations (same outputs, same dropout
 * scheme as st_train_forward: FFN site 2i, attention site 2i + 1 of block i); st_train_serial applies to it.
 * The backward takes d loss / d x (B, hidden, T) and / or d loss / d mu_x (B, out, T) -- either may be NULL, not both --
 * and writes EVERY parameter gradient (emb.weight, every block, proj) into grad_flat: st_train_grad_numel() floats in the
 * layout of st_train_grad_offset (NULL = the engine's own buffers, fetch with st_param_grad), and d loss / d c (B, gin) into
 * grad_c unless NULL.  Rows of emb.weight that no valid position reads get exact zeros; the result is bitwise repeatable.
 * A backward whose serial is not that of the forward the engine holds fails with ST_ERR_STATE.  st_train_param_part reports
 * part 0 for every text-encoder parameter (one part). */
int st_text_encoder_train_forward(st_engine* e, const int64_t* tokens, const int64_t* lengths, const float* c,
                                  float* x_out, float* mu_out, float* mask_out, int B, int T,
                                  float p_dropout, uint64_t seed, void* stream);
int st_text_encoder_train_backward(st_engine* e, int64_t serial, int B, int T, const float* grad_x /* nullable */,
                                   const float* grad_mu /* nullable */, float* grad_flat, float* grad_c /* nullable */,
                                   void* stream);

/* Copies the gradient of one parameter (reference state_dict name, `numel` fp32 values) to the device pointer dst. */
int st_param_grad(st_engine* e, const char* name, float* dst, int64_t numel, void* stream);

/* All parameter gradients in ONE copy: dst receives the flat layout described above (`numel` = st_train_grad_numel()). */
int st_param_grads_flat(st_engine* e, float* dst, int64_t numel, void* stream);

/* Non-finite guard (no reference analogue: the reference is fp32).  The kernel that writes the output of st_estimator_forward /
 * st_cfm_solve raises a flag when a value is NaN / Inf -- f16 MFMA operands overflow at 65504 (a checkpoint whose activations
 * exceed that needs operand_dtype = bf16), or the inputs were bad.  Synchronises `stream`, stores the flag of the calls completed
 * since the last query in *nonfinite (0 / 1) and clears it; after a flagged call the engine re-zeroes its workspace by itself. */
int st_output_status(st_engine* e, void* stream, int* nonfinite);

/* Function evaluations, attempted steps and rejected steps of the last st_cfm_solve (adaptive solvers vary). */
int st_last_solve_stats(const st_engine* e, int64_t* nfe, int64_t* steps, int64_t* rejects);

/* Engine options by name (no reference analogue: models/diffusion_transformer.py:70-77 computes the attention in fp32).
 *   "attention_precision"  0 (default): q, k, v enter the attention MFMAs as 16-bit operands.
 *                          1: q and k as hi + lo PAIRS of 16-bit operands, scores = q_hi k_hi + q_lo k_hi + q_hi k_lo (3x the QK^T
 *                             MFMAs) in st_estimator_forward / st_cfm_solve -- for checkpoints whose softmax has become an arg-max
 *                             (score maxima of 80-200), where the 2^-11 rounding of q and k moves the winning probability and
 *                             f16 operands miss the 1e-3 parity bar.  Takes effect at the next call.
 *   "fused_ffn"            read-only: 0 two-kernel FFN, 1 fused direct kernel (default), 3 fused Winograd kernel (ST_FUSED_FFN=3).
 * st_get_option returns ST_ERR_INVALID for an unknown name. */
int st_set_option(st_engine* e, const char* name, int value);
int st_get_option(const st_engine* e, const char* name, int* value);

/* Largest log-sum-exp (natural-log units; of the scaled, masked scores of softmax(q k^T / sqrt(d) + mask), diffusion_transformer.py:77)
 * over every valid attention row of the estimator evaluations completed on `stream` since the last query; -inf if there were none.  A
 * row's score maximum lies within log(T) below it, so this is the run-time sign of the arg-max regime above: seeded / freshly
 * initialised weights give ~10, values beyond ~50 mean "attention_precision" = 1 is needed for 1e-3 parity.  Synchronises `stream`,
 * reads 16 words, resets the statistic.  Costs one atomic per attention block while running. */
int st_attention_stats(st_engine* e, void* stream, float* max_lse);

/* ---- measurement / test hooks (no reference analogue) ------------------------------------- */

/* Copies a named internal tensor of the LAST st_estimator_forward call to `host_out` as fp32 in
 * the engine's time-major layout; returns the element count, or <0.  If host_out is
 * NULL only the count is returned.  Synchronises the device.  Names: "cond", "h0", "b<i>.x1",
 * "b<i>.h1", "b<i>.q", "b<i>.k", "b<i>.vt", "b<i>.attn", "b<i>.x2", "b<i>.h2", "b<i>.u",
 * "b<i>.x3", "lsc<j>", "v".  Capture must be enabled first (it snapshots after every stage). */
int st_debug_capture(st_engine* e, int enable);
int64_t st_debug_fetch(st_engine* e, const char* name, float* host_out, int64_t capacity);

/* Per-kernel-class timing with HIP events recorded on the launch stream.  Classes are listed by
 * st_profile_class_name(i), i in [0, st_profile_num_classes()).  st_profile_read synchronises,
 * returns launches and total milliseconds per class since the last reset, and resets. */
int st_profile_enable(st_engine* e, int enable);
/* Restrict event recording to the classes whose bit is set in class_mask (default: all). */
int st_profile_select(st_engine* e, uint64_t class_mask);
/* Record events around every stride-th launch of a selected class only (default 1 = every launch).  An event
 * pair costs ~10 us of idle stream time on MI355X, so a timed run samples: st_profile_read then reports the
 * SAMPLED launches and their total, i.e. total_ms / launches is still the mean launch duration. */
int st_profile_stride(st_engine* e, int stride);
int st_profile_num_classes(void);
const char* st_profile_class_name(int cls);
int st_profile_read(st_engine* e, int cls, int64_t* launches, double* total_ms, double* flops_per_launch);

/* Bytes of device memory currently held by the engine (weights + workspace). */
int64_t st_device_bytes(const st_engine* e);

#ifdef __cplusplus
}
#endif
#endif /* STABLETTS_HIP_H */
