// Launcher interface of the training side of the alignment step (align_train_kernels.hip): what StableTTS.forward does
// between the alignment search and the decoder, models/model.py:160-176, and duration_loss (duration_predictor.py:38-40).
// The 0/1 alignment has one token per frame and contiguous frames per token, so mu_y = attn^T mu_x is a gather and
// d mu_x a segmented sum over contiguous frame ranges: the kernels take the per-token frame counts and never see a dense
// (B, Ty, Tx) tensor.  fp32 in and out; the segmented sums and the loss reductions accumulate in fp64, in one fixed order
// (no atomics), so results do not depend on the batch, the grid or the neighbouring tokens.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace st {

constexpr int kAlignTrainMaxTx = 4096;      // the running sum of one item's durations lives in LDS (16 KB)
constexpr int kAlignTrainFrames = 256;      // frames per block of the forward
constexpr int kAlignTrainChannels = 16;     // channels per block, forward and backward
constexpr int kDurLossBlocks = 256;         // partial sums of the duration loss

// floats of scratch launch_align_train_forward needs: one partial of the prior sum and one of sum(y_mask) per block, then
// [2 n] = the prior sum and [2 n + 1] = the denominator sum(y_mask) * M (kept for the backward)
int align_train_scratch_floats(int B, int M, int Ty);
// floats of scratch launch_duration_loss needs: kDurLossBlocks partials, then the squared sum and the denominator
constexpr int kDurLossScratchFloats = kDurLossBlocks + 2;

// Frame -> token map from the running sum of durations: a token counts only where x_mask != 0, a negative count is 0, and
// the running sum is clipped to [0, Ty] before it is used, so no count can index outside a buffer.
//   frame_token (B, Ty) int32: the token of each frame, -1 where no token covers it
//   mu_y (B, M, Ty), optional: mu_x[:, :, frame_token], 0 where frame_token < 0                       (model.py:167-168)
//   mu_y_masked (B, M, Ty): mu_y * keep + (1 - keep) * fake_content, keep 0/1 per item; keep == null keeps every item,
//                           fake_content == null is 0                                                   (model.py:172)
//   prior_loss: sum(0.5 ((y - mu_y)^2 + log 2 pi) y_mask) / (sum(y_mask) * M)                           (model.py:175-176)
hipError_t launch_align_train_forward(const int32_t* durations, const float* x_mask, const float* y_mask, const float* mu_x,
                                      const float* y, const float* fake_content, const float* keep, int B, int M, int Tx, int Ty,
                                      int32_t* frame_token, float* mu_y, float* mu_y_masked, float* scratch, float* prior_loss,
                                      hipStream_t s);

// grad_mu_x[b][m][i] = sum over the frames t of token i, ascending, of
//     keep_b g_masked[b][m][t] + g_mu_y[b][m][t] + g_prior y_mask[b][t] (mu_x[b][m][i] - y[b][m][t]) / denom
// (every element written, 0 for a token without frames); grad_fake_content[m] = sum over items with keep == 0 and every
// frame of g_masked.  Each of g_masked, g_mu_y, g_prior may be null (that term is 0); grad_fake_content may be null.
hipError_t launch_align_train_backward(const int32_t* durations, const float* x_mask, const float* y_mask, const float* mu_x,
                                       const float* y, const float* keep, const float* scratch, const float* g_masked,
                                       const float* g_mu_y, const float* g_prior, int B, int M, int Tx, int Ty, float* grad_mu_x,
                                       float* grad_fake_content, hipStream_t s);

// logw_ = log(1e-8 + durations) * x_mask (model.py:162; optional output), loss = sum((logw - logw_)^2) / sum(x_lengths)
// (duration_predictor.py:38-40) over every element; the difference is formed in fp64 (logw close to logw_ cancels)
hipError_t launch_duration_loss(const float* logw, const int32_t* durations, const float* x_mask, const long long* x_lengths,
                                int B, int Tx, float* logw_target, float* scratch, float* loss, hipStream_t s);
// grad_logw = grad_loss[0] * 2 (logw - logw_) / sum(x_lengths)
hipError_t launch_duration_loss_bwd(const float* logw, const int32_t* durations, const float* x_mask, const float* scratch,
                                    const float* grad_loss, int B, int Tx, float* grad_logw, hipStream_t s);

}  // namespace st
