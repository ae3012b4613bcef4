// Launcher interface of the monotonic alignment search kernels (mas_kernels.hip).
// Reference: monotonic_align/core.py:14-46 (maximum_path_jit) and models/model.py:150-155 (neg_cent with s_p_sq_r = 1).
// The DP is fp32 adds and compares with integer output, so it is reproduced bit for bit; the file is compiled without
// contraction (build.py EXTRA_FLAGS) and uses no fast-math.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace st {

constexpr int kMasMaxTx = 4096;                 // widest row the register plan holds: 64 fp32 columns per lane
constexpr size_t kMasLdsBudget = 64 * 1024;     // decision bits of one utterance go to LDS up to this size, else to global

// Bytes of global workspace st_maximum_path needs: 0 when one utterance's decision bits (Ty x ceil(Tx/64) x 8 B) fit
// the LDS budget, else B times that.
size_t mas_workspace_bytes(int B, int Ty, int Tx);

// maximum_path_jit for every item: neg_cent (B, Ty, Tx) fp32 (read only), t_y / t_x (B) int32 (clamped to [0, Ty] /
// [0, Tx]); path (B, Ty, Tx) fp32 0/1, every cell written; durations (B, Tx) int32 frames per token, optional.
// Items with t_x == 0 or t_y == 0 get an all-zero path.  workspace: mas_workspace_bytes(B, Ty, Tx) bytes (or null if 0).
// Returns hipErrorInvalidValue for a shape the kernels do not cover (Tx > kMasMaxTx).
hipError_t launch_mas_path(const float* neg_cent, const int32_t* t_y, const int32_t* t_x, int B, int Ty, int Tx, float* path,
                           int32_t* durations, void* workspace, hipStream_t s);

// neg_cent[b][t][s] = D (-1/2 log 2 pi) - 1/2 sum_d y[b][d][t]^2 + sum_d y[b][d][t] mu_x[b][d][s] - 1/2 sum_d mu_x[b][d][s]^2
// mu_x (B, D, Tx), y (B, D, Ty), neg_cent (B, Ty, Tx); the cross term on the fp32-input MFMA.
hipError_t launch_mas_neg_cent(const float* mu_x, const float* y, int B, int D, int Tx, int Ty, float* neg_cent, hipStream_t s);

}  // namespace st
