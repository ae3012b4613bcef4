// Block-wide fp64 sum in one fixed order, shared by the kernels whose sums decide a loss or a gradient
// (align_train_kernels.hip, gan_loss_kernels.hip): no atomics, the same tree every time.
#pragma once
#include <hip/hip_runtime.h>

namespace st {

// sum of v over the 256 threads of the block, same tree every time; red: 256 doubles of LDS.  Every thread gets the sum.
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

}  // namespace st
