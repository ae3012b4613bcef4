// The optimizer step behind the C ABI (st_adamw_step / st_grad_norm / st_grad_clip / st_grad_norm_scratch_bytes): stateless
// helpers like the GAN losses (errors through st_last_error(NULL)).  The host arrays of device pointers and element counts are
// cut into launch groups of kOptimMaxTensors entries whose table is a kernel argument; every argument is checked before anything
// touches the device.  The kernels are in optim_kernels.hip.
#include "engine_internal.h"
#include "optim_launch.h"

#include <limits.h>
#include <math.h>

using namespace st;
using namespace sthost;

namespace {

int optim_fail(int code, const char* msg) { g_create_error = msg; return code; }

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

// counts of a list: ST_OK, or the error of the first bad entry.  *chunks: the sum of the entries' chunk counts.
int check_counts(const int64_t* numels, int n, long long* chunks) {
    if (n < 0) return optim_fail(ST_ERR_INVALID, "n must be >= 0");
    if (n > 0 && !numels) return optim_fail(ST_ERR_INVALID, "null argument");
    long long total = 0;
    for (int g = 0; g < n; g += kOptimMaxTensors) {
        long long in_group = 0;
        for (int i = g; i < n && i < g + kOptimMaxTensors; ++i) {
            if (numels[i] < 1) return optim_fail(ST_ERR_INVALID, "every element count must be >= 1");
            in_group += optim_chunks(numels[i]);
            if (in_group > INT_MAX) return optim_fail(ST_ERR_INVALID, "element counts out of range (one launch group exceeds 2^31 chunks)");
        }
        total += in_group;
    }
    *chunks = total;
    return ST_OK;
}

int check_pointers(const void* const* a, int n) {
    if (n > 0 && !a) return optim_fail(ST_ERR_INVALID, "null argument");
    for (int i = 0; i < n; ++i) {
        if (!a[i]) return optim_fail(ST_ERR_INVALID, "null tensor pointer");
        if (misaligned(a[i])) return optim_fail(ST_ERR_INVALID, "tensor pointers must be 4-byte aligned");
    }
    return ST_OK;
}

// the table of launch group [g, g + m) of a gradient list -> its block count
int fill_grad_table(GradTable& tab, void* const* grads, const int64_t* numels, int g, int m) {
    int blocks = 0;
    for (int i = 0; i < m; ++i) {
        tab.e[i] = GradEntry{(float*)grads[g + i], (long long)numels[g + i], blocks, 0};
        blocks += (int)optim_chunks(numels[g + i]);
    }
    return blocks;
}

}  // namespace

extern "C" {

int st_optim_chunk(void) { return kOptimChunk; }
int st_optim_max_tensors(void) { return kOptimMaxTensors; }

int64_t st_grad_norm_scratch_bytes(const int64_t* numels, int n) {
    long long chunks = 0;
    if (int rc = check_counts(numels, n, &chunks)) return rc;
    return 8ll * chunks;
}

int st_grad_norm(const void* const* grads, const int64_t* numels, int n, float* total_norm_out, void* scratch, int64_t scratch_bytes,
                 void* stream) {
    long long chunks = 0;
    if (int rc = check_counts(numels, n, &chunks)) return rc;
    if (int rc = check_pointers(grads, n)) return rc;
    if (!total_norm_out) return optim_fail(ST_ERR_INVALID, "null tensor pointer");
    if (misaligned(total_norm_out)) return optim_fail(ST_ERR_INVALID, "tensor pointers must be 4-byte aligned");
    if (chunks > 0 && (!scratch || ((uintptr_t)scratch & 7))) return optim_fail(ST_ERR_INVALID, "scratch must be a non-null, 8-byte aligned device pointer");
    if (scratch_bytes < 8ll * chunks) return optim_fail(ST_ERR_INVALID, "scratch is smaller than st_grad_norm_scratch_bytes() of this list");
    double* partials = (double*)scratch;
    hipStream_t s = (hipStream_t)stream;
    for (int g = 0; g < n; g += kOptimMaxTensors) {
        const int m = n - g < kOptimMaxTensors ? n - g : kOptimMaxTensors;
        GradTable tab{};
        const int blocks = fill_grad_table(tab, (void* const*)grads, numels, g, m);
        if (launch_grad_sumsq(tab, m, blocks, partials, s) != hipSuccess) return optim_fail(ST_ERR_HIP, "grad_sumsq kernel launch failed");
        partials += blocks;
    }
    if (launch_grad_norm_finish((const double*)scratch, chunks, total_norm_out, s) != hipSuccess)
        return optim_fail(ST_ERR_HIP, "grad_norm_finish kernel launch failed");
    return ST_OK;
}

int st_grad_clip(void* const* grads, const int64_t* numels, int n, const float* total_norm, float max_norm, void* stream) {
    long long chunks = 0;
    if (int rc = check_counts(numels, n, &chunks)) return rc;
    if (int rc = check_pointers(grads, n)) return rc;
    if (!total_norm) return optim_fail(ST_ERR_INVALID, "null tensor pointer");
    if (misaligned(total_norm)) return optim_fail(ST_ERR_INVALID, "tensor pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    for (int g = 0; g < n; g += kOptimMaxTensors) {
        const int m = n - g < kOptimMaxTensors ? n - g : kOptimMaxTensors;
        GradTable tab{};
        const int blocks = fill_grad_table(tab, grads, numels, g, m);
        if (launch_grad_clip(tab, m, blocks, total_norm, max_norm, s) != hipSuccess) return optim_fail(ST_ERR_HIP, "grad_clip kernel launch failed");
    }
    return ST_OK;
}

int st_adamw_step(void* const* params, const void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numels,
                  const int64_t* steps, int n, double lr, double beta1, double beta2, double eps, double weight_decay, void* stream) {
    long long chunks = 0;
    if (int rc = check_counts(numels, n, &chunks)) return rc;
    if (int rc = check_pointers(params, n)) return rc;
    if (int rc = check_pointers(grads, n)) return rc;
    if (int rc = check_pointers(exp_avg, n)) return rc;
    if (int rc = check_pointers(exp_avg_sq, n)) return rc;
    if (n > 0 && !steps) return optim_fail(ST_ERR_INVALID, "null argument");
    for (int i = 0; i < n; ++i)
        if (steps[i] < 1) return optim_fail(ST_ERR_INVALID, "every step must be >= 1 (the step numbers are already incremented)");
    const AdamwScalars sc{(float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps};
    hipStream_t s = (hipStream_t)stream;
    for (int g = 0; g < n; g += kOptimMaxTensors) {
        const int m = n - g < kOptimMaxTensors ? n - g : kOptimMaxTensors;
        AdamwTable tab{};
        int blocks = 0;
        for (int i = 0; i < m; ++i) {
            const double step = (double)steps[g + i];
            const double step_size = lr / (1.0 - pow(beta1, step)), bc2_sqrt = sqrt(1.0 - pow(beta2, step));
            tab.e[i] = AdamwEntry{(float*)params[g + i], (const float*)grads[g + i], (float*)exp_avg[g + i], (float*)exp_avg_sq[g + i],
                                  (long long)numels[g + i], blocks, (float)step_size, (float)bc2_sqrt, 0};
            blocks += (int)optim_chunks(numels[g + i]);
        }
        if (launch_adamw_step(tab, m, blocks, sc, s) != hipSuccess) return optim_fail(ST_ERR_HIP, "adamw_step kernel launch failed");
    }
    return ST_OK;
}

}  // extern "C"
