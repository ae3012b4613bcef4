// The scalar GAN losses of a Vocos step behind the C ABI (st_feature_loss_* / st_lsgan_loss_* / st_gan_loss_scratch_bytes):
// stateless helpers like st_align_train_* (errors through st_last_error(NULL)).  The host arrays of device pointers and element
// counts are cut into launch groups of kGanLossMaxPairs entries whose table is a kernel argument; every argument is checked
// before anything touches the device.  The kernels are in gan_loss_kernels.hip.
#include "engine_internal.h"
#include "gan_loss_launch.h"

#include <limits.h>

using namespace st;
using namespace sthost;

namespace {

int gan_fail(int code, const char* msg) { g_create_error = msg; return code; }

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

// counts of a list: ST_OK, or the error of the first bad entry.  *chunks: the sum of the entries' chunk counts.
int check_counts(const int64_t* numels, int n_pairs, long long* chunks) {
    if (n_pairs < 0) return gan_fail(ST_ERR_INVALID, "n_pairs must be >= 0");
    if (n_pairs > 0 && !numels) return gan_fail(ST_ERR_INVALID, "null argument");
    long long total = 0;
    for (int g = 0; g < n_pairs; g += kGanLossMaxPairs) {
        long long in_group = 0;
        for (int i = g; i < n_pairs && i < g + kGanLossMaxPairs; ++i) {
            if (numels[i] < 1) return gan_fail(ST_ERR_INVALID, "every element count must be >= 1");
            in_group += gan_loss_chunks(numels[i]);
            if (in_group > INT_MAX) return gan_fail(ST_ERR_INVALID, "element counts out of range (one launch group exceeds 2^31 chunks)");
        }
        total += in_group;
    }
    *chunks = total;
    return ST_OK;
}

int check_pointers(const void* const* a, const void* const* b, int n_pairs) {
    if (n_pairs > 0 && (!a || !b)) return gan_fail(ST_ERR_INVALID, "null argument");
    for (int i = 0; i < n_pairs; ++i) {
        if (!a[i] || !b[i]) return gan_fail(ST_ERR_INVALID, "null tensor pointer");
        if (misaligned(a[i]) || misaligned(b[i])) return gan_fail(ST_ERR_INVALID, "tensor pointers must be 4-byte aligned");
    }
    return ST_OK;
}

// forward of a list: stages 1 and 2 per launch group in list order, then one stage 3.  b == a for the one-input ops.
int run_forward(int op, float scale, const void* const* a, const void* const* b, const int64_t* numels, int n_pairs, float* out,
                void* scratch, int64_t scratch_bytes, void* stream, const char* what) {
    long long chunks = 0;
    if (int rc = check_counts(numels, n_pairs, &chunks)) return rc;
    if (int rc = check_pointers(a, b, n_pairs)) return rc;
    if (!out) return gan_fail(ST_ERR_INVALID, "null tensor pointer");
    const long long need = 8ll * (chunks + n_pairs);
    if (need > 0 && (!scratch || ((uintptr_t)scratch & 7))) return gan_fail(ST_ERR_INVALID, "scratch must be a non-null, 8-byte aligned device pointer");
    if (scratch_bytes < need) return gan_fail(ST_ERR_INVALID, "scratch is smaller than st_gan_loss_scratch_bytes() of this list");
    double* means64 = (double*)scratch;
    double* partials = means64 + n_pairs;
    hipStream_t s = (hipStream_t)stream;
    for (int g = 0; g < n_pairs; g += kGanLossMaxPairs) {
        const int m = n_pairs - g < kGanLossMaxPairs ? n_pairs - g : kGanLossMaxPairs;
        GanPairTable tab{};
        int blocks = 0;
        for (int i = 0; i < m; ++i) {
            tab.p[i] = GanPair{(const float*)a[g + i], (const float*)b[g + i], (long long)numels[g + i], blocks, 0};
            blocks += (int)gan_loss_chunks(numels[g + i]);
        }
        if (launch_gan_loss_group(op, tab, m, blocks, partials, means64 + g, out + 1 + g, s) != hipSuccess) return gan_fail(ST_ERR_HIP, what);
        partials += blocks;
    }
    if (launch_gan_loss_total(means64, n_pairs, scale, out, s) != hipSuccess) return gan_fail(ST_ERR_HIP, what);
    return ST_OK;
}

int run_backward(int op, const void* const* a, const void* const* b, const int64_t* numels, int n_pairs, const float* grad_loss,
                 void* const* da, void* const* db, void* stream, const char* what) {
    long long chunks = 0;
    if (int rc = check_counts(numels, n_pairs, &chunks)) return rc;
    if (int rc = check_pointers(a, b, n_pairs)) return rc;
    if (!grad_loss || (n_pairs > 0 && !da)) return gan_fail(ST_ERR_INVALID, "null argument");
    for (int i = 0; i < n_pairs; ++i)
        if (misaligned(da[i]) || (db && misaligned(db[i]))) return gan_fail(ST_ERR_INVALID, "tensor pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    for (int g = 0; g < n_pairs; g += kGanLossMaxPairs) {
        const int m = n_pairs - g < kGanLossMaxPairs ? n_pairs - g : kGanLossMaxPairs;
        GanGradTable tab{};
        int blocks = 0;
        for (int i = 0; i < m; ++i) {
            tab.p[i] = GanGradPair{(const float*)a[g + i], (const float*)b[g + i], (float*)da[g + i], db ? (float*)db[g + i] : nullptr,
                                   (long long)numels[g + i], blocks, 0};
            blocks += (int)gan_loss_chunks(numels[g + i]);
        }
        if (launch_gan_loss_backward_group(op, tab, m, blocks, grad_loss, s) != hipSuccess) return gan_fail(ST_ERR_HIP, what);
    }
    return ST_OK;
}

int lsgan_op(int mode) {
    return mode == ST_LSGAN_REAL ? GAN_OP_ONE_MINUS_SQ : mode == ST_LSGAN_FAKE ? GAN_OP_SQ : mode == ST_LSGAN_REAL_FAKE ? GAN_OP_ALTERNATE : -1;
}

}  // namespace

extern "C" {

int st_gan_loss_chunk(void) { return kGanLossChunk; }
int st_gan_loss_max_pairs(void) { return kGanLossMaxPairs; }

int64_t st_gan_loss_scratch_bytes(const int64_t* numels, int n_pairs) {
    long long chunks = 0;
    if (int rc = check_counts(numels, n_pairs, &chunks)) return rc;
    return 8ll * (chunks + n_pairs);
}

int st_feature_loss_forward(const void* const* real, const void* const* fake, const int64_t* numels, int n_pairs, float* out,
                            void* scratch, int64_t scratch_bytes, void* stream) {
    return run_forward(GAN_OP_ABS_DIFF, 2.0f, real, fake, numels, n_pairs, out, scratch, scratch_bytes, stream,
                       "feature_loss kernel launch failed");
}

int st_feature_loss_backward(const void* const* real, const void* const* fake, const int64_t* numels, int n_pairs,
                             const float* grad_loss, void* const* grad_real, void* const* grad_fake, void* stream) {
    if (n_pairs > 0 && !grad_fake) return gan_fail(ST_ERR_INVALID, "null argument");
    return run_backward(GAN_OP_ABS_DIFF, real, fake, numels, n_pairs, grad_loss, grad_real, grad_fake, stream,
                        "feature_loss backward kernel launch failed");
}

int st_lsgan_loss_forward(const void* const* x, const int64_t* numels, int n_pairs, int mode, float* out, void* scratch,
                          int64_t scratch_bytes, void* stream) {
    const int op = lsgan_op(mode);
    if (op < 0) return gan_fail(ST_ERR_INVALID, "mode must be ST_LSGAN_REAL, ST_LSGAN_FAKE or ST_LSGAN_REAL_FAKE");
    return run_forward(op, 1.0f, x, x, numels, n_pairs, out, scratch, scratch_bytes, stream, "lsgan_loss kernel launch failed");
}

int st_lsgan_loss_backward(const void* const* x, const int64_t* numels, int n_pairs, int mode, const float* grad_loss,
                           void* const* grad_x, void* stream) {
    const int op = lsgan_op(mode);
    if (op < 0) return gan_fail(ST_ERR_INVALID, "mode must be ST_LSGAN_REAL, ST_LSGAN_FAKE or ST_LSGAN_REAL_FAKE");
    return run_backward(op, x, x, numels, n_pairs, grad_loss, grad_x, nullptr, stream, "lsgan_loss backward kernel launch failed");
}

}  // extern "C"
