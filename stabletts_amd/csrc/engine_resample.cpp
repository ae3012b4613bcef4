// The sinc resampler behind the C ABI (st_resample / st_resample_chunk / st_resample_max_tensors): a stateless helper like the
// optimizer step (errors through st_last_error(NULL)).  The host arrays of device pointers and lengths are cut into launch
// groups of kResampleMaxTensors non-empty entries whose table is a kernel argument; every argument of the whole list is
// checked before anything touches the device.  The kernel is in resample_kernels.hip.
#include "engine_internal.h"
#include "resample_launch.h"

#include <limits.h>

using namespace st;
using namespace sthost;

namespace {

int resample_fail(int code, const char* msg) { g_create_error = msg; return code; }

bool misaligned(const void* p) { return ((uintptr_t)p & 3) != 0; }

}  // namespace

extern "C" {

int st_resample_chunk(void) { return kResampleChunk; }
int st_resample_max_tensors(void) { return kResampleMaxTensors; }

int st_resample(const void* const* x, void* const* y, const int64_t* in_len, const int64_t* out_len, int n, int orig, int new_,
                const float* taps, const int32_t* first, int S, void* stream) {
    if (n < 0) return resample_fail(ST_ERR_INVALID, "n must be >= 0");
    if (orig < 1 || new_ < 1 || S < 1) return resample_fail(ST_ERR_INVALID, "orig, new_ and S must be >= 1");
    if ((long long)new_ * S > kResampleMaxTable) return resample_fail(ST_ERR_UNSUPPORTED, "the tap table is limited to new_ * S <= 2^22 entries");
    if (!taps || !first || (n > 0 && (!x || !y || !in_len || !out_len))) return resample_fail(ST_ERR_INVALID, "null argument");
    if (misaligned(taps) || misaligned(first)) return resample_fail(ST_ERR_INVALID, "tensor pointers must be 4-byte aligned");
    // the whole list first: nothing is launched for a list with a bad entry
    for (int g = 0; g < n; ++g) {
        if (in_len[g] < 0 || out_len[g] < 0) return resample_fail(ST_ERR_INVALID, "every length must be >= 0");
        const __int128 want = ((__int128)new_ * in_len[g] + orig - 1) / orig;
        if ((__int128)out_len[g] != want) return resample_fail(ST_ERR_INVALID, "out_len must be ceil(new_ * in_len / orig)");
        if (in_len[g] == 0) continue;                      // nothing to read or write: its pointers are not looked at
        if (!x[g] || !y[g]) return resample_fail(ST_ERR_INVALID, "null tensor pointer");
        if (misaligned(x[g]) || misaligned(y[g])) return resample_fail(ST_ERR_INVALID, "tensor pointers must be 4-byte aligned");
        if (out_len[g] > (long long)(INT_MAX / kResampleMaxTensors) * kResampleChunk)    // so that a launch group's chunks fit an int
            return resample_fail(ST_ERR_INVALID, "lengths out of range (an entry exceeds 2^25 chunks)");
    }
    const ResampleFilter f{taps, first, orig, new_, S};
    hipStream_t s = (hipStream_t)stream;
    int g = 0;
    while (g < n) {
        ResampleTable tab{};
        int m = 0, blocks = 0;
        for (; g < n && m < kResampleMaxTensors; ++g) {
            if (in_len[g] == 0) continue;
            tab.e[m++] = ResampleEntry{(const float*)x[g], (float*)y[g], (long long)in_len[g], (long long)out_len[g], blocks, 0};
            blocks += (int)resample_chunks(out_len[g]);
        }
        if (m == 0) break;
        if (launch_resample(tab, m, blocks, f, s) != hipSuccess) return resample_fail(ST_ERR_HIP, "resample kernel launch failed");
    }
    return ST_OK;
}

}  // extern "C"
