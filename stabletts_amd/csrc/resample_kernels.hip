// The sinc resampler as one multi-tensor kernel: torchaudio.functional.resample's polyphase filter read through its compact tap
// table (only the taps inside the window, 13 or 14 of the dense form's 174 per phase at 48000 -> 44100).  One launch covers up to
// kResampleMaxTensors waveforms, the table of which is a kernel argument; block b produces one kResampleChunk-sample chunk of
// one entry's output, found from the entry's first_block.  fp32, no MFMA.
//
// Lane t of round k produces output q = chunk start + 256 k + t: consecutive lanes read consecutive taps (the table is
// tap-major and a phase is q mod new), store consecutive outputs, and gather inputs that ascend with the lane.  The table is
// always read through the vector L1 and the L2.  The block's input span (chunk orig / new + S samples) is read the same way
// for short filters and staged in LDS once for long ones (resample_stages(S)): measured on an MI355X at B = 32 x 10 s, staging
// costs 7 .. 12 % at S = 13 and 14, breaks even at S = 34 and wins 1.5 x at S = 373 (Kaiser, lowpass_filter_width = 64).  Every
// sample is one ordered chain of fmaf over its taps, written explicitly, whichever way its inputs arrive: no 16-byte variant, no
// sum across lanes, so a sample's bits cannot depend on its entry's address, list position, neighbours or launch.
//
// Taps of a sample that fall outside [0, L_in) are cut from its loop bounds (64-bit, once per sample): they contribute
// exactly zero and are never dereferenced.
#include "resample_launch.h"

namespace st {

namespace {

constexpr int kRounds = kResampleChunk / 256;
static_assert(kRounds * 256 == kResampleChunk, "a chunk is a whole number of 256-sample rounds");
static_assert(sizeof(ResampleTable) + sizeof(ResampleFilter) + 16 <= 3840, "the table travels as a kernel argument (4 KB in all, hidden arguments included)");

// entry of block blk: the last one whose first_block <= blk (first_block ascends, e[0].first_block == 0)
__device__ __forceinline__ int find_entry(const ResampleTable& tab, int n, int blk) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab.e[mid].first_block <= blk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace

__global__ __launch_bounds__(256) void resample_kernel(const ResampleTable tab, int n, const ResampleFilter f) {
    extern __shared__ float xs[];           // kResampleSpan floats where resample_stages(S), none otherwise
    const int blk = blockIdx.x;
    const int ent = find_entry(tab, n, blk);
    const ResampleEntry& e = tab.e[ent];
    const long long q0 = (long long)(blk - e.first_block) * kResampleChunk;      // the chunk's first output sample
    const long long left = e.L_out - q0;
    const int len = left < (long long)kResampleChunk ? (int)left : kResampleChunk;                     // >= 1
    const int orig = f.orig, new_ = f.new_, S = f.S;
    // block-uniform: the chunk's first input period and phase, then 32-bit steps from there (new_ * S <= 2^22)
    const long long j0 = q0 / new_;
    const int i0 = (int)(q0 - j0 * new_);
    const int step_j = 256 / new_, step_i = 256 - step_j * new_;                  // one round further: 256 outputs
    const unsigned first_ii = (unsigned)i0 + threadIdx.x;                         // < 2^22 + 256
    int dj = (int)(first_ii / (unsigned)new_);
    int i = (int)(first_ii - (unsigned)dj * (unsigned)new_);
    const float* __restrict__ x = e.x;
    float* __restrict__ y = e.y + q0;
    const float* __restrict__ taps = f.taps;
    const long long L_in = e.L_in;
    // The chunk's input span, from one sample before its first output's first tap to one past its last output's last tap,
    // staged once where it fits; a sample whose taps are not all inside what was staged reads the waveform itself.
    const long long q_last = q0 + len - 1, j_last = q_last / new_;
    const long long span_lo = j0 * (long long)orig + (long long)f.first[i0] - 1;
    const long long span_hi = j_last * (long long)orig + (long long)f.first[(int)(q_last - j_last * new_)] + S + 1;
    const bool staged = resample_stages(S) && span_hi - span_lo <= (long long)kResampleSpan;
    if (staged) {
        const int span = (int)(span_hi - span_lo);
        for (int p = (int)threadIdx.x; p < span; p += 256) {
            const long long idx = span_lo + p;
            xs[p] = idx >= 0 && idx < L_in ? x[idx] : 0.0f;
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < kRounds; ++k) {
        const int t = k * 256 + (int)threadIdx.x;
        if (t < len) {
            const long long base = (j0 + dj) * (long long)orig + (long long)f.first[i];   // input index of tap 0
            // taps s with 0 <= base + s < L_in
            const int s_lo = base < 0 ? (-base < (long long)S ? (int)-base : S) : 0;
            const long long room = L_in - base;
            const int s_hi = room < (long long)S ? (room > 0 ? (int)room : 0) : S;
            float acc = 0.0f;
            // The same ordered chain of fmaf over [s_lo, s_hi) on every path.  A sample with all S taps inside the waveform walks
            // the table by a block-uniform row pointer and reads its inputs at constant offsets from one address (four per
            // 16-byte load through the cache); a sample at either end of the waveform indexes both by its own bounds.
            if (s_lo == 0 && s_hi == S) {
                const float* trow = taps;
                if (staged && base >= span_lo && base + S <= span_hi) {
                    const float* xl = xs + (int)(base - span_lo);
#pragma unroll 4
                    for (int s = 0; s < S; ++s, trow += new_) acc = __fmaf_rn(trow[i], xl[s], acc);
                } else {
                    const float* xb = x + base;
#pragma unroll 4
                    for (int s = 0; s < S; ++s, trow += new_) acc = __fmaf_rn(trow[i], xb[s], acc);
                }
            } else {
                const float* tp = taps + i;
                const float* xb = x + base;                                       // dereferenced inside [s_lo, s_hi) only
                for (int s = s_lo; s < s_hi; ++s) acc = __fmaf_rn(tp[s * new_], xb[s], acc);
            }
            y[t] = acc;
        }
        dj += step_j;
        i += step_i;
        if (i >= new_) { i -= new_; ++dj; }
    }
}

hipError_t launch_resample(const ResampleTable& tab, int n, int blocks, const ResampleFilter& f, hipStream_t s) {
    if (n < 1 || n > kResampleMaxTensors || blocks < n) return hipErrorInvalidValue;
    if (f.orig < 1 || f.new_ < 1 || f.S < 1 || (long long)f.new_ * f.S > kResampleMaxTable) return hipErrorInvalidValue;
    const size_t lds = resample_stages(f.S) ? sizeof(float) * kResampleSpan : 0;
    hipLaunchKernelGGL(resample_kernel, dim3(blocks), dim3(256), lds, s, tab, n, f);
    return hipGetLastError();
}

}  // namespace st
