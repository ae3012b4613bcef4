// Launcher interface of the sinc resampler (resample_kernels.hip): torchaudio.functional.resample's polyphase filter over a LIST
// of fp32 waveforms, read through its compact tap table.  One multi-tensor family after optim_launch.h: a launch covers up to
// kResampleMaxTensors list entries whose table (pointers, lengths, first block) travels by value as a kernel argument -- no
// device allocation, no table copy.  Output sample q = j new + i of an entry is
//     y[q] = sum over s = 0 .. S-1, ascending, of taps[s * new + i] * x[j * orig + first[i] + s]
// as one fmaf per tap that lies inside [0, L_in); a tap outside it is skipped (contributes exactly zero, never dereferenced).
// A sample's bits depend on its own inputs alone: one block shape, no sum across lanes, and the same chain of fmaf whether its
// inputs come through the cache or, for long filters, from the block's LDS copy of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace st {

constexpr int kResampleMaxTensors = 64;     // list entries per launch: 64 x 40 B of kernel argument
constexpr int kResampleChunk = 1024;        // consecutive output samples of one entry a block produces: 256 threads x 4 rounds
constexpr int kResampleSpan = 6144;         // input samples a block stages in LDS for a long filter (24 KB: six blocks per CU)
constexpr int kResampleStageTaps = 64;      // ... from this S on (measured: staging loses at S = 14, breaks even at 34, wins at 373)
constexpr long long kResampleMaxTable = 1ll << 22;      // new * S entries of a tap table (16 MB): its indices are 32-bit

struct ResampleEntry {        // one list entry of a launch
    const float* x;
    float* y;
    long long L_in;           // >= 1
    long long L_out;          // ceil(new * L_in / orig), >= 1
    int first_block;          // index of the entry's first chunk in the launch's grid (ascending over the table)
    int pad;
};
struct ResampleTable { ResampleEntry e[kResampleMaxTensors]; };

struct ResampleFilter {       // the conversion, shared by every entry
    const float* taps;        // (S, new) tap-major, device
    const int* first;         // (new) signed offset of a phase's first tap from j * orig, device
    int orig, new_, S;
};

// whether a launch with S taps per phase stages its blocks' input spans in LDS: the kernel and its launcher both ask here
__host__ __device__ inline bool resample_stages(int S) { return S >= kResampleStageTaps; }

// chunks of an entry of L_out output samples (= its blocks in a launch)
inline long long resample_chunks(long long L_out) { return (L_out + kResampleChunk - 1) / kResampleChunk; }

// One launch group: n <= kResampleMaxTensors entries whose first_block fields are filled and sum to `blocks`.
hipError_t launch_resample(const ResampleTable& tab, int n, int blocks, const ResampleFilter& f, hipStream_t s);

}  // namespace st
