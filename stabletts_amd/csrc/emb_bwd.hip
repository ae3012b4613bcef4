// Embedding weight gradient of the text encoder (models/text_encoder.py:35: x = emb(tokens) * sqrt(C)), gfx950.
//
//   dE[v][c] = sqrt(C) * sum over valid rows r = b*T + t (t < len_b) with token id v of dX0[r][c]
//
// dX0 = the gradient at block 0's input.  The sum must be bitwise repeatable (no float atomics, like every other reduction of
// the training backward) and stay parallel under heavy skew: intersperse (text/__init__.py) makes token 0 every other
// position, so one vocabulary row receives about half of all rows.  Six launches:
//   rank     per 256-row chunk: rank of each row among the chunk's rows with the same id, and the chunk's count per id
//   colscan  one wave per id: exclusive prefix of its chunk counts in chunk order (64 chunks per step)
//   scan     over ids: bucket starts and 32-row piece starts
//   scatter  order[start[id] + chunk prefix + rank] = r: a STABLE counting sort of the row indices by id
//   pieces   one block per 32-row piece of one id's bucket: partial[piece][c] = sum of its rows in sorted (= row) order
//   final    one block per id: dE[v][c] = scale * sum of its pieces in order (exact zeros for ids no row carries)
// Integer atomics are not used either: the counts come out of the rank pass, so the whole chain is a fixed function of the ids.
#include "common.h"
#include "train_launch.h"

namespace st {

namespace {
constexpr int kChunk = 256;      // rows per rank / scatter block
constexpr int kPiece = 32;       // rows per reduction piece
constexpr int kScanThreads = 1024;

struct EmbScratch { int *rank, *order, *ccnt, *start, *pstart; float* partial; };

EmbScratch carve(void* base, int64_t R, int V, int C) {
    const int64_t nchunks = (R + kChunk - 1) / kChunk;
    const int64_t npieces = (R + kPiece - 1) / kPiece + V;
    char* p = (char*)base;
    auto take = [&](size_t bytes) { char* q = p; p += (bytes + 255) / 256 * 256; return q; };
    EmbScratch s;
    s.rank = (int*)take((size_t)R * 4);
    s.order = (int*)take((size_t)R * 4);
    s.ccnt = (int*)take((size_t)nchunks * V * 4);
    s.start = (int*)take((size_t)(V + 1) * 4);
    s.pstart = (int*)take((size_t)(V + 1) * 4);
    s.partial = (float*)take((size_t)npieces * C * 4);
    return s;
}
}  // namespace

size_t emb_bwd_scratch_bytes(int64_t R, int n_vocab, int C) {
    const int64_t nchunks = (R + kChunk - 1) / kChunk;
    const int64_t npieces = (R + kPiece - 1) / kPiece + n_vocab;
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    return up((size_t)R * 4) * 2 + up((size_t)nchunks * n_vocab * 4) + up((size_t)(n_vocab + 1) * 4) * 2 + up((size_t)npieces * C * 4);
}

// ids[r] = the row's token id clamped to [0, n_vocab) exactly as embed_tokens_kernel reads it; -1 on padded rows
__global__ __launch_bounds__(256) void emb_ids_kernel(const long long* tokens, const long long* lengths, int n_vocab, int B, int T, int* ids) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= B * T) return;
    const int b = r / T, t = r - b * T;
    long long tok = tokens[r];
    tok = tok < 0 ? 0 : (tok >= n_vocab ? n_vocab - 1 : tok);
    ids[r] = (long long)t < lengths[b] ? (int)tok : -1;
}

hipError_t launch_emb_ids(const long long* tokens, const long long* lengths, int n_vocab, int B, int T, int* ids, hipStream_t s) {
    const int rows = B * T;
    hipLaunchKernelGGL(emb_ids_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, tokens, lengths, n_vocab, B, T, ids);
    return hipGetLastError();
}

__global__ __launch_bounds__(kChunk) void emb_rank_kernel(const int* ids, int64_t R, int V, int* rank, int* ccnt) {
    __shared__ int s_id[kChunk];
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * kChunk + tid;
    const int id = r < R ? ids[r] : -1;
    s_id[tid] = id;
    __syncthreads();
    int rk = 0;
    bool last = true;
    for (int j = 0; j < kChunk; ++j) {      // every lane reads the same word: an LDS broadcast
        const int o = s_id[j];
        rk += (j < tid && o == id) ? 1 : 0;
        last = last && !(j > tid && o == id);
    }
    if (r < R) rank[r] = rk;
    if (id >= 0 && last) ccnt[(size_t)blockIdx.x * V + id] = rk + 1;
}

// one wave per id: exclusive prefix of its chunk counts over the chunks, 64 chunks per step (in place); the id's row count goes
// to start[v] and its piece count to pstart[v] (emb_scan_kernel turns both into starts)
__global__ __launch_bounds__(256) void emb_colscan_kernel(int* __restrict__ ccnt, int nchunks, int V, int* __restrict__ start,
                                                          int* __restrict__ pstart) {
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= V) return;      // (whole waves: no barrier below)
    int run = 0;
    for (int c0 = 0; c0 < nchunks; c0 += 64) {
        const int c = c0 + lane;
        const size_t i = (size_t)c * V + v;
        const int x = c < nchunks ? ccnt[i] : 0;
        int incl = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (c < nchunks) ccnt[i] = run + incl - x;
        run += __shfl(incl, 63, 64);
    }
    if (lane == 0) { start[v] = run; pstart[v] = (run + kPiece - 1) / kPiece; }
}

// one block: the bucket starts and piece starts over ids (exclusive scans of emb_colscan_kernel's counts)
__global__ __launch_bounds__(kScanThreads) void emb_scan_kernel(int V, int* start, int* pstart) {
    __shared__ int s_a[kScanThreads], s_b[kScanThreads];
    __shared__ int carry[2];
    const int tid = threadIdx.x;
    if (tid == 0) { carry[0] = 0; carry[1] = 0; }
    __syncthreads();
    for (int base = 0; base < V; base += kScanThreads) {
        const int v = base + tid;
        const int a = v < V ? start[v] : 0, b = v < V ? pstart[v] : 0;
        s_a[tid] = a; s_b[tid] = b;
        __syncthreads();
        for (int off = 1; off < kScanThreads; off <<= 1) {      // inclusive Hillis-Steele scan
            const int xa = tid >= off ? s_a[tid - off] : 0, xb = tid >= off ? s_b[tid - off] : 0;
            __syncthreads();
            s_a[tid] += xa; s_b[tid] += xb;
            __syncthreads();
        }
        if (v < V) { start[v] = carry[0] + s_a[tid] - a; pstart[v] = carry[1] + s_b[tid] - b; }
        __syncthreads();
        if (tid == 0) { carry[0] += s_a[kScanThreads - 1]; carry[1] += s_b[kScanThreads - 1]; }
        __syncthreads();
    }
    if (tid == 0) { start[V] = carry[0]; pstart[V] = carry[1]; }
}

__global__ __launch_bounds__(kChunk) void emb_scatter_kernel(const int* ids, int64_t R, int V, const int* rank, const int* ccnt,
                                                              const int* start, int* order) {
    const int64_t r = (int64_t)blockIdx.x * kChunk + threadIdx.x;
    if (r >= R) return;
    const int id = ids[r];
    if (id < 0) return;
    order[start[id] + ccnt[(size_t)blockIdx.x * V + id] + rank[r]] = (int)r;
}

__global__ __launch_bounds__(256) void emb_piece_kernel(const float* dX, int C, int V, const int* order, const int* start,
                                                         const int* pstart, float* partial) {
    const int p = blockIdx.x;
    if (p >= pstart[V]) return;
    int lo = 0, hi = V - 1;      // the last id whose first piece is <= p (ids without rows share the next id's pstart)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pstart[mid] <= p) lo = mid; else hi = mid - 1;
    }
    const int v = lo;
    const int beg = start[v] + (p - pstart[v]) * kPiece;
    const int end = min(beg + kPiece, start[v + 1]);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float acc = 0.f;
        for (int j = beg; j < end; ++j) acc += dX[(size_t)order[j] * C + c];
        partial[(size_t)p * C + c] = acc;
    }
}

__global__ __launch_bounds__(256) void emb_final_kernel(const float* partial, int C, const int* pstart, float scale,
                                                         const float* unscale, float* dE) {
    const int v = blockIdx.x;
    const float f = scale * (unscale ? unscale[1] : 1.0f);
    const int p0 = pstart[v], p1 = pstart[v + 1];
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float acc = 0.f;
        for (int p = p0; p < p1; ++p) acc += partial[(size_t)p * C + c];
        dE[(size_t)v * C + c] = p1 > p0 ? acc * f : 0.0f;
    }
}

hipError_t launch_emb_bwd(const float* dX, int C, const int* ids, int64_t R, int n_vocab, float scale, const float* unscale,
                          void* scratch, float* dE, hipStream_t s) {
    if (R < 1 || R >= ((int64_t)1 << 31) || n_vocab < 1) return hipErrorInvalidValue;
    const int V = n_vocab;
    const int nchunks = (int)((R + kChunk - 1) / kChunk);
    const int npieces = (int)((R + kPiece - 1) / kPiece) + V;
    EmbScratch sc = carve(scratch, R, V, C);
    hipError_t err = hipMemsetAsync(sc.ccnt, 0, (size_t)nchunks * V * 4, s);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(emb_rank_kernel, dim3(nchunks), dim3(kChunk), 0, s, ids, R, V, sc.rank, sc.ccnt);
    hipLaunchKernelGGL(emb_colscan_kernel, dim3((V + 3) / 4), dim3(256), 0, s, sc.ccnt, nchunks, V, sc.start, sc.pstart);
    hipLaunchKernelGGL(emb_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, V, sc.start, sc.pstart);
    hipLaunchKernelGGL(emb_scatter_kernel, dim3(nchunks), dim3(kChunk), 0, s, ids, R, V, sc.rank, sc.ccnt, sc.start, sc.order);
    hipLaunchKernelGGL(emb_piece_kernel, dim3(npieces), dim3(256), 0, s, dX, C, V, sc.order, sc.start, sc.pstart, sc.partial);
    hipLaunchKernelGGL(emb_final_kernel, dim3(V), dim3(256), 0, s, sc.partial, C, sc.pstart, scale, unscale, dE);
    return hipGetLastError();
}

}  // namespace st
