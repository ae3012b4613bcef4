// MelStyleEncoder and DurationPredictor kernels (models/reference_encoder.py:22-93, models/duration_predictor.py:5-37).
// fp32 throughout: the durations downstream are ceil()ed (models/model.py:83-84), so a logw error of 1e-3 already flips about
// one frame per 200-token utterance; the convolutions and linears therefore run on the fp32-input MFMA
// (v_mfma_f32_32x32x2_f32: bit-for-bit a k-ordered fp32 FMA chain) instead of the 16-bit operands of the DiT blocks.
// Tensors stay in the reference's channel-major layout (B, C, T); both modules run once per utterance and are small.
#include "fp32_tile.h"
#include "style_dp_drop.h"

#include <math.h>

namespace st {

// One block = a 64 (channel) x 64 (frame) output tile on fp32_tile.h's wave / lane mapping.  K = (input channel, tap) pairs in
// the weight's own order, 16 channels x TAPS per LDS chunk; the B operand is a halo tile [16][64 + TAPS - 1] of the input.
// MODE (training, style_dp_bwd.hip) -- SD_MODE_FWD: the inference kernel.  SD_MODE_DGRAD: the data gradient of a conv whose
// nn.Conv1d weight is W (Cin_fwd = a.Cout, Cout_fwd = a.Cin, TAPS): A is staged straight from W, transposed and tap-flipped,
// W'[ci][co][j] = W[co][ci][TAPS - 1 - j]; no bias, no epilogue activation, a.res (if set) is added after the output mask.
// SD_MODE_FWD_PRE: the inference kernel that also writes the pre-activation (acc + bias) to a.pre for the backward.
// CHAINS: independent accumulators over the K loop, LDS chunk c into accumulator c % CHAINS, added in ascending order at the end.
// 1 is the k-ordered chain; 4 (SdConvArgs::chains, taps = 1: the Vocos generator above dim 512, whose contractions run to 2048
// terms through 12 blocks) quarters the length of every rounding chain.
template <int TAPS, int MODE, int CHAINS = 1>
__global__ __launch_bounds__(256) void sd_conv_kernel(SdConvArgs a) {
    constexpr int KC = kTileChunk * TAPS, WS = KC + 1, PAD = TAPS / 2, XS = kTile + TAPS - 1;
    __shared__ float Ws[kTile * WS];
    __shared__ float Xs[kTileChunk * XS];
    const int tid = threadIdx.x;
    const TileLane l = tile_lane();
    const int t0 = blockIdx.x * kTile, co0 = blockIdx.y * kTile, b = blockIdx.z;
    const int Cin = a.Cin, Cout = a.Cout, T = a.T;
    const float* inb = a.in + (size_t)b * Cin * T;
    f32x16 accs[CHAINS];
#pragma unroll
    for (int q = 0; q < CHAINS; ++q) accs[q] = tile_zero();
    for (int cq = 0; cq < Cin; cq += kTileChunk * CHAINS) {
#pragma unroll
      for (int q = 0; q < CHAINS; ++q) {
        const int ci0 = cq + q * kTileChunk;
        if (CHAINS > 1 && ci0 >= Cin) break;      // block-uniform
        f32x16& acc = accs[q];
        for (int i = tid; i < kTile * KC; i += 256) {
            const int row = i / KC, kk = i - row * KC;
            const int co = co0 + row, ci = ci0 + kk / TAPS;
            if constexpr (MODE == SD_MODE_DGRAD) {
                const int j = kk - (kk / TAPS) * TAPS;
                Ws[row * WS + kk] = (co < Cout && ci < Cin) ? a.w[((size_t)ci * Cout + co) * TAPS + (TAPS - 1 - j)] : 0.0f;
            } else {
                Ws[row * WS + kk] = (co < Cout && ci < Cin) ? a.w[((size_t)co * Cin + ci0) * TAPS + kk] : 0.0f;
            }
        }
        for (int i = tid; i < kTileChunk * XS; i += 256) {
            const int row = i / XS, j = i - row * XS;
            const int ci = ci0 + row, t = t0 + j - PAD;
            float v = 0.0f;
            if (ci < Cin && t >= 0 && t < T) {
                v = inb[(size_t)ci * T + t];
                if (a.addv) v += a.addv[(size_t)b * Cin + ci];
                if (a.imask) v *= a.imask[(size_t)b * T + t];
            }
            Xs[row * XS + j] = v;
        }
        __syncthreads();
        tile_mfma<KC, 8>(acc, Ws, WS, l, [&](int k, int col) { const int cil = k / TAPS; return Xs[cil * XS + col + (k - cil * TAPS)]; });
        __syncthreads();
      }
    }
    f32x16 acc = accs[0];
#pragma unroll
    for (int q = 1; q < CHAINS; ++q) acc += accs[q];
    const int t = t0 + l.wt * 32 + l.r;
    if (t >= T) return;
    const float om = a.omask ? a.omask[(size_t)b * T + t] : 1.0f;
    tile_for_each(acc, l, [&](int row, float sum) {
        const int co = co0 + row;
        if (co >= Cout) return;
        const size_t o = ((size_t)b * Cout + co) * T + t;
        if constexpr (MODE == SD_MODE_DGRAD) {
            a.out[o] = a.res ? sum * om + a.res[o] : sum * om;
            return;
        }
        float v = sum + a.bias[co];
        if constexpr (MODE == SD_MODE_FWD_PRE) a.pre[o] = v;
        if (a.epi == SD_EPI_MISH) {          // x * tanh(softplus(x)), softplus at torch's threshold 20
            const float sp = v > 20.0f ? v : log1pf(expf(v));
            v = v * tanhf(sp);
        } else if (a.epi == SD_EPI_RELU) {
            v = fmaxf(v, 0.0f);
        }
        a.out[o] = v * om;
    });
}

hipError_t launch_sd_conv(const SdConvArgs& a, hipStream_t s) {
    if (a.B < 1 || a.T < 1 || a.Cin < 1 || a.Cout < 1 || !a.in || !a.w || !a.bias || !a.out) return hipErrorInvalidValue;
    const dim3 grid((a.T + kTile - 1) / kTile, (a.Cout + kTile - 1) / kTile, a.B), blk(256);
    if (a.chains != 1 && (a.chains != 4 || a.taps != 1)) return hipErrorInvalidValue;
    switch (a.taps) {
        case 1: if (a.chains == 4) hipLaunchKernelGGL((sd_conv_kernel<1, SD_MODE_FWD, 4>), grid, blk, 0, s, a);
                else               hipLaunchKernelGGL((sd_conv_kernel<1, SD_MODE_FWD>), grid, blk, 0, s, a);
                break;
        case 3: hipLaunchKernelGGL((sd_conv_kernel<3, SD_MODE_FWD>), grid, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL((sd_conv_kernel<5, SD_MODE_FWD>), grid, blk, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_sd_conv_pre(const SdConvArgs& a, hipStream_t s) {
    if (a.B < 1 || a.T < 1 || a.Cin < 1 || a.Cout < 1 || !a.in || !a.w || !a.bias || !a.out || !a.pre || a.chains != 1) return hipErrorInvalidValue;
    const dim3 grid((a.T + kTile - 1) / kTile, (a.Cout + kTile - 1) / kTile, a.B), blk(256);
    switch (a.taps) {
        case 1: hipLaunchKernelGGL((sd_conv_kernel<1, SD_MODE_FWD_PRE>), grid, blk, 0, s, a); break;
        case 3: hipLaunchKernelGGL((sd_conv_kernel<3, SD_MODE_FWD_PRE>), grid, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL((sd_conv_kernel<5, SD_MODE_FWD_PRE>), grid, blk, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_sd_conv_dgrad(const SdConvArgs& a, hipStream_t s) {
    if (a.B < 1 || a.T < 1 || a.Cin < 1 || a.Cout < 1 || !a.in || !a.w || !a.out || a.addv || a.imask) return hipErrorInvalidValue;
    const dim3 grid((a.T + kTile - 1) / kTile, (a.Cout + kTile - 1) / kTile, a.B), blk(256);
    if (a.chains != 1 && (a.chains != 4 || a.taps != 1)) return hipErrorInvalidValue;
    switch (a.taps) {
        case 1: if (a.chains == 4) hipLaunchKernelGGL((sd_conv_kernel<1, SD_MODE_DGRAD, 4>), grid, blk, 0, s, a);
                else               hipLaunchKernelGGL((sd_conv_kernel<1, SD_MODE_DGRAD>), grid, blk, 0, s, a);
                break;
        case 3: hipLaunchKernelGGL((sd_conv_kernel<3, SD_MODE_DGRAD>), grid, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL((sd_conv_kernel<5, SD_MODE_DGRAD>), grid, blk, 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void sd_glu_residual_kernel(float* __restrict__ h, const float* __restrict__ u, int C, int T, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t per = (int64_t)C * T;
        const int64_t b = i / per, rem = i - b * per;          // rem = c * T + t
        const float* ub = u + b * 2 * per;
        const float val = ub[rem], gate = ub[per + rem];
        h[i] = h[i] + val * (1.0f / (1.0f + expf(-gate)));
    }
}

hipError_t launch_sd_glu_residual(float* h, const float* u, int B, int C, int T, hipStream_t s) {
    const int64_t n = (int64_t)B * C * T;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(sd_glu_residual_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, h, u, C, T, n);
    return hipGetLastError();
}

// One block = 64 frames of one item; 4 threads per frame split the channels, partial sums meet in LDS.  Two passes
// (mean, then the mean squared deviation: nn.LayerNorm's biased variance), then the affine write.
__global__ __launch_bounds__(256) void sd_layernorm_channels_kernel(float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ bb, float eps, int C, int T) {
    __shared__ float red[4][64];
    const int tl = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int t = blockIdx.x * 64 + tl, b = blockIdx.y;
    const bool ok = t < T;
    float* xb = x + (size_t)b * C * T;
    float sum = 0.0f;
    if (ok) for (int c = g; c < C; c += 4) sum += xb[(size_t)c * T + t];
    red[g][tl] = sum;
    __syncthreads();
    const float mean = (red[0][tl] + red[1][tl] + red[2][tl] + red[3][tl]) / (float)C;
    __syncthreads();
    float sq = 0.0f;
    if (ok) for (int c = g; c < C; c += 4) { const float d = xb[(size_t)c * T + t] - mean; sq += d * d; }
    red[g][tl] = sq;
    __syncthreads();
    const float var = (red[0][tl] + red[1][tl] + red[2][tl] + red[3][tl]) / (float)C;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (ok) for (int c = g; c < C; c += 4) {
        const size_t i = (size_t)c * T + t;
        xb[i] = (xb[i] - mean) * rstd * w[c] + bb[c];
    }
}

hipError_t launch_sd_layernorm_channels(float* x, const float* w, const float* b, float eps, int B, int C, int T, hipStream_t s) {
    hipLaunchKernelGGL(sd_layernorm_channels_kernel, dim3((T + 63) / 64, B), dim3(256), 0, s, x, w, b, eps, C, T);
    return hipGetLastError();
}

// One wave = 64 queries of one (item, head), one query per lane: q and the output accumulator (64 + 64 fp32) live in
// registers, keys and values stream through LDS 64 frames at a time (every lane reads the same element: broadcast).
// Softmax is the online form, rescaled once per key tile; exact expf.  Masked keys get a score of -inf and weight 0.
// TRAIN (style_dp_bwd.hip): the probabilities (not the normaliser) take the dropout factors of site d, and every query's final
// running max and 1 / sum go to stats[0 / 1][(b * H + head) * T + query] for the backward.  TRAIN = false is the inference kernel.
template <bool TRAIN>
__global__ __launch_bounds__(64) void sd_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ kmask,
                                                          float* __restrict__ out, int H, int T, SdDrop drop, float* __restrict__ stats) {
    __shared__ float Ks[64 * 64];
    __shared__ float Vs[64 * 64];
    __shared__ float valid[64];
    __shared__ float Zs[TRAIN ? 64 * 64 : 1];
    __shared__ float Ss[TRAIN ? 64 * 64 : 1];
    const int lane = threadIdx.x, hd = blockIdx.y, b = blockIdx.z;
    const int tq = blockIdx.x * 64 + lane, D = H * 64;
    const float* qb = qkv + ((size_t)b * 3 * D + hd * 64) * T;
    const float* kb = qb + (size_t)D * T;
    const float* vb = qb + (size_t)2 * D * T;
    float q[64], acc[64];
#pragma unroll
    for (int d = 0; d < 64; ++d) { q[d] = tq < T ? qb[(size_t)d * T + tq] * 0.125f : 0.0f; acc[d] = 0.0f; }
    float m = -INFINITY, l = 0.0f;
    for (int k0 = 0; k0 < T; k0 += 64) {
        const int tk = k0 + lane;
        const bool kv = tk < T && (!kmask || kmask[(size_t)b * T + tk] != 0.0f);
        for (int d = 0; d < 64; ++d) {
            Ks[d * 64 + lane] = tk < T ? kb[(size_t)d * T + tk] : 0.0f;
            Vs[d * 64 + lane] = tk < T ? vb[(size_t)d * T + tk] : 0.0f;
        }
        valid[lane] = kv ? 1.0f : 0.0f;
        __syncthreads();
        if constexpr (!TRAIN) {
        float sc[64];
        float mt = -INFINITY;
#pragma unroll
        for (int j = 0; j < 64; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int d = 0; d < 64; ++d) s = fmaf(q[d], Ks[d * 64 + j], s);
            sc[j] = valid[j] != 0.0f ? s : -INFINITY;
            mt = fmaxf(mt, sc[j]);
        }
        const float mn = fmaxf(m, mt);
        if (mn != -INFINITY) {
            const float corr = expf(m - mn);          // m == -inf: 0 (acc and l are 0 then)
            l *= corr;
#pragma unroll
            for (int d = 0; d < 64; ++d) acc[d] *= corr;
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                const float p = expf(sc[j] - mn);     // masked: exp(-inf) = 0
                l += p;
#pragma unroll
                for (int d = 0; d < 64; ++d) acc[d] = fmaf(p, Vs[d * 64 + j], acc[d]);
            }
            m = mn;
        }
        } else {
        // TRAIN: the same arithmetic in the same order, the scores and this query's keep factors (sd_drop_attn's mask) in its
        // own LDS columns instead of registers (the extra factor pushed the register-resident form past 256 VGPRs)
        float mt = -INFINITY;
        const unsigned rh = drop_rowh(drop.seed, (unsigned)((b * H + hd) * T + tq));
#pragma unroll 1
        for (int j = 0; j < 64; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int d = 0; d < 64; ++d) s = fmaf(q[d], Ks[d * 64 + j], s);
            s = valid[j] != 0.0f ? s : -INFINITY;
            Ss[j * 64 + lane] = s;
            mt = fmaxf(mt, s);
            const unsigned hh = drop_pair(rh, drop_colh(drop.seed, (unsigned)(k0 + j) >> 1));
            Zs[j * 64 + lane] = !drop.thresh16 || ((j & 1) ? (hh >> 16) : (hh & 0xFFFFu)) >= drop.thresh16 ? drop.scale : 0.0f;
        }
        const float mn = fmaxf(m, mt);
        if (mn != -INFINITY) {
            const float corr = expf(m - mn);
            l *= corr;
#pragma unroll
            for (int d = 0; d < 64; ++d) acc[d] *= corr;
#pragma unroll 2
            for (int j = 0; j < 64; ++j) {
                float p = expf(Ss[j * 64 + lane] - mn);
                l += p;
                p *= Zs[j * 64 + lane];
#pragma unroll
                for (int d = 0; d < 64; ++d) acc[d] = fmaf(p, Vs[d * 64 + j], acc[d]);
            }
            m = mn;
        }
        }
        __syncthreads();
    }
    if (tq >= T) return;
    const float inv = l > 0.0f ? 1.0f / l : 0.0f;
    if constexpr (TRAIN) {
        const size_t r = (size_t)(b * H + hd) * T + tq;
        stats[r] = m;
        stats[(size_t)gridDim.z * H * T + r] = inv;
    }
    float* ob = out + ((size_t)b * D + hd * 64) * T + tq;
#pragma unroll
    for (int d = 0; d < 64; ++d) ob[(size_t)d * T] = acc[d] * inv;
}

hipError_t launch_sd_attention(const float* qkv, const float* kmask, float* out, int B, int H, int T, hipStream_t s) {
    hipLaunchKernelGGL(sd_attention_kernel<false>, dim3((T + 63) / 64, H, B), dim3(64), 0, s, qkv, kmask, out, H, T, SdDrop{}, nullptr);
    return hipGetLastError();
}

hipError_t launch_sd_attention_train(const float* qkv, const float* kmask, float* out, float* stats, const SdDrop& d, int B, int H, int T,
                                     hipStream_t s) {
    hipLaunchKernelGGL(sd_attention_kernel<true>, dim3((T + 63) / 64, H, B), dim3(64), 0, s, qkv, kmask, out, H, T, d, stats);
    return hipGetLastError();
}

// One block = one (item, channel) row: the 256 lanes stride over the frames (coalesced loads), partial sums and valid-frame
// counts meet in a fixed LDS tree (deterministic).
__global__ __launch_bounds__(256) void sd_mean_pool_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                           float* __restrict__ c, int O, int T) {
    __shared__ float ssum[256], scnt[256];
    const int o = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* xo = x + ((size_t)b * O + o) * T;
    const float* mb = mask ? mask + (size_t)b * T : nullptr;
    float sum = 0.0f, n = 0.0f;
    for (int t = tid; t < T; t += 256) {
        if (mb && mb[t] == 0.0f) continue;
        sum += xo[t];
        n += 1.0f;
    }
    ssum[tid] = sum; scnt[tid] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { ssum[tid] += ssum[tid + w]; scnt[tid] += scnt[tid + w]; }
        __syncthreads();
    }
    if (tid == 0) c[(size_t)b * O + o] = scnt[0] > 0.0f ? ssum[0] / scnt[0] : __builtin_nanf("");
}

hipError_t launch_sd_mean_pool(const float* x, const float* mask, float* c, int B, int O, int T, hipStream_t s) {
    hipLaunchKernelGGL(sd_mean_pool_kernel, dim3(O, B), dim3(256), 0, s, x, mask, c, O, T);
    return hipGetLastError();
}

}  // namespace st
