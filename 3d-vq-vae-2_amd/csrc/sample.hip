// Prior sampling, one raster position per launch (the reference's PixelSNAIL.sample,
// pixel_model/pixelsnail.py:219-272: the forward's output at the position, then the hard
// Gumbel-softmax): the parse_output head on the position's hidden row, the draw, and the three
// writes, for every sample of the batch -- one workgroup (256 threads) per sample.
//
//   logit[k] = bias[k] + sum_c hidden[b][p][c] * W[k][c]      (fp32 accumulation; 16-bit hidden: W rounded
//                                                             to that format on load; no rounding after)
//   code     = argmax_k (logit[k] / T + g_k), first index on a tie;  T == 0: argmax_k logit[k]
//   g_k      = -logf(-logf(u_k)),  u_k = (float(hash >> 9) + 0.5f) * 2^-23   (in (0, 1), exact in fp32)
//   hash     = mix(mix(mix(lo ^ hi * 0x9E3779B1 ^ s_lo * 0xC2B2AE3D ^ s_hi * 0x165667B1)
//                      ^ p_lo * 0x85EBCA77 ^ p_hi * 0x9E3779B1) ^ k * 0x27D4EB2F)
//              lo / hi: the halves of *seed; s = sample_base + b; mix: the lowbias32 finisher
//              x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
//              (attention.hip's logit_hash, chained: for one (seed, s, p) the K hashes are distinct)
//
// The hidden row is staged in LDS as fp32.  A wave owns kU logits at a time: its lanes stride over c
// (256-byte coalesced reads of each W row, conflict-free LDS reads), kU independent accumulators keep
// kU loads in flight, and the fixed DPP tree of wave_sum finishes each logit, so a logit's value does
// not depend on the batch or the launch.  The scores' argmax runs per thread over k, then over the
// wave by shuffles and over the four waves through LDS, comparing (score, index) so the first index
// wins a tie at every level.  The work is tiny (at most 1 MB of weights per sample): one clean pass,
// no tuning for peak rates.  *pos and *seed are read, never written (graph replays advance them).
#include "common.h"

#include <cmath>

namespace vq3d {
namespace {

constexpr int kNT = 256, kWaves = kNT / kWave;
constexpr int kMaxK = 1024, kMaxC = 1024, kMinK = 8;
constexpr int kU = 4;  // logits a wave accumulates side by side

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// a parse_output weight as the head's operand: fp32 as it is, else rounded to the 16-bit format
template <typename TH>
__device__ __forceinline__ float w_operand(float w) {
    if constexpr (sizeof(TH) == 4)
        return w;
    else
        return h2f_lo(f2h(w));
}

template <typename TH, typename TO>
__global__ __launch_bounds__(kNT) void k_sample_step(const TH *__restrict__ hidden, int64_t hidden_positions, int c,
                                                     const float *__restrict__ W, const float *__restrict__ bias,
                                                     int k, const int64_t *__restrict__ pos, float temperature,
                                                     const uint64_t *__restrict__ seed, int64_t sample_base,
                                                     TO *__restrict__ onehot, int64_t *__restrict__ codes,
                                                     int64_t npos, float *__restrict__ logits_out) {
    __shared__ float hs[kMaxC], lg[kMaxK];
    __shared__ float best_s[kWaves];
    __shared__ int best_i[kWaves];
    const int64_t p = *pos;
    if (p < 0 || p >= min(npos, hidden_positions)) return;  // the whole grid alike
    const int b = int(blockIdx.x), tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;

    const TH *h = hidden + (int64_t(b) * hidden_positions + p) * c;
    for (int i = tid; i < c; i += kNT) hs[i] = ld(h + i);
    __syncthreads();

    for (int k0 = wave * kU; k0 < k; k0 += kWaves * kU) {
        float acc[kU] = {0.f, 0.f, 0.f, 0.f};
        for (int i = lane; i < c; i += kWave) {
            const float x = hs[i];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int kk = min(k0 + u, k - 1);  // a clamped row past the end is computed and dropped
                acc[u] = fmaf(x, w_operand<TH>(W[int64_t(kk) * c + i]), acc[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const float s = wave_sum(acc[u]);
            if (lane == 0 && k0 + u < k) lg[k0 + u] = bias[k0 + u] + s;
        }
    }
    __syncthreads();

    const uint64_t sd = *seed, smp = uint64_t(sample_base + b);
    const uint32_t h0 = mix32(uint32_t(sd) ^ (uint32_t(sd >> 32) * 0x9E3779B1u) ^ (uint32_t(smp) * 0xC2B2AE3Du) ^
                              (uint32_t(smp >> 32) * 0x165667B1u));
    const uint32_t h1 = mix32(h0 ^ (uint32_t(p) * 0x85EBCA77u) ^ (uint32_t(uint64_t(p) >> 32) * 0x9E3779B1u));
    float best = -INFINITY;
    int arg = tid;  // >= k in threads without a logit: loses every tie against a real index
    for (int kk = tid; kk < k; kk += kNT) {
        float s = lg[kk];
        if (temperature > 0.f) {
            const uint32_t hash = mix32(h1 ^ (uint32_t(kk) * 0x27D4EB2Fu));
            const float u = (float(hash >> 9) + 0.5f) * 0x1p-23f;
            s = s / temperature + -logf(-logf(u));
        }
        if (s > best) {
            best = s;
            arg = kk;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(best, o, kWave);
        const int oi = __shfl_xor(arg, o, kWave);
        if (os > best || (os == best && oi < arg)) {
            best = os;
            arg = oi;
        }
    }
    if (lane == 0) {
        best_s[wave] = best;
        best_i[wave] = arg;
    }
    __syncthreads();
    best = best_s[0];
    arg = best_i[0];  // thread 0's start index is 0: arg < k whatever the scores are
#pragma unroll
    for (int w = 1; w < kWaves; ++w)
        if (best_s[w] > best || (best_s[w] == best && best_i[w] < arg)) {
            best = best_s[w];
            arg = best_i[w];
        }

    TO *row = onehot + (int64_t(b) * npos + p) * k;
    for (int kk = tid; kk < k; kk += kNT) {
        st(row + kk, kk == arg ? 1.f : 0.f);
        if (logits_out) logits_out[int64_t(b) * k + kk] = lg[kk];
    }
    if (tid == 0) codes[int64_t(b) * npos + p] = arg;
}

template <typename TH>
void launch(int32_t onehot_dtype, const void *hidden, int64_t hidden_positions, int c, const float *W,
            const float *bias, int k, const int64_t *pos, float temperature, const uint64_t *seed, int64_t sample_base,
            void *onehot, int64_t *codes, int64_t npos, int batch, float *logits_out, hipStream_t s) {
    const TH *h = static_cast<const TH *>(hidden);
    if (onehot_dtype == VQ3D_F32)
        k_sample_step<TH, float><<<batch, kNT, 0, s>>>(h, hidden_positions, c, W, bias, k, pos, temperature, seed,
                                                       sample_base, static_cast<float *>(onehot), codes, npos,
                                                       logits_out);
    else
        k_sample_step<TH, h16_t><<<batch, kNT, 0, s>>>(h, hidden_positions, c, W, bias, k, pos, temperature, seed,
                                                       sample_base, static_cast<h16_t *>(onehot), codes, npos,
                                                       logits_out);
}

}  // namespace
}  // namespace vq3d

using namespace vq3d;

extern "C" {

int vq3d_prior_sample_step(int32_t hidden_dtype, const void *hidden, int64_t hidden_positions, int32_t c,
                           const float *weight, const float *bias, int32_t k, const int64_t *pos, float temperature,
                           const uint64_t *seed, int64_t sample_base, int32_t onehot_dtype, void *onehot,
                           int64_t *codes, int64_t npos, int32_t batch, float *logits_out, vq3d_stream_t stream) {
    if ((hidden_dtype != VQ3D_F32 && hidden_dtype != VQ3D_HALF) || (onehot_dtype != VQ3D_F32 && onehot_dtype != VQ3D_HALF))
        return fail("prior_sample_step: hidden and onehot must be fp32 or one 16-bit format");
    if (k < kMinK || k > kMaxK) return fail("prior_sample_step: 8 <= k <= 1024");
    if (c <= 0 || c > kMaxC || c % 8 != 0) return fail("prior_sample_step: c must be a multiple of 8, at most 1024");
    if (batch <= 0 || npos <= 0 || hidden_positions <= 0) return fail("prior_sample_step: bad sizes");
    if (!hidden || !weight || !bias || !pos || !seed || !onehot || !codes) return fail("prior_sample_step: null pointer");
    if (!(temperature >= 0.f) || std::isinf(temperature))
        return fail("prior_sample_step: temperature must be finite and not negative (0: argmax)");
    hipStream_t s = as_stream(stream);
    if (hidden_dtype == VQ3D_F32)
        launch<float>(onehot_dtype, hidden, hidden_positions, c, weight, bias, k, pos, temperature, seed, sample_base,
                      onehot, codes, npos, batch, logits_out, s);
    else
        launch<h16_t>(onehot_dtype, hidden, hidden_positions, c, weight, bias, k, pos, temperature, seed, sample_base,
                      onehot, codes, npos, batch, logits_out, s);
    return check_launch("prior_sample_step");
}

}  // extern "C"
