// The PixelSNAIL prior's output head fused with its loss (pixel_model/pixelsnail.py:78-82 parse_output,
// :112-161 the cross-entropy of shared_step, train_helpers.py:50-63 the two-target mixup loss): per
// voxel row v
//
//   logit[j] = bias[j] + sum_c hidden[v][c] * weight[j][c]     fp32 accumulation on the matrix cores,
//                                                             nothing rounded after the sum (as the sampler's
//                                                             head, sample.hip)
//   lse[v]   = log sum_j exp(logit[j])                         max-subtracted online softmax, fp32
//   loss[v]  = lse[v] - lam * logit[target_a[v]] - (1 - lam) * logit[target_b[v]]
//   pred[v]  = the first index of the largest logit
//
// without the [nrows][k] logits ever reaching memory.  The backward recomputes the logit tiles with the
// same device code (head_tile below: bit-identical logits) and writes
//
//   dlogits[v][j] = round16(gloss[v] * (exp(logit[j] - lse[v]) - lam [j = target_a[v]] - (1 - lam) [j = target_b[v]]))
//
// (the bracket and the product evaluated in double from the fp32 exponential and rounded once: at a
// target the bracket cancels) for vq3d_rows_gemm (dHidden) and vq3d_rows_wgrad (dW, dbias).  lam is a
// device scalar that is read and never written, so a captured step replays with a new value in it.
// Targets are compared against the code index as the tiles go by and never used as addresses: one
// outside [0, k) matches nothing.
//
// Tiling (rows_gemm.hip's): v_mfma_f32_16x16x32, a 64-code tile of W staged in LDS as the A operand
// ([code][c] rows, pitch c + 8 elements: one ds_read_b128 per fragment), the voxel rows the B operand,
// 16 bytes per lane straight from memory, the next k-step's in flight.  The workgroup (4 waves) loops
// the 64-code tiles of k; a lane's accumulator holds 4 consecutive codes of one voxel, and the lane
// carries (max, sum), (best, index) and the two target logits of its codes across the tiles.  The
// four lanes of a voxel meet by two shuffles, the waves sharing a row group through LDS, in a fixed
// order: no atomics, no scratch, bit-identical run to run.
//
// SPLIT waves share 16 rows, each taking 64 / SPLIT codes of every tile, so a workgroup covers
// 64 / SPLIT rows: the host takes the largest row tile (64, 32, 16) that still gives every CU a
// workgroup -- at the published mid level (8,192 rows) 64-row workgroups would fill 128 of 256 CUs,
// 32-row ones fill all of them.  A logit is summed by one wave in k-step order whatever SPLIT is, so
// forward and backward agree bit for bit on it.
#include "launch.h"

#include <cmath>

namespace vq3d {
namespace {

constexpr int HL_N = 64;  // codes per LDS tile
constexpr int HL_KMIN = 8, HL_KMAX = 1024, HL_CMAX = 1024;

struct HlArgs {
    int64_t nrows, ldh, ldw, ldg;
    int C, K, KS, pitch, ntiles;  // hidden width, codes, 32-wide k-steps, LDS row pitch (elements), code tiles
};

// the running softmax statistics, argmax and target logits of a set of codes of one row
struct HlStat {
    float m, s, best, ta, tb;
    int arg;
};

// exp(mi - m) for a running maximum mi <= m; an empty set (mi = -inf) weighs nothing even when m is -inf
__device__ __forceinline__ float hl_weight(float mi, float m) { return mi == -INFINITY ? 0.f : expf(mi - m); }

// x as an fp32 rounded to odd (the last bit is sticky): rounding that to the 16-bit format gives the
// correctly rounded 16-bit value of x, where double -> float -> 16 bit could round twice
__device__ __forceinline__ float hl_to_odd(double x) {
    const float f = float(x);
    const double back = double(f);
    uint32_t b = __float_as_uint(f);
    if (back != x && !(b & 1u)) b += fabs(back) > fabs(x) ? 0xffffffffu : 1u;  // inexact and even: one step towards x
    return __uint_as_float(b);
}

// a (+)= b: the union of two disjoint code sets; the first index wins an argmax tie
__device__ __forceinline__ void hl_merge(HlStat &a, const HlStat &b) {
    const float m = fmaxf(a.m, b.m);
    a.s = a.s * hl_weight(a.m, m) + b.s * hl_weight(b.m, m);
    a.m = m;
    if (b.best > a.best || (b.best == a.best && b.arg < a.arg)) {
        a.best = b.best;
        a.arg = b.arg;
    }
    a.ta += b.ta;  // at most one set holds the target: the other adds an exact zero
    a.tb += b.tb;
}

// Stage code tile n0 .. n0 + 63 of W in LDS and multiply this wave's NT 16-code blocks of it with
// its 16 voxel rows: acc[t][j] = sum_c W[n0 + cw0 + 16 t + 4 kb + j][c] hidden[row col][c] in lane (col, kb).
template <int NT>
__device__ __forceinline__ void head_tile(const HlArgs &a, h16_t *ws, const h16_t *__restrict__ w,
                                          const h16_t *__restrict__ xr, int n0, int cw0, int tid, int col, int kb,
                                          f32x4 (&acc)[NT]) {
    const int kc = a.C / 8;  // 16-byte chunks per W row
    auto ldb = [&](int ks) -> u32x4 {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (32 * ks + 8 * kb < a.C) v = *reinterpret_cast<const u32x4 *>(xr + 32 * ks);
        return v;
    };
    u32x4 bn = ldb(0);  // in flight across the staging
    __syncthreads();    // every wave is done with the previous tile
    for (int i = tid; i < HL_N * kc; i += 256) {
        const int r = i / kc, c = i - r * kc;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (n0 + r < a.K) v = *reinterpret_cast<const u32x4 *>(w + int64_t(n0 + r) * a.ldw + 8 * c);
        *reinterpret_cast<u32x4 *>(ws + r * a.pitch + 8 * c) = v;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < a.KS; ++ks) {
        const hx8 bf = __builtin_bit_cast(hx8, bn);
        if (ks + 1 < a.KS) bn = ldb(ks + 1);
        const int k0 = 32 * ks + 8 * kb;  // k0 >= C: the B chunk is zero and the LDS row tail it meets is zero
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const hx8 af =
                __builtin_bit_cast(hx8, *reinterpret_cast<const u32x4 *>(ws + (cw0 + 16 * t + col) * a.pitch + k0));
            acc[t] = VQ3D_MFMA_16X16X32(af, bf, acc[t], 0, 0, 0);
        }
    }
}

// c <= 256 (the published priors' model_dim): a row's eight k-step fragments stay in registers for
// every code tile, and the next tile of W is loaded into registers (8 chunks per thread) while the
// matrix cores work on the current one, so no tile waits on memory behind a barrier.  At 8,192 rows one
// workgroup per CU has nothing else to hide that latency with.  The k-steps are summed in the same order
// as head_tile's.
constexpr int HL_SKS = 8, HL_SC = 32 * HL_SKS;  // register-resident k-steps; the largest c of this path

__device__ __forceinline__ void stage_load(const HlArgs &a, const h16_t *__restrict__ w, int n0, int tid,
                                           u32x4 (&wr)[HL_SKS]) {
    const int kc = a.C / 8;
#pragma unroll
    for (int u = 0; u < HL_SKS; ++u) {
        const int i = tid + 256 * u, r = i / kc, c = i - r * kc;
        wr[u] = u32x4{0u, 0u, 0u, 0u};
        if (i < HL_N * kc && n0 + r < a.K)
            wr[u] = *reinterpret_cast<const u32x4 *>(w + int64_t(n0 + r) * a.ldw + 8 * c);
    }
}

__device__ __forceinline__ void stage_store(const HlArgs &a, h16_t *ws, int tid, const u32x4 (&wr)[HL_SKS]) {
    const int kc = a.C / 8;
#pragma unroll
    for (int u = 0; u < HL_SKS; ++u) {
        const int i = tid + 256 * u, r = i / kc, c = i - r * kc;
        if (i < HL_N * kc) *reinterpret_cast<u32x4 *>(ws + r * a.pitch + 8 * c) = wr[u];
    }
}

template <int NT>
__device__ __forceinline__ void head_tile_small(const HlArgs &a, h16_t *ws, const h16_t *__restrict__ w, int tile,
                                                int cw0, int tid, int col, int kb, const u32x4 (&br)[HL_SKS],
                                                u32x4 (&wr)[HL_SKS], f32x4 (&acc)[NT]) {
    __syncthreads();  // every wave is done with the previous tile
    stage_store(a, ws, tid, wr);
    __syncthreads();
    if (tile + 1 < a.ntiles) stage_load(a, w, (tile + 1) * HL_N, tid, wr);  // in flight across this tile's products
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < HL_SKS; ++ks) {
        if (ks >= a.KS) break;
        const hx8 bf = __builtin_bit_cast(hx8, br[ks]);
        const int k0 = 32 * ks + 8 * kb;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const hx8 af =
                __builtin_bit_cast(hx8, *reinterpret_cast<const u32x4 *>(ws + (cw0 + 16 * t + col) * a.pitch + k0));
            acc[t] = VQ3D_MFMA_16X16X32(af, bf, acc[t], 0, 0, 0);
        }
    }
}

// two waves per SIMD at least: unbounded, the register-resident variants keep every tile's A fragments in
// flight (250 registers, one wave per SIMD); a bound of three spills
template <int SPLIT, bool BWD, bool SMALLC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_head_loss(
    HlArgs a, const h16_t *__restrict__ hidden, const h16_t *__restrict__ w, const float *__restrict__ bias,
    const int64_t *__restrict__ target_a, const int64_t *__restrict__ target_b, const float *__restrict__ lam_p,
    float *__restrict__ loss, float *__restrict__ lse_out, int32_t *__restrict__ pred,
    const float *__restrict__ lse_in, const float *__restrict__ gloss, h16_t *__restrict__ dlogits) {
    constexpr int CW = HL_N / SPLIT, NT = CW / 16, RG = 4 / SPLIT;  // codes per wave and tile, row groups
    extern __shared__ __attribute__((aligned(16))) char smem[];
    h16_t *ws = reinterpret_cast<h16_t *>(smem);  // [HL_N][pitch]: W[n0 + r][c]
    __shared__ HlStat red[4][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, col = lane & 15, kb = lane >> 4;
    const int rg = wave / SPLIT, part = wave % SPLIT, cw0 = part * CW;
    // the row tails C .. pitch - 1 meet the zero B chunks of the last k-step's lanes past C: they must be
    // finite (zero).  The staging never writes them; head_tile's barriers order these stores.
    for (int i = tid; i < HL_N * (a.pitch - a.C); i += 256) {
        const int r = i / (a.pitch - a.C), c = i - r * (a.pitch - a.C);
        ws[r * a.pitch + a.C + c] = 0;
    }
    const int64_t v = int64_t(blockIdx.x) * (16 * RG) + 16 * rg + col;
    const int64_t vr = min(v, a.nrows - 1);  // this lane's row (clamped: masked at the stores)
    const h16_t *xr = hidden + vr * a.ldh + 8 * kb;
    const float lam = (lam_p && target_b) ? *lam_p : 1.f;
    // the targets as code indices to compare with; -1 (no code) when outside [0, K)
    const int64_t ta64 = target_a[vr], tb64 = target_b ? target_b[vr] : -1;
    const int ta = (ta64 >= 0 && ta64 < a.K) ? int(ta64) : -1, tb = (tb64 >= 0 && tb64 < a.K) ? int(tb64) : -1;
    HlStat st{-INFINITY, 0.f, -INFINITY, 0.f, 0.f, 0x7fffffff};
    float lse_v = 0.f, gl = 0.f;
    if constexpr (BWD) {
        lse_v = lse_in[vr];
        gl = gloss[vr];
    }
    u32x4 br[HL_SKS], wr[HL_SKS];
    if constexpr (SMALLC) {
#pragma unroll
        for (int ks = 0; ks < HL_SKS; ++ks) {
            br[ks] = u32x4{0u, 0u, 0u, 0u};
            if (32 * ks + 8 * kb < a.C) br[ks] = *reinterpret_cast<const u32x4 *>(xr + 32 * ks);
        }
        stage_load(a, w, 0, tid, wr);
    }
    for (int tile = 0; tile < a.ntiles; ++tile) {
        const int n0 = tile * HL_N;
        f32x4 acc[NT];
        if constexpr (SMALLC)
            head_tile_small<NT>(a, ws, w, tile, cw0, tid, col, kb, br, wr, acc);
        else
            head_tile<NT>(a, ws, w, xr, n0, cw0, tid, col, kb, acc);
        // lane (col, kb) holds codes n .. n + 3 of its row; K % 8 == 0: the four are inside or outside together
        if constexpr (!BWD) {
            float x[NT][4], tmax = -INFINITY;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int n = n0 + cw0 + 16 * t + 4 * kb;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[t][j] = -INFINITY;
                    if (n < a.K) {
                        const float xv = acc[t][j] + bias[n + j];
                        x[t][j] = xv;
                        if (xv > st.best) {  // codes in ascending order: the first of equal logits stays
                            st.best = xv;
                            st.arg = n + j;
                        }
                        st.ta += (n + j == ta) ? xv : 0.f;
                        st.tb += (n + j == tb) ? xv : 0.f;
                    }
                    tmax = fmaxf(tmax, x[t][j]);
                }
            }
            if (tmax > -INFINITY) {
                const float m = fmaxf(st.m, tmax);
                float s = st.s * hl_weight(st.m, m);
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) s += expf(x[t][j] - m);  // exp(-inf) = 0 for the codes past K
                st.m = m;
                st.s = s;
            }
        } else {
            if (v < a.nrows) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int n = n0 + cw0 + 16 * t + 4 * kb;
                    if (n >= a.K) continue;
                    float d[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xv = acc[t][j] + bias[n + j];
                        // at a target p - lam cancels: the bracket and the product in double, one rounding
                        const double in = double(expf(xv - lse_v)) - ((n + j == ta) ? double(lam) : 0.0) -
                                          ((n + j == tb) ? 1.0 - double(lam) : 0.0);
                        d[j] = hl_to_odd(double(gl) * in);
                    }
                    *reinterpret_cast<u32x2 *>(dlogits + v * a.ldg + n) = u32x2{pk2(d[0], d[1]), pk2(d[2], d[3])};
                }
            }
        }
    }
    if constexpr (!BWD) {
        // the row's four lanes (kb = 0 .. 3), then the waves sharing the row group, in a fixed order
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            HlStat ot;
            ot.m = __shfl_xor(st.m, o, kWave);
            ot.s = __shfl_xor(st.s, o, kWave);
            ot.best = __shfl_xor(st.best, o, kWave);
            ot.ta = __shfl_xor(st.ta, o, kWave);
            ot.tb = __shfl_xor(st.tb, o, kWave);
            ot.arg = __shfl_xor(st.arg, o, kWave);
            hl_merge(st, ot);
        }
        if constexpr (SPLIT > 1) {
            if (kb == 0) red[wave][col] = st;
            __syncthreads();
            if (part == 0 && kb == 0) {
#pragma unroll
                for (int p = 1; p < SPLIT; ++p) hl_merge(st, red[wave + p][col]);
            }
        }
        if (part == 0 && kb == 0 && v < a.nrows) {
            const float l = st.m + logf(st.s);
            lse_out[v] = l;
            loss[v] = float(double(l) - double(lam) * double(st.ta) - (1.0 - double(lam)) * double(st.tb));
            pred[v] = st.arg == 0x7fffffff ? 0 : st.arg;  // no logit compared greater than -inf (all NaN)
        }
    }
}

template <int SPLIT, bool BWD, bool SMALLC>
void launch_split_c(const HlArgs &a, const void *hidden, const void *w, const float *bias, const int64_t *ta,
                  const int64_t *tb, const float *lam, float *loss, float *lse_out, int32_t *pred, const float *lse_in,
                  const float *gloss, void *dlogits, hipStream_t s) {
    const size_t lds = size_t(HL_N) * a.pitch * sizeof(h16_t);
    // above 64 KB of dynamic LDS (c > 472) the kernel must opt in (gfx950: 160 KB per workgroup)
    constexpr size_t kLdsOptIn = size_t(HL_N) * (HL_CMAX + 8) * sizeof(h16_t);
    opt_in_lds(k_head_loss<SPLIT, BWD, SMALLC>, kLdsOptIn);
    const int rows = 64 / SPLIT;
    const unsigned grid = unsigned((a.nrows + rows - 1) / rows);
    k_head_loss<SPLIT, BWD, SMALLC><<<grid, 256, lds, s>>>(a, (const h16_t *)hidden, (const h16_t *)w, bias, ta, tb,
                                                           lam, loss, lse_out, pred, lse_in, gloss, (h16_t *)dlogits);
}

template <int SPLIT, bool BWD>
void launch_split(const HlArgs &a, const void *hidden, const void *w, const float *bias, const int64_t *ta,
                  const int64_t *tb, const float *lam, float *loss, float *lse_out, int32_t *pred, const float *lse_in,
                  const float *gloss, void *dlogits, hipStream_t s) {
    if (a.C <= HL_SC)
        launch_split_c<SPLIT, BWD, true>(a, hidden, w, bias, ta, tb, lam, loss, lse_out, pred, lse_in, gloss, dlogits,
                                         s);
    else
        launch_split_c<SPLIT, BWD, false>(a, hidden, w, bias, ta, tb, lam, loss, lse_out, pred, lse_in, gloss, dlogits,
                                          s);
}

template <bool BWD>
int launch_head_loss(int32_t dtype, int64_t nrows, int c, int k, const void *hidden, int64_t ldh, const void *w,
                     int64_t ldw, const float *bias, const int64_t *ta, const int64_t *tb, const float *lam,
                     float *loss, float *lse_out, int32_t *pred, const float *lse_in, const float *gloss,
                     void *dlogits, int64_t ldg, hipStream_t s) {
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    if (dtype != VQ3D_HALF) return fail("prior_head_loss: hidden and weight must be bf16 or fp16 (16-bit dtypes only)");
    if (k < HL_KMIN || k > HL_KMAX || k % 8) return fail("prior_head_loss: 8 <= k <= 1024 and k % 8 == 0");
    if (c < 8 || c > HL_CMAX || c % 8) return fail("prior_head_loss: c must be a multiple of 8, at most 1024");
    if (nrows < 1 || nrows > (int64_t(1) << 31) - 64) return fail("prior_head_loss: bad row count");
    if (ldh % 8 || ldw % 8 || ldh < c || ldw < c || (BWD && (ldg % 8 || ldg < k)))
        return fail("prior_head_loss: row strides must be multiples of 8 and at least the row length");
    if (!hidden || !w || !bias || !ta) return fail("prior_head_loss: null pointer");
    if (BWD ? (!lse_in || !gloss || !dlogits) : (!loss || !lse_out || !pred))
        return fail("prior_head_loss: null pointer");
    if (!al(hidden) || !al(w) || (BWD && !al(dlogits)))
        return fail("prior_head_loss: hidden, weight and dlogits must be 16-byte aligned");
    HlArgs a;
    a.nrows = nrows;
    a.ldh = ldh;
    a.ldw = ldw;
    a.ldg = ldg;
    a.C = c;
    a.K = k;
    a.KS = (c + 31) / 32;
    a.pitch = 32 * a.KS + 8;  // every k-step's fragment inside the row; +8: rows off the bank period
    a.ntiles = (k + HL_N - 1) / HL_N;
    // the largest row tile that still gives every CU a workgroup
    const int64_t cus = n_cu();
    if ((nrows + 63) / 64 >= cus)
        launch_split<1, BWD>(a, hidden, w, bias, ta, tb, lam, loss, lse_out, pred, lse_in, gloss, dlogits, s);
    else if ((nrows + 31) / 32 >= cus)
        launch_split<2, BWD>(a, hidden, w, bias, ta, tb, lam, loss, lse_out, pred, lse_in, gloss, dlogits, s);
    else
        launch_split<4, BWD>(a, hidden, w, bias, ta, tb, lam, loss, lse_out, pred, lse_in, gloss, dlogits, s);
    return check_launch(BWD ? "prior_head_loss_bwd" : "prior_head_loss_fwd");
}

}  // namespace
}  // namespace vq3d

using namespace vq3d;

extern "C" {

int vq3d_prior_head_loss_fwd(int32_t dtype, int64_t nrows, int32_t c, int32_t k, const void *hidden, int64_t ldh,
                             const void *weight, int64_t ldw, const float *bias, const int64_t *target_a,
                             const int64_t *target_b, const float *lam, float *loss, float *lse, int32_t *pred,
                             vq3d_stream_t stream) {
    return launch_head_loss<false>(dtype, nrows, c, k, hidden, ldh, weight, ldw, bias, target_a, target_b, lam, loss,
                                   lse, pred, nullptr, nullptr, nullptr, 0, as_stream(stream));
}

int vq3d_prior_head_loss_bwd(int32_t dtype, int64_t nrows, int32_t c, int32_t k, const void *hidden, int64_t ldh,
                             const void *weight, int64_t ldw, const float *bias, const int64_t *target_a,
                             const int64_t *target_b, const float *lam, const float *lse, const float *gloss,
                             void *dlogits, int64_t ldg, vq3d_stream_t stream) {
    return launch_head_loss<true>(dtype, nrows, c, k, hidden, ldh, weight, ldw, bias, target_a, target_b, lam, nullptr,
                                  nullptr, nullptr, lse, gloss, dlogits, ldg, as_stream(stream));
}

}  // extern "C"
