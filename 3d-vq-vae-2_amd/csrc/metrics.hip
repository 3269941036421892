// Validation metrics of a reconstruction: slice-wise SSIM (the reference's SSIM3DSlices,
// metrics/evaluate.py:27-36, with PL 1.2's ssim at kernel 11x11, sigma 1.5), NMSE and PSNR
// (metrics/evaluate.py:18-24), fused into one pass over the decoder output and the target.
//
// Volumes are (B, 1, H, W, D) with D innermost; every (b, d) is one 2-D slice over (h, w).  The
// Gaussian window is separable: the w-filter is an 11-tap filter at stride D, the h-filter one at
// stride W D.  A workgroup (512 threads) owns kTW output columns x kTD consecutive d x a segment of
// output rows and marches down h:
//   * each input row of the tile (kTW + 10 columns x kTD d) is loaded once, activated (ELU) and
//     masked (d >= nvs[b] -> 0) as k_recon_fwd does, and staged in LDS (two buffers, one barrier
//     per row; the next row's global loads are issued before the barrier).  The squared-error and
//     target-energy sums are taken here, each input voxel counted by exactly one workgroup;
//   * lane = d, wave = a group of kE output columns: a thread runs the w-filter for its kE columns
//     of the five quantities (p, t, p^2, t^2, p t) from LDS into registers;
//   * the h-filter lives in registers: 11 running accumulators per quantity and column, accumulator
//     s collecting output row r with r % 11 == s.  The row loop is unrolled by 11 so every
//     accumulator index and tap weight is a compile-time constant; the accumulator that receives
//     its 11th row yields that row's SSIM values.
// A thread only ever sees one d, so its SSIM sum is a partial sum of one slice: the eight waves'
// sums are added through LDS and stored per (tile, segment, b, d); a finishing kernel adds the
// partials in a fixed order in double.  No atomics, no host synchronisation.
#include "block_util.h"
#include "common.h"
#include "launch.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace vq3d {
namespace {

constexpr int kWin = 11, kHalo = kWin - 1;
constexpr int kNT = 512;                   // threads of a workgroup
constexpr int kE = 2;                      // output columns per thread: 110 accumulator registers, so the
                                           // workgroup's 8 waves sit two to a SIMD (4 columns at 256 threads
                                           // needed 284 registers, one wave per SIMD: measured 1.3x slower)
constexpr int kTD = 64;                    // d per tile: one per lane
constexpr int kTW = (kNT / 64) * kE;       // output columns per tile
constexpr int kCols = kTW + kHalo;         // input columns per tile
constexpr int kTargetWgs = 256;            // H is cut into segments until the grid has about this many:
                                           // one workgroup per CU is resident (registers), so one wave of them
constexpr int kMinSegRows = 32;            // ... but no segment shorter than this (10 rows of overlap each)
constexpr int kRangeBlocks = 1024;
constexpr int kHead = 16;                  // floats in front of the workspace: [0] the computed data range

typedef float f2 __attribute__((ext_vector_type(2)));

// f(integral_constant<I>) ... f(integral_constant<N - 1>): a loop whose index is a constant expression
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

struct Taps {
    float g[kWin];
};

struct Plan {
    int n_dt, n_wt, nseg, seg_rows;
    int64_t tiles() const { return int64_t(n_dt) * n_wt * nseg; }
};

Plan make_plan(int B, int H, int W, int D) {
    Plan p;
    p.n_dt = (D + kTD - 1) / kTD;
    p.n_wt = (W - kHalo + kTW - 1) / kTW;
    const int rows = H - kHalo;
    const int64_t tiles = int64_t(B) * p.n_dt * p.n_wt;
    const int64_t want = std::max<int64_t>(1, (kTargetWgs + tiles - 1) / tiles);
    const int nseg = int(std::min<int64_t>(want, std::max(1, rows / kMinSegRows)));
    p.seg_rows = (rows + nseg - 1) / nseg;
    p.nseg = (rows + p.seg_rows - 1) / p.seg_rows;
    return p;
}

// ---------------------------------------------------------------- data range (optional first pass)
template <typename T>
__global__ __launch_bounds__(256) void k_metrics_range(const T *__restrict__ pred, const float *__restrict__ tgt,
                                                      const int64_t *__restrict__ nvs, int64_t n, int64_t per_b,
                                                      int D, int act, float *__restrict__ part) {
    __shared__ float red[4][4];
    float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
        const int d = int(i % D);
        const int b = int(i / per_b);
        float p = ld(pred + i);
        if (act) p = elu_fast(p);
        if (d >= nvs[b]) p = 0.f;
        const float t = tgt[i];
        pmin = fminf(pmin, p);
        pmax = fmaxf(pmax, p);
        tmin = fminf(tmin, t);
        tmax = fmaxf(tmax, t);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pmin = fminf(pmin, __shfl_xor(pmin, o, 64));
        pmax = fmaxf(pmax, __shfl_xor(pmax, o, 64));
        tmin = fminf(tmin, __shfl_xor(tmin, o, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, o, 64));
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) {
        red[wid][0] = pmin;
        red[wid][1] = pmax;
        red[wid][2] = tmin;
        red[wid][3] = tmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            pmin = fminf(pmin, red[k][0]);
            pmax = fmaxf(pmax, red[k][1]);
            tmin = fminf(tmin, red[k][2]);
            tmax = fmaxf(tmax, red[k][3]);
        }
        float *o = part + int64_t(blockIdx.x) * 4;
        o[0] = pmin;
        o[1] = pmax;
        o[2] = tmin;
        o[3] = tmax;
    }
}

// one workgroup: R = max(max p - min p, max t - min t) from the blocks' extremes
__global__ __launch_bounds__(256) void k_metrics_range_fin(const float *__restrict__ part, int nb,
                                                          float *__restrict__ range) {
    __shared__ float red[256][4];
    float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
    for (int j = threadIdx.x; j < nb; j += 256) {
        pmin = fminf(pmin, part[4 * j]);
        pmax = fmaxf(pmax, part[4 * j + 1]);
        tmin = fminf(tmin, part[4 * j + 2]);
        tmax = fmaxf(tmax, part[4 * j + 3]);
    }
    red[threadIdx.x][0] = pmin;
    red[threadIdx.x][1] = pmax;
    red[threadIdx.x][2] = tmin;
    red[threadIdx.x][3] = tmax;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 256; ++k) {
            pmin = fminf(pmin, red[k][0]);
            pmax = fmaxf(pmax, red[k][1]);
            tmin = fminf(tmin, red[k][2]);
            tmax = fmaxf(tmax, red[k][3]);
        }
        *range = fmaxf(pmax - pmin, tmax - tmin);
    }
}

// ---------------------------------------------------------------- the fused pass
// How a thread takes part in staging one input row of the tile: N consecutive d of one column per
// step (VEC: 4, as one 8- or 16-byte load; D % 4 == 0 and aligned bases), IT steps per row.
template <bool VEC>
struct Stage {
    static constexpr int N = VEC ? 4 : 1;
    static constexpr int TPC = kTD / N;                   // threads per column
    static constexpr int CPI = kNT / TPC;                 // columns per step
    static constexpr int IT = (kCols + CPI - 1) / CPI;    // steps per row
};

template <typename T, bool VEC>
__global__ __launch_bounds__(kNT) void k_slice_metrics(const T *__restrict__ pred, const float *__restrict__ tgt,
                                                      const int64_t *__restrict__ nvs, int B, int H, int W, int D,
                                                      int act, int cyl, Taps taps, float r_host,
                                                      const float *__restrict__ r_dev, float k1, float k2, Plan pl,
                                                      float *__restrict__ ssim_part, float *__restrict__ mse_part) {
    using S = Stage<VEC>;
    __shared__ float lds[2][2][kCols * kTD];  // [buffer][p | t][column][d]
    __shared__ float red[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int bx = blockIdx.x;
    const int seg = bx % pl.nseg;
    bx /= pl.nseg;
    const int iw = bx % pl.n_wt, id = bx / pl.n_wt;
    const int b = blockIdx.y;
    const int w0 = iw * kTW, d0 = id * kTD;
    const int r0 = seg * pl.seg_rows, r1 = min(H - kHalo, r0 + pl.seg_rows);
    const int nrows = r1 - r0 + kHalo;  // input rows r0 .. r1 + 9
    // the input voxels this workgroup counts in the error sums: its own columns and rows, the last
    // tile / segment also the 10 trailing ones
    const int own_w1 = iw == pl.n_wt - 1 ? W : w0 + kTW;
    const int own_h1 = seg == pl.nseg - 1 ? H : r1;
    const int64_t nvb = nvs[b];
    const float R = r_dev ? *r_dev : r_host;
    const float c1 = (k1 * R) * (k1 * R), c2 = (k2 * R) * (k2 * R);

    // staging coordinates of this thread
    const int s_col = tid / S::TPC, s_dl = (tid % S::TPC) * S::N;
    const int64_t base_b = int64_t(b) * H * W * D;
    Raw<T, S::N> rp[S::IT];
    Raw<float, S::N> rt[S::IT];
    float sse = 0.f, st2 = 0.f;

    auto load_row = [&](int h) {
#pragma unroll
        for (int k = 0; k < S::IT; ++k) {
            const int col = s_col + k * S::CPI, w = w0 + col, d = d0 + s_dl;
            if (col < kCols && w < W && d < D) {
                const int64_t off = base_b + (int64_t(h) * W + w) * D + d;
                rp[k] = ldraw<T, S::N>(pred + off);
                rt[k] = ldraw<float, S::N>(tgt + off);
            } else {
#pragma unroll
                for (int j = 0; j < Raw<T, S::N>::W; ++j) rp[k].w[j] = 0u;
#pragma unroll
                for (int j = 0; j < Raw<float, S::N>::W; ++j) rt[k].w[j] = 0u;
            }
        }
    };
    auto commit_row = [&](int h, float *bp, float *bt) {
#pragma unroll
        for (int k = 0; k < S::IT; ++k) {
            const int col = s_col + k * S::CPI, w = w0 + col;
            if (col >= kCols) continue;
            float pv[S::N], tv[S::N];
            unraw<T, S::N>(rp[k], pv);
            unraw<float, S::N>(rt[k], tv);
            const bool counted = w < own_w1 && h < own_h1 && (!cyl || in_cylinder(h, w, H, W));
#pragma unroll
            for (int j = 0; j < S::N; ++j) {
                const int d = d0 + s_dl + j;
                float p = act ? elu_fast(pv[j]) : pv[j];
                if (d >= nvb) p = 0.f;
                pv[j] = p;
                if (counted && d < D) {  // out-of-volume positions hold zeros and count nothing
                    const float df = p - tv[j];
                    sse = fmaf(df, df, sse);
                    st2 = fmaf(tv[j], tv[j], st2);
                }
            }
            if constexpr (VEC) {
                *reinterpret_cast<float4 *>(bp + col * kTD + s_dl) = float4{pv[0], pv[1], pv[2], pv[3]};
                *reinterpret_cast<float4 *>(bt + col * kTD + s_dl) = float4{tv[0], tv[1], tv[2], tv[3]};
            } else {
                bp[col * kTD + s_dl] = pv[0];
                bt[col * kTD + s_dl] = tv[0];
            }
        }
    };

    // which of this thread's kE output columns exist
    bool valid[kE];
#pragma unroll
    for (int e = 0; e < kE; ++e) valid[e] = (w0 + wv * kE + e < W - kHalo) && (d0 + lane < D);

    f2 acc[kWin][5][kE / 2];
#pragma unroll
    for (int s = 0; s < kWin; ++s)
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int e = 0; e < kE / 2; ++e) acc[s][q][e] = f2{0.f, 0.f};
    float ssum = 0.f;

    // one input row i of the segment, at phase i % 11 of the accumulator rotation
    auto row_step = [&](auto phase, int i) __attribute__((always_inline)) {
        constexpr int ph = decltype(phase)::value;
        float *bp = lds[i & 1][0], *bt = lds[i & 1][1];
        commit_row(r0 + i, bp, bt);
        if (i + 1 < nrows) load_row(r0 + i + 1);
        __syncthreads();
        // w-filter of the five quantities for this thread's kE columns
        f2 v[5][kE / 2];
#pragma unroll
        for (int q = 0; q < 5; ++q)
#pragma unroll
            for (int e = 0; e < kE / 2; ++e) v[q][e] = f2{0.f, 0.f};
        const float *cp = bp + wv * kE * kTD + lane, *ct = bt + wv * kE * kTD + lane;
#pragma unroll
        for (int cc = 0; cc < kE + kHalo; ++cc) {
            const float p = cp[cc * kTD], t = ct[cc * kTD];
            const float pp = p * p, tt = t * t, pt = p * t;
#pragma unroll
            for (int e = 0; e < kE / 2; ++e) {
                const int ka = cc - 2 * e, kb = ka - 1;  // taps of columns 2e and 2e + 1
                const bool ia = ka >= 0 && ka < kWin, ib = kb >= 0 && kb < kWin;
                if (!ia && !ib) continue;
                const f2 g = f2{ia ? taps.g[ia ? ka : 0] : 0.f, ib ? taps.g[ib ? kb : 0] : 0.f};
                v[0][e] += g * p;
                v[1][e] += g * t;
                v[2][e] += g * pp;
                v[3][e] += g * tt;
                v[4][e] += g * pt;
            }
        }
        // h-filter: input row i is tap k of output row i - k, held by accumulator (i - k) % 11
#pragma unroll
        for (int s = 0; s < kWin; ++s) {
            const int k = (ph - s + kWin) % kWin;
            const float g = taps.g[k];
#pragma unroll
            for (int q = 0; q < 5; ++q)
#pragma unroll
                for (int e = 0; e < kE / 2; ++e)
                    acc[s][q][e] = k == 0 ? g * v[q][e] : acc[s][q][e] + g * v[q][e];
            if (k == kHalo && i >= kHalo) {  // output row r0 + i - 10 is complete
#pragma unroll
                for (int e = 0; e < kE; ++e) {
                    const float mp = acc[s][0][e / 2][e & 1], mt = acc[s][1][e / 2][e & 1];
                    const float spp = acc[s][2][e / 2][e & 1] - mp * mp;
                    const float stt = acc[s][3][e / 2][e & 1] - mt * mt;
                    const float spt = acc[s][4][e / 2][e & 1] - mp * mt;
                    const float num = (2.f * mp * mt + c1) * (2.f * spt + c2);
                    const float den = (mp * mp + mt * mt + c1) * (spp + stt + c2);
                    const float sv = num * __builtin_amdgcn_rcpf(den);
                    ssum += valid[e] ? sv : 0.f;
                }
            }
        }
    };
    load_row(r0);
    for (int i0 = 0; i0 < nrows; i0 += kWin)
        static_for<0, kWin>([&](auto phase) __attribute__((always_inline)) {
            const int i = i0 + decltype(phase)::value;
            if (i < nrows) row_step(phase, i);  // the same in every thread of the workgroup
        });

    // the slice partial: the waves' sums of one d, in wave order
    __syncthreads();
    float *sred = lds[0][0];
    sred[wv * kTD + lane] = ssum;
    __syncthreads();
    if (wv == 0 && d0 + lane < D) {
        float t = sred[lane];
#pragma unroll
        for (int k = 1; k < kNT / 64; ++k) t += sred[k * kTD + lane];
        ssim_part[(int64_t(iw) * pl.nseg + seg) * (int64_t(B) * D) + int64_t(b) * D + d0 + lane] = t;
    }
    float ss[2] = {sse, st2};
    block_sums<float, kNT, 2, 8>(ss, red);
    if (tid == 0) {
        float *o = mse_part + (int64_t(blockIdx.y) * gridDim.x + blockIdx.x) * 2;
        o[0] = ss[0];
        o[1] = ss[1];
    }
}

// One workgroup: the per-slice means and the scalars from the partials, fixed order, in double.
// stats = {ssim, mse, nmse, psnr, data_range_used}
__global__ __launch_bounds__(256) void k_metrics_fin(const float *__restrict__ ssim_part, int nparts, int nslices,
                                                    double inv_nwin, const float *__restrict__ mse_part, int64_t nwg,
                                                    double count, float r_host, const float *__restrict__ r_dev,
                                                    float psnr_range, float *__restrict__ per_slice,
                                                    float *__restrict__ stats) {
    __shared__ double red[4];
    const float R = r_dev ? *r_dev : r_host;
    const bool flat = !(R > 0.f);  // a computed range of 0: both volumes constant, the formula is 0 / 0
    double tot = 0.0;
    for (int s = threadIdx.x; s < nslices; s += 256) {
        double a = 0.0;
        for (int j = 0; j < nparts; ++j) a += double(ssim_part[int64_t(j) * nslices + s]);
        const double m = flat ? double(NAN) : a * inv_nwin;
        per_slice[s] = float(m);
        tot += m;
    }
    tot = block_sum<double, 256>(tot, red);
    double e = 0.0, q = 0.0;
    for (int64_t j = threadIdx.x; j < nwg; j += 256) {
        e += double(mse_part[2 * j]);
        q += double(mse_part[2 * j + 1]);
    }
    e = block_sum<double, 256>(e, red);
    q = block_sum<double, 256>(q, red);
    if (threadIdx.x == 0) {
        const double mse = e / count;
        stats[0] = float(tot / double(nslices));
        stats[1] = float(mse);
        stats[2] = float(e / q);
        stats[3] = float(10.0 * log10(double(psnr_range) * double(psnr_range) / mse));
        stats[4] = R;
    }
}

struct Layout {
    Plan plan;
    int64_t nwg, nparts, nslices;
    size_t range_off, mse_off, ssim_off, floats;
};

Layout make_layout(int B, int H, int W, int D) {
    Layout l;
    l.plan = make_plan(B, H, W, D);
    l.nwg = l.plan.tiles() * B;
    l.nparts = int64_t(l.plan.n_wt) * l.plan.nseg;
    l.nslices = int64_t(B) * D;
    l.range_off = kHead;
    l.mse_off = l.range_off + size_t(kRangeBlocks) * 4;
    l.ssim_off = l.mse_off + size_t(l.nwg) * 2;
    l.floats = l.ssim_off + size_t(l.nparts) * size_t(l.nslices);
    return l;
}

bool sizes_ok(int32_t batch, int32_t h, int32_t w, int32_t dd) {
    return batch > 0 && batch <= 65535 && h >= kWin && w >= kWin && dd > 0 &&
           int64_t(batch) * dd <= INT32_MAX && make_plan(batch, h, w, dd).tiles() <= INT32_MAX;
}

template <typename T>
int launch(const T *pred, const float *target, const int64_t *nvs, int B, int H, int W, int D, int act, int cyl,
           float data_range, float k1, float k2, float psnr_range, float *per_slice, float *stats, float *ws,
           hipStream_t s) {
    const Layout l = make_layout(B, H, W, D);
    const int64_t n = int64_t(B) * H * W * D;
    const float *r_dev = nullptr;
    if (!(data_range > 0.f)) {
        const int nb = int(std::min<int64_t>(kRangeBlocks, (n + 255) / 256));
        k_metrics_range<T><<<nb, 256, 0, s>>>(pred, target, nvs, n, int64_t(H) * W * D, D, act, ws + l.range_off);
        k_metrics_range_fin<<<1, 256, 0, s>>>(ws + l.range_off, nb, ws);
        r_dev = ws;
    }
    Taps taps;
    double g[kWin], sum = 0.0;
    for (int i = 0; i < kWin; ++i) {
        const double x = (i - kWin / 2) / 1.5;
        sum += g[i] = std::exp(-0.5 * x * x);
    }
    for (int i = 0; i < kWin; ++i) taps.g[i] = float(g[i] / sum);
    const dim3 grid(unsigned(l.plan.tiles()), unsigned(B));
    const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(pred) & 15) == 0 &&
                     (reinterpret_cast<uintptr_t>(target) & 15) == 0;
    if (vec)
        k_slice_metrics<T, true><<<grid, kNT, 0, s>>>(pred, target, nvs, B, H, W, D, act, cyl, taps, data_range, r_dev,
                                                     k1, k2, l.plan, ws + l.ssim_off, ws + l.mse_off);
    else
        k_slice_metrics<T, false><<<grid, kNT, 0, s>>>(pred, target, nvs, B, H, W, D, act, cyl, taps, data_range,
                                                      r_dev, k1, k2, l.plan, ws + l.ssim_off, ws + l.mse_off);
    const double nwin = double(H - kHalo) * double(W - kHalo);
    const double cnt = double(B) * D * double(cyl ? vq3d_cylinder_count(H, W) : int64_t(H) * W);
    k_metrics_fin<<<1, 256, 0, s>>>(ws + l.ssim_off, int(l.nparts), int(l.nslices), 1.0 / nwin, ws + l.mse_off, l.nwg,
                                    cnt, data_range, r_dev, psnr_range, per_slice, stats);
    return check_launch("slice_metrics");
}

}  // namespace
}  // namespace vq3d

using namespace vq3d;

extern "C" {

size_t vq3d_slice_metrics_workspace_size(int32_t batch, int32_t h, int32_t w, int32_t dd) {
    if (!sizes_ok(batch, h, w, dd)) return 0;
    return make_layout(batch, h, w, dd).floats * sizeof(float);
}

int vq3d_slice_metrics(int32_t dtype, const void *pred, const float *target, const int64_t *nvs, int32_t batch,
                       int32_t h, int32_t w, int32_t dd, int32_t activation, int32_t cylinder, float data_range,
                       float k1, float k2, float psnr_range, float *ssim_per_slice, float *stats, void *workspace,
                       vq3d_stream_t stream) {
    if (dtype != VQ3D_F32 && dtype != VQ3D_HALF) return fail("slice_metrics: dtype must be fp32 or this build's 16-bit format");
    if (batch <= 0 || h <= 0 || w <= 0 || dd <= 0) return fail("slice_metrics: bad sizes");
    if (h < kWin || w < kWin) return fail("slice_metrics: H and W must be at least 11 (the SSIM window)");
    if (!sizes_ok(batch, h, w, dd)) return fail("slice_metrics: batch <= 65535 and batch * D < 2^31");
    if (!pred || !target || !nvs || !ssim_per_slice || !stats || !workspace) return fail("slice_metrics: null pointer");
    if (activation != 0 && activation != 1) return fail("slice_metrics: activation is 0 (none) or 1 (ELU)");
    if (!(k1 >= 0.f) || !(k2 >= 0.f)) return fail("slice_metrics: k1 and k2 must not be negative");
    if (!(psnr_range > 0.f)) return fail("slice_metrics: psnr_range must be positive");
    hipStream_t s = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    if (dtype == VQ3D_F32)
        return launch<float>(static_cast<const float *>(pred), target, nvs, batch, h, w, dd, activation, cylinder != 0,
                             data_range, k1, k2, psnr_range, ssim_per_slice, stats, ws, s);
    return launch<h16_t>(static_cast<const h16_t *>(pred), target, nvs, batch, h, w, dd, activation, cylinder != 0,
                         data_range, k1, k2, psnr_range, ssim_per_slice, stats, ws, s);
}

}  // extern "C"
