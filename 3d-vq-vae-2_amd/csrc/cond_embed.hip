// The conditioned PixelCNN prior's condition embedding (include/vq3d.h: vq3d_cond_embed_*): one-hot,
// trilinear interpolation and embed_condition's 1x1x1 conv are all linear, so e is a trilinear blend of
// eight rows of the [kc][m] table per voxel (sixteen with mixup).  The forward is bound by its output
// stream: one thread per (voxel, 8 channels), 16-byte loads of table rows (<= 1 MiB, L2 resident), fp32
// accumulation, one 16-byte (32-byte in fp32) store.  The backward is two launches, no atomics:
// k_cond_gather, the adjoint interpolation in gather form into an fp32 [b][coarse][m] workspace, then
// k_cond_scatter, one workgroup per code summing its rows in index order (and m / 32 more the bias sums).
#include "common.h"
#include <algorithm>

namespace vq3d {
namespace {

constexpr int CE_KMIN = 8, CE_KMAX = 1024, CE_MMAX = 1024, CE_AXIS_MAX = 1 << 20;

// one axis of ATen's align_corners = False source index, in fp32 with no contraction into an fma
struct Axis {
    int i0, i1;
    float t0, t1;
};
__device__ __forceinline__ Axis axis_coeff(int o, int n_in, float s) {
    float src = __fsub_rn(__fmul_rn(s, float(o) + 0.5f), 0.5f);
    if (src < 0.f) src = 0.f;
    Axis a;
    a.i0 = min(int(src), n_in - 1);
    a.i1 = a.i0 + (a.i0 < n_in - 1 ? 1 : 0);
    a.t1 = __fsub_rn(src, float(a.i0));
    a.t0 = __fsub_rn(1.f, a.t1);
    return a;
}
// the weight of coarse index c in fine index o's pair
__device__ __forceinline__ float axis_weight(const Axis &a, int c) {
    return (a.i0 == c ? a.t0 : 0.f) + (a.i1 == c ? a.t1 : 0.f);
}
// a superset [lo, hi] of the fine indices whose pair holds coarse index c: floor(src) is c - 1 or c, i.e.
// (c - 0.5) / s - 0.5 <= o < (c + 1.5) / s - 0.5, the bounds in double (exact to far below one index for the
// axis lengths check_geo admits) with one spare index either side against src's own fp32 rounding; the
// weights themselves come from axis_coeff
__device__ __forceinline__ void axis_range(int c, int n_in, int n_out, float s, int &lo, int &hi) {
    const double inv = 1.0 / double(s);
    lo = c == 0 ? 0 : max(0, int(floor((double(c) - 0.5) * inv - 0.5)) - 1);
    hi = c == n_in - 1 ? n_out - 1 : min(n_out - 1, int(ceil((double(c) + 1.5) * inv - 0.5)) + 1);
}

struct Geo {
    int b, cd, ch, cw, d, h, w, d_out, m, kc;
    float sz, sy, sx;
};

// the sample mixed into sample bb: index[bb], or bb itself (no mixing) when that is no sample of the batch --
// never an address the batch does not have, and the two weights of a sample always sum to 1
__device__ __forceinline__ int64_t mix_source(const int64_t *index, int bb, int b) {
    const int64_t src = index[bb];
    return uint64_t(src) < uint64_t(b) ? src : int64_t(bb);
}

template <typename T>
__device__ __forceinline__ void add_row(float (&acc)[8], const T *__restrict__ table, int64_t code, int kc, int m,
                                        int c0, float wgt) {
    if (uint64_t(code) >= uint64_t(kc) || wgt == 0.f) return;
    float r[8];
    ldvec<T, 8>(table + int64_t(code) * m + c0, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = fmaf(wgt, r[j], acc[j]);
}

template <typename T>
__device__ __forceinline__ void blend8(float (&acc)[8], const T *__restrict__ table, const int64_t *__restrict__ cs,
                                       const Geo &q, const Axis &az, const Axis &ay, const Axis &ax, int c0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int iz = (j & 4) ? az.i1 : az.i0, iy = (j & 2) ? ay.i1 : ay.i0, ix = (j & 1) ? ax.i1 : ax.i0;
        const float wgt = ((j & 4) ? az.t1 : az.t0) * ((j & 2) ? ay.t1 : ay.t0) * ((j & 1) ? ax.t1 : ax.t0);
        add_row<T>(acc, table, cs[(int64_t(iz) * q.ch + iy) * q.cw + ix], q.kc, q.m, c0, wgt);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_cond_fwd(Geo q, int64_t items, const int64_t *__restrict__ codes,
                                                  const T *__restrict__ table, const float *__restrict__ bias,
                                                  const float *lam, const int64_t *index, T *__restrict__ e) {
    const int mg = q.m >> 3;
    const int64_t ncoarse = int64_t(q.cd) * q.ch * q.cw;
    for (int64_t it = int64_t(blockIdx.x) * 256 + threadIdx.x; it < items; it += int64_t(gridDim.x) * 256) {
        const int c0 = int(it % mg) * 8;
        uint32_t v = uint32_t(it / mg);  // voxel of the [b][d_out][h][w] output (< 2^31: check_geo)
        const int x = int(v % q.w);
        v /= q.w;
        const int y = int(v % q.h);
        v /= q.h;
        const int z = int(v % q.d_out), bb = int(v / q.d_out);
        const Axis az = axis_coeff(z, q.cd, q.sz), ay = axis_coeff(y, q.ch, q.sy), ax = axis_coeff(x, q.cw, q.sx);
        float ea[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, out[8], bv[8];
        blend8<T>(ea, table, codes + bb * ncoarse, q, az, ay, ax, c0);
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = bias[c0 + j];
        if (lam && index) {
            const float l = *lam;
            const int64_t src = mix_source(index, bb, q.b);
            float eb[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            blend8<T>(eb, table, codes + src * ncoarse, q, az, ay, ax, c0);
            const float l1 = 1.f - l;
#pragma unroll
            for (int j = 0; j < 8; ++j) out[j] = bv[j] + l * ea[j] + l1 * eb[j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) out[j] = bv[j] + ea[j];
        }
        stvec<T, 8>(e + it * 8, out);
    }
}

// ws[B'][cv][c0 .. c0 + 8) = the sum over destinations B (B' weighted lam, index[B] == B' weighted 1 - lam) and
// over the fine voxels of wz wy wx g[B][z][y][x][c0 ..].  A workgroup is 64 items (coarse voxel, 8 channels:
// consecutive items read consecutive 16 bytes of one g row) times GZ waves; wave s takes the fine slabs
// z0 + s, z0 + s + GZ, ... of every item, B in order, then y, x in index order, and wave 0 adds the waves'
// partial sums in wave order: a fixed order, no atomics.  The x loop loads four rows before it uses any
// (rows past the range are the clamped last one, weight 0: never an address outside the grid).
constexpr int GZ = 4;
template <typename T>
__global__ __launch_bounds__(64 * GZ) void k_cond_gather(Geo q, int64_t items, const T *__restrict__ g,
                                                        const float *lam, const int64_t *index,
                                                        float *__restrict__ ws) {
    __shared__ float part[GZ - 1][64][8];
    const int mg = q.m >> 3, li = threadIdx.x & 63, zs = threadIdx.x >> 6;
    const bool mix = lam && index;
    const float l = mix ? *lam : 1.f, l1 = 1.f - l;
    for (int64_t base = int64_t(blockIdx.x) * 64; base < items; base += int64_t(gridDim.x) * 64) {
        const int64_t it = base + li;
        const bool live = it < items;
        float tot[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (live) {
            const int c0 = int(it % mg) * 8;
            uint32_t v = uint32_t(it / mg);  // coarse voxel of [b][cd][ch][cw]
            const int cx = int(v % q.cw);
            v /= q.cw;
            const int cy = int(v % q.ch);
            v /= q.ch;
            const int cz = int(v % q.cd), bsrc = int(v / q.cd);
            int z0, z1, y0, y1, x0, x1;
            axis_range(cz, q.cd, q.d, q.sz, z0, z1);
            axis_range(cy, q.ch, q.h, q.sy, y0, y1);
            axis_range(cx, q.cw, q.w, q.sx, x0, x1);
            for (int bd = 0; bd < q.b; ++bd) {
                const bool own = bd == bsrc, named = mix && mix_source(index, bd, q.b) == int64_t(bsrc);
                if (!own && !named) continue;
                const float mw = (own ? l : 0.f) + (named ? l1 : 0.f);
                float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                for (int z = z0 + zs; z <= z1; z += GZ) {
                    const double wz = axis_weight(axis_coeff(z, q.cd, q.sz), cz);
                    if (wz == 0.0) continue;
                    for (int y = y0; y <= y1; ++y) {
                        const double wzy = wz * axis_weight(axis_coeff(y, q.ch, q.sy), cy);
                        if (wzy == 0.0) continue;
                        const T *row = g + (((int64_t(bd) * q.d + z) * q.h + y) * q.w) * q.m + c0;
                        for (int x = x0; x <= x1; x += 4) {
                            Raw<T, 8> raw[4];
                            float wgt[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int xi = min(x + u, x1);
                                raw[u] = ldraw<T, 8>(row + int64_t(xi) * q.m);
                                wgt[u] = x + u <= x1 ? float(wzy * axis_weight(axis_coeff(xi, q.cw, q.sx), cx)) : 0.f;
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                float r[8];
                                unraw<T, 8>(raw[u], r);
                                if (wgt[u] != 0.f) {
#pragma unroll
                                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(wgt[u], r[j], acc[j]);
                                }
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) tot[j] = fmaf(mw, acc[j], tot[j]);
            }
        }
        if (zs > 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) part[zs - 1][li][j] = tot[j];
        }
        __syncthreads();
        if (zs == 0 && live) {
            for (int s = 0; s < GZ - 1; ++s) {
#pragma unroll
                for (int j = 0; j < 8; ++j) tot[j] += part[s][li][j];
            }
            stvec<float, 8>(ws + it * 8, tot);
        }
        __syncthreads();
    }
}

// workgroup k < kc: dwe[c][k] += the sum, in row order, of the workspace rows whose code is k.  The rows go
// by in chunks of SC_ROWS: thread t compares its 8 consecutive rows of the chunk, an exclusive prefix of the
// threads' counts places the matches in an LDS list in row order, and every thread then adds the listed
// rows of its (up to 4) channels.  Workgroups kc ...: dbe[c] += the sum of every row of 32 channels each (the
// interpolation and mixing weights of a fine voxel sum to 1), eight interleaved row slices added in slice
// order.
constexpr int SC_ROWS = 2048;
__global__ __launch_bounds__(256) void k_cond_scatter(int rows, int m, int kc, const int64_t *__restrict__ codes,
                                                      const float *__restrict__ ws, float *__restrict__ dwe,
                                                      float *__restrict__ dbe) {
    __shared__ int list[SC_ROWS];
    __shared__ int cnt[256];
    __shared__ float part[7][32];
    const int t = threadIdx.x;
    if (int(blockIdx.x) >= kc) {
        const int cl = t & 31, sl = t >> 5, c = (int(blockIdx.x) - kc) * 32 + cl;
        float acc = 0.f;
        if (c < m)
            for (int r = sl; r < rows; r += 8) acc += ws[int64_t(r) * m + c];
        if (sl > 0) part[sl - 1][cl] = acc;
        __syncthreads();
        if (sl == 0 && c < m) {
            for (int j = 0; j < 7; ++j) acc += part[j][cl];
            dbe[c] += acc;
        }
        return;
    }
    const int64_t k = blockIdx.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};  // channels t, t + 256, t + 512, t + 768 (m <= 1024)
    bool any = false;
    for (int r0 = 0; r0 < rows; r0 += SC_ROWS) {
        const int n = min(SC_ROWS, rows - r0);
        unsigned hit = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = t * 8 + j;
            if (r < n && codes[r0 + r] == k) hit |= 1u << j;
        }
        cnt[t] = __popc(hit);
        __syncthreads();
        int off = 0, nm = 0;
        for (int j = 0; j < 256; ++j) {
            const int cj = cnt[j];
            if (j < t) off += cj;
            nm += cj;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (hit >> j & 1u) list[off++] = r0 + t * 8 + j;
        __syncthreads();
        for (int j = 0; j < nm; ++j) {
            const int64_t r = list[j];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = t + 256 * u;
                if (c < m) acc[u] += ws[r * m + c];
            }
        }
        any |= nm > 0;
        __syncthreads();
    }
    if (any) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = t + 256 * u;
            if (c < m) dwe[int64_t(c) * kc + k] += acc[u];
        }
    }
}

bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int check_geo(const char *who, int32_t dtype, int b, int cd, int ch, int cw, int d, int h, int w, int d_out, int m,
              int kc, Geo &q) {
    const std::string n(who);
    if (dtype != VQ3D_F32 && dtype != VQ3D_HALF) return fail(n + ": dtype must be fp32, bf16 or fp16");
    if (m < 8 || m > CE_MMAX || m % 8) return fail(n + ": m must be a multiple of 8, at most 1024");
    if (kc < CE_KMIN || kc > CE_KMAX) return fail(n + ": 8 <= kc <= 1024");
    if (b < 1 || cd < 1 || ch < 1 || cw < 1 || d < 1 || h < 1 || w < 1) return fail(n + ": bad grid or batch size");
    if (std::max({cd, ch, cw, d, h, w}) > CE_AXIS_MAX) return fail(n + ": an axis of a grid is longer than 2^20");
    if (d_out < 1 || d_out > d) return fail(n + ": d_out must be in [1, d]");
    if (int64_t(b) * cd * ch * cw > (int64_t(1) << 24) || int64_t(b) * d * h * w > (int64_t(1) << 31) - 1)
        return fail(n + ": grid too large");
    q = Geo{b, cd, ch, cw, d, h, w, d_out, m, kc, float(cd) / float(d), float(ch) / float(h), float(cw) / float(w)};
    return 0;
}

unsigned grid_items(int64_t items) { return unsigned(std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 65536))); }

}  // namespace
}  // namespace vq3d

using namespace vq3d;

extern "C" {

int vq3d_cond_embed_fwd(int32_t dtype, int32_t b, int32_t cd, int32_t ch, int32_t cw, int32_t d, int32_t h,
                        int32_t w, int32_t d_out, int32_t m, int32_t kc, const int64_t *codes, const void *table,
                        const float *bias, const float *lam, const int64_t *index, void *e, vq3d_stream_t stream) {
    Geo q;
    if (int rc = check_geo("cond_embed_fwd", dtype, b, cd, ch, cw, d, h, w, d_out, m, kc, q)) return rc;
    if (!codes || !table || !bias || !e) return fail("cond_embed_fwd: null pointer");
    if (!al16(table) || !al16(e)) return fail("cond_embed_fwd: table and e must be 16-byte aligned");
    const int64_t items = int64_t(b) * d_out * h * w * (m / 8);
    hipStream_t s = as_stream(stream);
    if (dtype == VQ3D_F32)
        k_cond_fwd<float><<<grid_items(items), 256, 0, s>>>(q, items, codes, (const float *)table, bias, lam, index,
                                                          (float *)e);
    else
        k_cond_fwd<h16_t><<<grid_items(items), 256, 0, s>>>(q, items, codes, (const h16_t *)table, bias, lam, index,
                                                          (h16_t *)e);
    return check_launch("cond_embed_fwd");
}

size_t vq3d_cond_embed_bwd_workspace_bytes(int32_t b, int32_t cd, int32_t ch, int32_t cw, int32_t m) {
    if (b < 1 || cd < 1 || ch < 1 || cw < 1 || m < 1) return 0;
    return size_t(b) * size_t(cd) * size_t(ch) * size_t(cw) * size_t(m) * sizeof(float);
}

int vq3d_cond_embed_bwd(int32_t dtype, int32_t b, int32_t cd, int32_t ch, int32_t cw, int32_t d, int32_t h,
                        int32_t w, int32_t m, int32_t kc, const int64_t *codes, const void *g, const float *lam,
                        const int64_t *index, float *dwe, float *dbe, void *workspace, size_t ws_bytes,
                        vq3d_stream_t stream) {
    Geo q;
    if (int rc = check_geo("cond_embed_bwd", dtype, b, cd, ch, cw, d, h, w, d, m, kc, q)) return rc;
    if (!codes || !g || !workspace) return fail("cond_embed_bwd: null pointer");
    if (!al16(g) || !al16(workspace)) return fail("cond_embed_bwd: g and the workspace must be 16-byte aligned");
    if (ws_bytes < vq3d_cond_embed_bwd_workspace_bytes(b, cd, ch, cw, m)) return fail("cond_embed_bwd: workspace too small");
    if (!dwe && !dbe) return 0;
    const int rows = b * cd * ch * cw;
    const int64_t items = int64_t(rows) * (m / 8);
    hipStream_t s = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    const unsigned ngather = unsigned(std::max<int64_t>(1, std::min<int64_t>((items + 63) / 64, 65536)));
    if (dtype == VQ3D_F32)
        k_cond_gather<float><<<ngather, 64 * GZ, 0, s>>>(q, items, (const float *)g, lam, index, ws);
    else
        k_cond_gather<h16_t><<<ngather, 64 * GZ, 0, s>>>(q, items, (const h16_t *)g, lam, index, ws);
    if (int rc = check_launch("cond_embed_bwd (gather)")) return rc;
    // the per-code workgroups (none without dwe), then the bias sums' (none without dbe)
    const int nk = dwe ? kc : 0, nbias = dbe ? (m + 31) / 32 : 0;
    k_cond_scatter<<<unsigned(nk + nbias), 256, 0, s>>>(rows, m, nk, codes, ws, dwe, dbe);
    return check_launch("cond_embed_bwd");
}

}  // extern "C"
