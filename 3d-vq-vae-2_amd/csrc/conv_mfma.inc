// bf16 implicit-GEMM 3-D convolution on the CDNA4 matrix cores (v_mfma_f32_16x16x32_bf16).
//
// One workgroup (4 waves) owns a brick of output voxels (BH x BW x BD).  Per channel chunk
// of CP (multiple of 8) channels it stages:
//   halo  : the brick's input footprint, prologue applied once per element, circular wrap or
//           zero padding resolved here, stored [position][CP] bf16 (16-B rows = one A fragment)
//   weights: [k-chunk of 8][N][8] bf16 (one B fragment = one ds_read_b128)
// and runs M = voxels (16 per tile), N = output channels (16 per tile), K = taps x CP.
// The epilogue is shared with the VALU kernels (scale / bias / conv bias / residual /
// fused ELU-affine activation for forward; derivative / addend / scalar partials for
// backward-data).
//
// Backward-data of a stride-1 conv IS a stride-1 conv of g with the transposed, flipped
// kernel and padding k-1-p (circular or zero): same kernel, DGRAD = true.
// (included by conv3d.hip after the shared epilogue helpers)
namespace vq3d {

struct MArgs {
    int B, Ca, Cb, N;        // input channels (Ca from x, Cb from x2), output channels of this GEMM
    int iH, iW, iD;          // input grid of this GEMM
    int oH, oW, oD;          // output grid of this GEMM
    int k, s, p, circ;
    int pro_kind;
    const float *pro_a, *pro_b;
    int wCt;                 // channel extent of the weight's 2nd dim (W[co][wCt][k^3])
    int bh, bw, bd;          // brick (output voxels)
    int hh, hw, hd;          // halo extents
    int nbh, nbw, nbd;       // bricks per dim
    int lbd, lbw;            // log2 of the (power-of-two) brick extents bd, bw
    FastDiv fhd, fhw;        // division by the halo extents hd, hw
    FastDiv fN;              // division by N (epilogue element -> voxel)
    int region0;             // bytes of the halo / output-tile region (weights follow)
};

__device__ __forceinline__ int mwrap(int i, int n) {
    while (i < 0) i += n;
    while (i >= n) i -= n;
    return i;
}

__device__ __forceinline__ half_t to_half(float f) { return static_cast<half_t>(f); }

template <int NT>
struct MTiles {
    // M tiles (16 voxels each) per wave, bounded by the accumulator budget (MTW * NT <= 16)
    static constexpr int value = NT <= 2 ? 8 : (NT <= 4 ? 4 : 2);
};

// 8 consecutive channels [ch0, ch0 + 8) of one voxel as bf16, prologue applied; zero beyond Ctot.
// 16 / 8 / 4-byte vector loads for 8k / 4 / 2-channel single-input tensors; raw bits pass
// through untouched when there is no prologue.
template <bool PRO>
__device__ __forceinline__ hx8 load8(const h16_t *__restrict__ x, const h16_t *__restrict__ x2, int Ca, int Cb,
                                        int64_t vox, int ch0, const Prologue &pro) {
    const int Ctot = Ca + Cb;
    const bool raw = !PRO || pro.kind == VQ3D_PRO_NONE;
    uint4 q = {0u, 0u, 0u, 0u};
    bool vec = true;
    if (Cb == 0 && (Ca & 7) == 0 && ch0 + 8 <= Ca) {
        q = *reinterpret_cast<const uint4 *>(x + vox * Ca + ch0);
    } else if (Cb == 0 && Ca == 4 && ch0 == 0) {
        const uint2 t = *reinterpret_cast<const uint2 *>(x + vox * 4);
        q.x = t.x;
        q.y = t.y;
    } else if (Cb == 0 && Ca == 2 && ch0 == 0) {
        q.x = *reinterpret_cast<const uint32_t *>(x + vox * 2);
    } else {
        vec = false;
    }
    if (vec && raw) return __builtin_bit_cast(hx8, q);
    float v[8];
    if (vec) {
        const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = h2f_lo(u[j]);
            v[2 * j + 1] = h2f_hi(u[j]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ch = ch0 + j;
            v[j] = ch < Ca ? ld(x + vox * Ca + ch) : (ch < Ctot ? ld(x2 + vox * Cb + (ch - Ca)) : 0.f);
        }
    }
    hx8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float f = (!raw && ch0 + j < Ctot) ? pro.apply(v[j]) : v[j];
        r[j] = to_half(f);
    }
    return r;
}

// Stage a brick's input footprint for channels [c0, c0 + CP): one item = one position x 8
// channels = one 16-B LDS slot; prologue applied once; circular wrap / zero pad resolved.
// Circular wrap is one conditional step (the planner guarantees pad and overhang <= extent);
// positions still outside the grid only feed voxels beyond the output grid and stage as zero.
template <int CP, bool PRO>
__device__ __forceinline__ void stage_halo(const MArgs &a, const h16_t *__restrict__ x,
                                           const h16_t *__restrict__ x2, int b, int ih0, int iw0, int id0,
                                           int c0, const Prologue &pro, hx8 *halo) {
    constexpr int G = CP / 8;
    const int npos = a.hh * a.hw * a.hd;
    const int64_t vb = int64_t(b) * a.iH * a.iW * a.iD;
    const int total = npos * G;
    // 4 items per thread in flight: all loads issue before the LDS stores wait on them
    for (int e0 = threadIdx.x; e0 < total; e0 += 4 * 256) {
        hx8 val[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = e0 + j * 256;
            val[j] = hx8{};
            if (e < total) {
                const int gi = e % G, pos = e / G;
                const int t = int(a.fhd.div(uint32_t(pos))), pd = pos - t * a.hd;
                const int ph = int(a.fhw.div(uint32_t(t))), pw = t - ph * a.hw;
                int ih = ih0 + ph, iw = iw0 + pw, id = id0 + pd;
                if (a.circ) {
                    ih += ih < 0 ? a.iH : (ih >= a.iH ? -a.iH : 0);
                    iw += iw < 0 ? a.iW : (iw >= a.iW ? -a.iW : 0);
                    id += id < 0 ? a.iD : (id >= a.iD ? -a.iD : 0);
                }
                const bool ok =
                    unsigned(ih) < unsigned(a.iH) && unsigned(iw) < unsigned(a.iW) && unsigned(id) < unsigned(a.iD);
                if (ok) val[j] = load8<PRO>(x, x2, a.Ca, a.Cb, vb + (ih * a.iW + iw) * a.iD + id, c0 + 8 * gi, pro);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j * 256 < total) halo[e0 + j * 256] = val[j];
    }
}

template <int CP, int NT, bool DGRAD>
__global__ __launch_bounds__(256) void k_conv_mfma(MArgs a, const h16_t *__restrict__ x, const h16_t *__restrict__ x2,
                                                  const float *__restrict__ w, FwdEpi<h16_t> fe, BwdEpi<h16_t> be,
                                                  int cin_split, const float *__restrict__ gscale,
                                                  h16_t *__restrict__ y, h16_t *__restrict__ y2, float *dpre,
                                                  float *dpost, int nbricks, GridSum gsum) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NTOT = NT * 16;
    constexpr int MTW = MTiles<NT>::value;
    constexpr int G = CP / 8;                    // 8-channel groups per position
    const int K3 = a.k * a.k * a.k;
    const int nkc = (K3 * CP + 7) / 8;           // 8-wide k chunks
    const int nks = (nkc + 3) / 4;               // 32-wide k steps
    hx8 *halo = reinterpret_cast<hx8 *>(smem);     // [npos][G]; after the MFMAs: fp32 tile [nvb][N]
    float *otile = reinterpret_cast<float *>(smem);
    hx8 *wl = reinterpret_cast<hx8 *>(smem + a.region0);  // [nks*4][NTOT]
    int *ktab = reinterpret_cast<int *>(wl + nks * 4 * NTOT);  // [nks*4]: halo slot offset of k chunk, -1 = pad
    __shared__ float red[8];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Ctot = a.Ca + a.Cb;
    const int nvb = a.bh * a.bw * a.bd;
    const int nmt = (nvb + 15) / 16;
    const bool one_chunk = Ctot <= CP;
    const Prologue pro = make_prologue(a.pro_kind, a.pro_a, a.pro_b);

    // k chunk kc = 8 consecutive (tap, c) with c fastest: tap = kc*8 / CP, group gi
    for (int kc = tid; kc < nks * 4; kc += 256) {
        const int kk = kc * 8, tap = kk / CP, gi = (kk - tap * CP) / 8;
        int off = -1;
        if (tap < K3) {
            const int kd = tap % a.k, kw = (tap / a.k) % a.k, kh = tap / (a.k * a.k);
            off = ((kh * a.hw + kw) * a.hd + kd) * G + gi;
        }
        ktab[kc] = off;
    }
    // weights of channel chunk c0: one item = 8 consecutive k of one output channel n
    auto stage_w = [&](int c0) {
        for (int e = tid; e < nks * 4 * NTOT; e += 256) {
            const int n = e % NTOT, kc = e / NTOT;
            hx8 r;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int kk = kc * 8 + j;
                const int tap = kk / CP, c = kk - tap * CP, ch = c0 + c;
                float val = 0.f;
                if (tap < K3 && ch < Ctot && n < a.N) {
                    if (!DGRAD) {
                        val = w[(int64_t(n) * a.wCt + ch) * K3 + tap];
                    } else {
                        // g channel ch = conv output channel, n = conv input channel, flipped tap
                        val = w[(int64_t(ch) * a.wCt + n) * K3 + (K3 - 1 - tap)];
                    }
                }
                r[j] = to_half(val);
            }
            wl[e] = r;
        }
    };
    if (one_chunk) stage_w(0);

    // this lane's A-row voxel per M-tile (wave w owns tiles w, w + 4, ...), relative to the halo
    const int row = lane & 15, kq = lane >> 4;
    int posbase[MTW];
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
        int v = (wave + 4 * m) * 16 + row;
        if (v >= nvb) v = 0;
        const int ld_ = v & (a.bd - 1), lw_ = (v >> a.lbd) & (a.bw - 1), lh_ = v >> (a.lbd + a.lbw);
        posbase[m] = (((lh_ * a.s) * a.hw + lw_ * a.s) * a.hd + ld_ * a.s) * G;
    }
    float pre = 0.f, post = 0.f;
    const float gs = gscale ? *gscale : 1.f;
    const float sc = fe.scale ? *fe.scale : 1.f, bias = fe.bias ? *fe.bias : 0.f;
    const float aa = fe.act_a ? *fe.act_a : 0.f, ab = fe.act_b ? *fe.act_b : 0.f;
    ActDeriv dv;
    dv.mode = (DGRAD && be.aux) ? be.mode : 0;
    dv.p = (dv.mode && be.p) ? *be.p : 0.f;

    const TileSched bsc = xcd_sched(nbricks);
    for (int brick = bsc.t; brick < bsc.end; brick += bsc.step) {
        int bi = brick;
        const int bzd = bi % a.nbd; bi /= a.nbd;
        const int bzw = bi % a.nbw; bi /= a.nbw;
        const int bzh = bi % a.nbh;
        const int b = bi / a.nbh;
        const int oh0 = bzh * a.bh, ow0 = bzw * a.bw, od0 = bzd * a.bd;
        const int ih0 = oh0 * a.s - a.p, iw0 = ow0 * a.s - a.p, id0 = od0 * a.s - a.p;
        f32x4 acc[MTW][NT];
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int c0 = 0; c0 < Ctot; c0 += CP) {
            __syncthreads();
            stage_halo<CP, !DGRAD>(a, x, x2, b, ih0, iw0, id0, c0, pro, halo);
            if (!one_chunk) stage_w(c0);
            __syncthreads();
            // ---- MFMA over the k steps of this chunk
            for (int ks = 0; ks < nks; ++ks) {
                const int kc = ks * 4 + kq;
                const int off = ktab[kc];
                hx8 bfr[NT];
#pragma unroll
                for (int n = 0; n < NT; ++n) bfr[n] = wl[kc * NTOT + n * 16 + row];
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    if (wave + 4 * m >= nmt) break;
                    hx8 afr = hx8{};
                    if (off >= 0) afr = halo[posbase[m] + off];
#pragma unroll
                    for (int n = 0; n < NT; ++n)
                        acc[m][n] = VQ3D_MFMA_16X16X32(afr, bfr[n], acc[m][n], 0, 0, 0);
                }
            }
        }

        // ---- epilogue: accumulators -> LDS tile [nvb][N] (lane: voxel rows kq*4 + i, column
        // `row` of each N tile), then element-wise over the tile in output-memory order so
        // consecutive lanes read / write consecutive channels of consecutive voxels
        __syncthreads();
#pragma unroll
        for (int m = 0; m < MTW; ++m) {
            if (wave + 4 * m >= nmt) break;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int v = (wave + 4 * m) * 16 + kq * 4 + i;
#pragma unroll
                for (int n = 0; n < NT; ++n) {
                    const int co = n * 16 + row;
                    if (v < nvb && co < a.N) otile[v * a.N + co] = acc[m][n][i];
                }
            }
        }
        __syncthreads();
        const int64_t ob = int64_t(b) * a.oH * a.oW * a.oD;  // batch base voxel
        for (int e = tid; e < nvb * a.N; e += 256) {
            const int v = int(a.fN.div(uint32_t(e))), co = e - v * a.N;
            const int ld_ = v & (a.bd - 1), lw_ = (v >> a.lbd) & (a.bw - 1), lh_ = v >> (a.lbd + a.lbw);
            const int oh = oh0 + lh_, ow = ow0 + lw_, od = od0 + ld_;
            if (oh >= a.oH || ow >= a.oW || od >= a.oD) continue;
            const int64_t vox = ob + (oh * a.oW + ow) * a.oD + od;
            float val = otile[e];
            if (!DGRAD) {
                if (fe.scale) val = val * sc;
                if (fe.bias) val = val + bias;
                if (fe.cbias) val = val + fe.cbias[co];
                if (fe.res) {
                    if (!fe.res_up2) {
                        val = val + ld(fe.res + vox * a.N + co);
                    } else {
                        const int rH = a.oH / 2, rW = a.oW / 2, rD = a.oD / 2;
                        int h0, h1, w0, w1, d0, d1;
                        float lh, lw, ldd;
                        up_coeff(oh, rH, h0, h1, lh);
                        up_coeff(ow, rW, w0, w1, lw);
                        up_coeff(od, rD, d0, d1, ldd);
                        auto R = [&](int hh, int ww, int dd) {
                            return ld(fe.res + (((int64_t(b) * rH + hh) * rW + ww) * rD + dd) * a.N + co);
                        };
                        val = val + ((1.f - lh) * ((1.f - lw) * ((1.f - ldd) * R(h0, w0, d0) + ldd * R(h0, w0, d1)) +
                                                  lw * ((1.f - ldd) * R(h0, w1, d0) + ldd * R(h0, w1, d1))) +
                                     lh * ((1.f - lw) * ((1.f - ldd) * R(h1, w0, d0) + ldd * R(h1, w0, d1)) +
                                           lw * ((1.f - ldd) * R(h1, w1, d0) + ldd * R(h1, w1, d1))));
                    }
                }
                st(y + vox * a.N + co, epi_act(fe.act, val, aa, ab));
            } else {
                // output channel co = conv input channel (y: first cin_split, y2: the rest)
                if (gscale) val = val * gs;
                if (co < cin_split) {
                    const int64_t o = vox * cin_split + co;
                    pre += val;
                    if (dv.mode) val = val * dv(ld(be.aux + o));
                    post += val;
                    if (be.addend) val = val + ld(be.addend + o);
                    st(y + o, val);
                } else {
                    st(y2 + vox * (a.N - cin_split) + (co - cin_split), val);
                }
            }
        }
    }
    if (DGRAD && (dpre || dpost)) {
        pre = block_sum<float, 256>(pre, red);
        post = block_sum<float, 256>(post, red + 4);
        grid_sum2<256>(gsum, pre, post, dpre, dpost, red);
    }
}

// ---------------------------------------------------------------------------------------- host
static int round8(int c) { return (c + 7) / 8 * 8; }

struct MPlan {
    MArgs a;
    int cp, nt;
    size_t lds;
    unsigned blocks;
    bool ok;
};

static MPlan plan_mfma(int B, int Ca, int Cb, int N, int iH, int iW, int iD, int oH, int oW, int oD, int k, int s,
                       int p, int circ, bool wgrad = false) {
    MPlan m = {};
    MArgs &a = m.a;
    a.B = B; a.Ca = Ca; a.Cb = Cb; a.N = N;
    a.iH = iH; a.iW = iW; a.iD = iD; a.oH = oH; a.oW = oW; a.oD = oD;
    a.k = k; a.s = s; a.p = p; a.circ = circ;
    // one-step circular wrap in the staging needs pad and overhang within every extent
    if (circ && (p > std::min(iH, std::min(iW, iD)) || k - 1 - p > std::min(iH, std::min(iW, iD)))) return m;
    const int Ctot = Ca + Cb;
    m.cp = Ctot >= 32 ? 32 : (Ctot > 16 ? round8(Ctot) : (Ctot > 8 ? 16 : 8));
    if (m.cp == 24 && Ctot > 24) m.cp = 32;
    const int ntr = (N + 15) / 16;
    m.nt = ntr <= 5 ? ntr : (ntr <= 8 ? 8 : 0);
    if (wgrad) m.nt = 1;  // brick sizing only
    if (m.nt == 0) return m;
    const int mtw = m.nt <= 2 ? 8 : (m.nt <= 4 ? 4 : 2);
    const int target = 64 * mtw;  // voxels per brick = 4 waves x mtw tiles x 16
    auto pow2_floor = [](int v) { int r = 1; while (r * 2 <= v) r *= 2; return r; };
    auto pow2_ceil = [](int v) { int r = 1; while (r < v) r *= 2; return r; };
    a.bd = std::min(pow2_ceil(oD), 16);
    a.bw = std::min(pow2_ceil(oW), pow2_floor(std::max(1, target / (a.bd * 4))));
    a.bh = std::min(pow2_ceil(oH), pow2_floor(std::max(1, target / (a.bd * a.bw))));
    while (a.bh * a.bw * a.bd > target) {
        if (a.bh > 1) a.bh /= 2;
        else if (a.bw > 1) a.bw /= 2;
        else a.bd /= 2;
    }
    const int K3 = k * k * k;
    auto lds_of = [&]() {
        const int hh = (a.bh - 1) * s + k, hw = (a.bw - 1) * s + k, hd = (a.bd - 1) * s + k;
        const size_t halo = size_t(hh) * hw * hd * m.cp * 2;
        if (wgrad) {  // + g tile [voxels padded to 32][co padded to 16] bf16
            const size_t nvp = (size_t(a.bh) * a.bw * a.bd + 31) / 32 * 32;
            return std::max(halo + nvp * ((N + 15) / 16) * 16 * 2, size_t(256) * 16 * 4);
        }
        const int nks = ((K3 * m.cp + 7) / 8 + 3) / 4;
        const size_t wts = size_t(nks) * 4 * m.nt * 16 * 16;
        const size_t r0 = (std::max(halo, size_t(a.bh) * a.bw * a.bd * N * 4) + 15) & ~size_t(15);
        return r0 + wts + size_t(nks) * 4 * 4;
    };
    while (lds_of() > 64 * 1024) {
        if (a.bh > 1) a.bh /= 2;
        else if (a.bw > 1) a.bw /= 2;
        else if (a.bd > 1) a.bd /= 2;
        else return m;
    }
    a.lbd = 0;
    while ((1 << a.lbd) < a.bd) ++a.lbd;
    a.lbw = 0;
    while ((1 << a.lbw) < a.bw) ++a.lbw;
    a.hh = (a.bh - 1) * s + k;
    a.hw = (a.bw - 1) * s + k;
    a.hd = (a.bd - 1) * s + k;
    a.fhd = FastDiv(uint32_t(a.hd));
    a.fhw = FastDiv(uint32_t(a.hw));
    a.fN = FastDiv(uint32_t(N));
    {
        const size_t halo = size_t(a.hh) * a.hw * a.hd * m.cp * 2;
        a.region0 = int((std::max(halo, size_t(a.bh) * a.bw * a.bd * N * 4) + 15) & ~size_t(15));
    }
    a.nbh = (oH + a.bh - 1) / a.bh;
    a.nbw = (oW + a.bw - 1) / a.bw;
    a.nbd = (oD + a.bd - 1) / a.bd;
    m.lds = lds_of();
    m.blocks = unsigned(int64_t(B) * a.nbh * a.nbw * a.nbd);
    m.ok = true;
    return m;
}

template <bool DGRAD>
static int launch_mfma(const MPlan &m, const h16_t *x, const h16_t *x2, const float *w, const FwdEpi<h16_t> &fe,
                       const BwdEpi<h16_t> &be, int cin_split, const float *gscale, h16_t *y, h16_t *y2,
                       float *dpre, float *dpost, hipStream_t s) {
    const int nbricks = int(m.blocks);
#define KL(CP, NT)                                                                                           \
    {                                                                                                        \
        auto kern = k_conv_mfma<CP, NT, DGRAD>;                                                              \
        /* persistent grid: the chip filled at the kernel's occupancy, bricks strided (weights */            \
        /* staged once per workgroup for single-chunk convs) */                                              \
        const unsigned nb = resident_blocks(kern, 256, m.lds, m.blocks);                                     \
        kern<<<nb, 256, m.lds, s>>>(m.a, x, x2, w, fe, be, cin_split, gscale, y, y2, dpre, dpost, nbricks,   \
                                    grid_sum_for(s, nb, DGRAD && (dpre || dpost)));                          \
    }
#define NTS(CP)                                                                                              \
    switch (m.nt) {                                                                                          \
    case 1: KL(CP, 1) break;                                                                                 \
    case 2: KL(CP, 2) break;                                                                                 \
    case 3: KL(CP, 3) break;                                                                                 \
    case 4: KL(CP, 4) break;                                                                                 \
    case 5: KL(CP, 5) break;                                                                                 \
    default: KL(CP, 8) break;                                                                                \
    }
    switch (m.cp) {
    case 8: NTS(8) break;
    case 16: NTS(16) break;
    case 24: NTS(24) break;
    default: NTS(32) break;
    }
#undef NTS
#undef KL
    return check_launch(DGRAD ? "conv3d_bwd_data(mfma)" : "conv3d_fwd(mfma)");
}


// ---------------------------------------------------------------------------------------- weight gradient
// G[co][c][tap] = sum_v g[v][co] * halo[pos(v) + off(tap)][c] over the staged brick (same halo as
// the forward).  Thread tile = (tap, 8 input channels, 8 output channels): 64 fp32 accumulators,
// one ds_read_b128 of x and one of g per voxel; voxel sub-streams fill the workgroup; bricks are
// grid-strided; tiles are ordered tap-fastest so each wave's atomics walk consecutive addresses
// of the reference [co][ci][tap] layout.  blockIdx.y: tile group, blockIdx.z: channel chunk.
template <int CP>
__global__ __launch_bounds__(256) void k_wgrad_tiled(MArgs a, const h16_t *__restrict__ x,
                                                    const h16_t *__restrict__ x2, const h16_t *__restrict__ g,
                                                    int ncog, int tpb, int S, int nbricks,
                                                    const float *__restrict__ w, const float *__restrict__ escale,
                                                    float *dw, float *dscale, float *dbias, float *dcbias,
                                                    float *part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int G = CP / 8;
    __shared__ float red8[8];
    const int K3 = a.k * a.k * a.k;
    const int npos = a.hh * a.hw * a.hd;
    const int nvb = a.bh * a.bw * a.bd;
    const int Ctot = a.Ca + a.Cb;
    const int c0 = blockIdx.z * CP;
    hx8 *halo = reinterpret_cast<hx8 *>(smem);  // [npos][G]
    hx8 *gs = halo + npos * G;                       // [nvb][ncog]
    float *scr = reinterpret_cast<float *>(smem);       // reduction scratch (after the brick loop)
    const int tid = threadIdx.x;
    const int tl = tid % tpb, sub = tid / tpb;
    const int T = K3 * G * ncog;
    const int tt = blockIdx.y * tpb + tl;
    const bool active = sub < S && tt < T;
    // tt = ((cog * G + gi) * K3 + tap): tap fastest
    const int tap = tt % K3, r = tt / K3, gi = r % G, cog = r / G;
    const int kd = tap % a.k, kw = (tap / a.k) % a.k, kh = tap / (a.k * a.k);
    const int toff = (kh * a.hw + kw) * a.hd + kd;
    const Prologue pro = make_prologue(a.pro_kind, a.pro_a, a.pro_b);
    Prologue none;
    none.kind = VQ3D_PRO_NONE;
    none.a = none.b = 0.f;
    const bool do_bias = blockIdx.y == 0 && blockIdx.z == 0 && (dbias || dcbias);

    float acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    float gsum = 0.f;  // thread co = tid < N: sum of g over this block's voxels

    const TileSched bsc = xcd_sched(nbricks);
    for (int brick = bsc.t; brick < bsc.end; brick += bsc.step) {
        int bi = brick;
        const int bzd = bi % a.nbd; bi /= a.nbd;
        const int bzw = bi % a.nbw; bi /= a.nbw;
        const int bzh = bi % a.nbh;
        const int b = bi / a.nbh;
        const int oh0 = bzh * a.bh, ow0 = bzw * a.bw, od0 = bzd * a.bd;
        __syncthreads();
        stage_halo<CP, true>(a, x, x2, b, oh0 * a.s - a.p, ow0 * a.s - a.p, od0 * a.s - a.p, c0, pro, halo);
        // g tile: voxels outside the output grid are zero rows
        for (int e = tid; e < nvb * ncog; e += 256) {
            const int cg = e % ncog, v = e / ncog;
            const int ld_ = v & (a.bd - 1), lw_ = (v >> a.lbd) & (a.bw - 1), lh_ = v >> (a.lbd + a.lbw);
            const int oh = oh0 + lh_, ow = ow0 + lw_, od = od0 + ld_;
            hx8 val = hx8{};
            if (oh < a.oH && ow < a.oW && od < a.oD) {
                const int64_t vox = ((int64_t(b) * a.oH + oh) * a.oW + ow) * a.oD + od;
                val = load8<false>(g, nullptr, a.N, 0, vox, cg * 8, none);
            }
            gs[e] = val;
        }
        __syncthreads();
        if (do_bias && tid < a.N) {
            const int cg = tid / 8, j = tid % 8;
            for (int v = 0; v < nvb; ++v) gsum += float(gs[v * ncog + cg][j]);
        }
        if (active) {
            for (int v = sub; v < nvb; v += S) {
                const int ld_ = v & (a.bd - 1), lw_ = (v >> a.lbd) & (a.bw - 1), lh_ = v >> (a.lbd + a.lbw);
                const int pb = ((lh_ * a.s) * a.hw + lw_ * a.s) * a.hd + ld_ * a.s;
                const hx8 xv = halo[(pb + toff) * G + gi];
                const hx8 gv = gs[v * ncog + cog];
                float xf[8], gf[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    xf[i] = float(xv[i]);
                    gf[i] = float(gv[i]);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(xf[i], gf[j], acc[i][j]);
            }
        }
    }
    // reduce the S voxel sub-streams (16 accumulators per round through LDS); then either this
    // workgroup's image of its tiles into the workspace (part: k_wgrad_gen_reduce sums the images
    // in a fixed order) or atomics
    const float sc = escale ? *escale : 1.f;
    float wg = 0.f;
    float *img = part ? part + (size_t(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (tpb * 64) +
                            tl * 64
                      : nullptr;
    for (int rnd = 0; rnd < 4; ++rnd) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) scr[q * 256 + tid] = acc[(rnd * 16 + q) / 8][(rnd * 16 + q) % 8];
        __syncthreads();
        if (active && sub == 0) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                float sum = 0.f;
                for (int j = 0; j < S; ++j) sum += scr[q * 256 + j * tpb + tl];
                const int idx = rnd * 16 + q, ci = c0 + gi * 8 + idx / 8, co = cog * 8 + idx % 8;
                if (img) {
                    img[idx] = sum;
                } else if (ci < Ctot && co < a.N) {
                    const int64_t e = (int64_t(co) * a.wCt + ci) * K3 + tap;
                    if (dw) atomicAdd(dw + e, escale ? sum * sc : sum);
                    if (dscale) wg = fmaf(w[e], sum, wg);
                }
            }
        }
    }
    if (part) {
        if (do_bias && tid < a.N)
            part[size_t(gridDim.z) * gridDim.y * gridDim.x * (tpb * 64) + size_t(blockIdx.x) * a.N + tid] = gsum;
        return;
    }
    if (dscale) {
        wg = block_sum<float, 256>(wg, red8);
        if (tid == 0) atomicAdd(dscale, wg);
    }
    if (do_bias) {
        if (dcbias && tid < a.N) atomicAdd(dcbias + tid, gsum);
        if (dbias) {
            const float t = block_sum<float, 256>(tid < a.N ? gsum : 0.f, red8 + 4);
            if (tid == 0) atomicAdd(dbias, t);
        }
    }
}

// Geometry of the two generic weight-gradient kernels (k_wgrad_tiled: outputs > 64, k_wgrad_mfma)
// and the size of their per-workgroup images: group g = (channel chunk z, tile group y) holds E
// entries per workgroup x; the conv-bias sums follow as nbx rows of N.
struct GenW {
    bool mfma;
    int nbx, ytiles, nchunks, E;
    int ncog, tpb, S, T;  // tiled
    int ntm, npw, KK;     // mfma
};
static GenW gen_wgrad_geom(const MPlan &m) {
    const MArgs &a = m.a;
    GenW g = {};
    const int K3 = a.k * a.k * a.k;
    const int nbricks = int(m.blocks);
    g.nchunks = (a.Ca + a.Cb + m.cp - 1) / m.cp;
    g.mfma = a.N <= 64;
    if (!g.mfma) {
        const int G = m.cp / 8;
        g.ncog = (a.N + 7) / 8;
        g.T = K3 * G * g.ncog;
        g.tpb = std::min(g.T, 256);
        // few bricks (the top levels' 128-channel convs on 128..1,024 voxels): narrower tile groups
        // per workgroup, each split over 256 / tpb voxel sub-streams, so the grid still covers the chip
        while (g.tpb == 256 && nbricks * ((g.T + 127) / 128) * g.nchunks <= 256 && g.T >= 128) g.tpb = 128;
        while (g.tpb == 128 && nbricks * ((g.T + 63) / 64) * g.nchunks <= 256 && g.T >= 64) g.tpb = 64;
        g.S = std::max(1, 256 / g.tpb);
        g.ytiles = (g.T + g.tpb - 1) / g.tpb;
        g.nbx = std::max(1, std::min(nbricks, 512 / std::max(1, g.ytiles * g.nchunks)));
        g.E = g.tpb * 64;
        return g;
    }
    g.ntm = (a.N + 15) / 16;  // 1..4 (planner guarantees N <= 64)
    const int ntiles = (K3 * m.cp + 15) / 16;
    // N tiles per wave: accumulators NTM x NPW x 4 stay <= 112 VGPRs
    const int cap = g.ntm == 1 ? 14 : (g.ntm == 2 ? 14 : 7);
    const int need = (ntiles + 3) / 4;
    const int npw = need <= 2 ? 2 : (need <= 4 ? 4 : (need <= 7 ? 7 : 14));
    g.npw = std::min(npw, cap);
    g.ytiles = (ntiles + 4 * g.npw - 1) / (4 * g.npw);
    int nbx = std::max(1, std::min(nbricks, 1024 / (g.nchunks * g.ytiles)));
    // 9..16-channel 3x3x3 (the 18-channel blocks' branch conv, 1,024 bricks at 128^2 x 32): two
    // bricks per workgroup measured 72.5 -> 65.0 us (workgroup-cap sweep, round 1);
    // the 4- / 8-channel (and larger) grids are fastest uncapped
    if (m.cp == 16 && a.k == 3 && a.s == 1 && nbricks <= 1024) nbx = std::min(nbx, 512);
    g.nbx = nbx;
    g.KK = K3 * m.cp;
    g.E = a.N * 64 * g.npw;
    return g;
}
static size_t gen_wgrad_bytes(const GenW &g, int N) {
    return (size_t(g.nchunks) * g.ytiles * g.nbx * g.E + size_t(g.nbx) * N) * 4;
}

// dW (+ escale), dscale, conv-bias and scalar-bias sums from the generic kernels' images: LANES
// lanes per entry, each summing a strided slice of the nbx images (8 loads in flight), combined by
// a fixed shuffle tree: deterministic.
struct GRArgs {
    int mfma, ngrp, nbx, E, N, K3, wCt, Ctot, CP, ytiles;
    int tpb, G, T;  // tiled
    int KK, KB;     // mfma
};
template <int LANES>
__global__ __launch_bounds__(256) void k_wgrad_gen_reduce(GRArgs r, const float *__restrict__ part,
                                                          const float *__restrict__ w,
                                                          const float *__restrict__ escale, float *dw, float *dscale,
                                                          float *dbias, float *dcbias, GridSum gsum) {
    __shared__ float red[8];
    const int64_t nw = int64_t(r.ngrp) * r.E;
    const int lane = threadIdx.x % LANES;
    const int64_t f = int64_t(blockIdx.x) * (256 / LANES) + threadIdx.x / LANES;
    const bool bias = dbias || dcbias;
    const bool in = f < nw + (bias ? r.N : 0);
    float sum = 0.f;
    if (in) {
        const float *p;
        int64_t stride;
        if (f < nw) {
            const int64_t gi = f / r.E, j = f - gi * r.E;
            p = part + gi * r.nbx * r.E + j;
            stride = r.E;
        } else {
            p = part + nw * r.nbx + (f - nw);
            stride = r.N;
        }
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int x0 = lane; x0 < r.nbx; x0 += 8 * LANES) {
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (x0 + u * LANES < r.nbx) acc[u] += p[(x0 + u * LANES) * stride];
        }
        sum = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    sum = group_sum<LANES>(sum);
    float wg = 0.f, bs = 0.f;
    if (in && lane == 0) {
        if (f < nw) {
            const int gi = int(f / r.E), j = int(f - int64_t(gi) * r.E);
            const int y = gi % r.ytiles, z = gi / r.ytiles, c0 = z * r.CP;
            int co = -1, ci = 0, tap = 0;
            if (!r.mfma) {
                const int tl = j / 64, idx = j - tl * 64, tt = y * r.tpb + tl;
                if (tt < r.T) {
                    tap = tt % r.K3;
                    const int rr = tt / r.K3, gg = rr % r.G, cog = rr / r.G;
                    ci = c0 + gg * 8 + idx / 8;
                    co = cog * 8 + idx % 8;
                }
            } else {
                const int c_o = j / r.KB, kk = y * r.KB + (j - c_o * r.KB);
                if (kk < r.KK) {
                    tap = kk / r.CP;
                    ci = c0 + kk - tap * r.CP;
                    co = c_o;
                }
            }
            if (co >= 0 && co < r.N && ci < r.Ctot) {
                const int64_t e = (int64_t(co) * r.wCt + ci) * r.K3 + tap;
                if (dw) dw[e] += escale ? sum * *escale : sum;
                if (dscale) wg = w[e] * sum;
            }
        } else {
            if (dcbias) dcbias[f - nw] += sum;
            bs = sum;
        }
    }
    if (dscale || dbias) {
        wg = block_sum<float, 256>(wg, red);
        bs = block_sum<float, 256>(bs, red + 4);
        grid_sum2<256>(gsum, wg, bs, dscale, dbias, red);
    }
}

static int launch_wgrad_gen_reduce(const MPlan &m, const GenW &gw, const float *part, const float *w,
                                   const float *escale, float *dw, float *dscale, float *dbias, float *dcbias,
                                   hipStream_t s) {
    const MArgs &a = m.a;
    GRArgs r = {};
    r.mfma = gw.mfma;
    r.ngrp = gw.nchunks * gw.ytiles;
    r.nbx = gw.nbx;
    r.E = gw.E;
    r.N = a.N;
    r.K3 = a.k * a.k * a.k;
    r.wCt = a.wCt;
    r.Ctot = a.Ca + a.Cb;
    r.CP = m.cp;
    r.ytiles = gw.ytiles;
    r.tpb = gw.tpb;
    r.G = m.cp / 8;
    r.T = gw.T;
    r.KK = gw.KK;
    r.KB = 64 * gw.npw;
    const int64_t n = int64_t(r.ngrp) * r.E + ((dbias || dcbias) ? r.N : 0);
    // lanes per entry: at most ~16 images per lane
    int lanes = 1;
    while (lanes < 64 && lanes * 16 < r.nbx) lanes *= 2;
#define GR(L)                                                                                                  \
    {                                                                                                          \
        const unsigned nb = unsigned((n + 256 / L - 1) / (256 / L));                                           \
        k_wgrad_gen_reduce<L><<<nb, 256, 0, s>>>(r, part, w, escale, dw, dscale, dbias, dcbias,                \
                                                 grid_sum_for(s, nb, dscale || dbias));                       \
    }
    switch (lanes) {
    case 1: GR(1) break;
    case 2: GR(2) break;
    case 4: GR(4) break;
    case 8: GR(8) break;
    case 16: GR(16) break;
    case 32: GR(32) break;
    default: GR(64) break;
    }
#undef GR
    return check_launch("conv3d_bwd_weight(generic reduce)");
}

// part: the call's workspace, gen_wgrad_bytes long (conv3d.hip's launch_wgrad refuses a shorter one,
// so the kernels' part == nullptr atomic branch is never taken from here)
static int launch_wgrad_tiled(MPlan m, const h16_t *x, const h16_t *x2, const h16_t *g, const float *w,
                              const float *escale, float *dw, float *dscale, float *dbias, float *dcbias,
                              float *part, hipStream_t s) {
    const GenW gw = gen_wgrad_geom(m);
    const int ncog = gw.ncog, tpb = gw.tpb, S = gw.S, nbx = gw.nbx;
    const int nbricks = int(m.blocks);
    dim3 grid((unsigned)nbx, (unsigned)gw.ytiles, (unsigned)gw.nchunks);
#define WG(CP) k_wgrad_tiled<CP><<<grid, 256, m.lds, s>>>(m.a, x, x2, g, ncog, tpb, S, nbricks, w, escale, dw, dscale, dbias, dcbias, part)
    switch (m.cp) {
    case 8: WG(8); break;
    case 16: WG(16); break;
    case 24: WG(24); break;
    default: WG(32); break;
    }
#undef WG
    if (int r = check_launch("conv3d_bwd_weight(tiled)")) return r;
    return launch_wgrad_gen_reduce(m, gw, part, w, escale, dw, dscale, dbias, dcbias, s);
}


// ---------------------------------------------------------------------------------------- weight gradient (MFMA)
// dW[co][(tap, c)] += sum_v g[v][co] * X[v][(tap, c)],  X[v][(tap, c)] = halo[pos(v) + off(tap)][c]
// as D[M = co][N = (tap, c)] += A[co][v] B[v][(tap, c)] with K = voxels, 32 per MFMA.  Both
// operands come from row-major LDS tiles through the gfx950 transposing read
// ds_read_b64_tr_b16 (each lane gathers 4 rows x 4 columns, lanes receive columns): A from the
// g tile [v][16 co], B straight from the staged halo [pos][CP] (any row address per lane, so
// the tap shift costs nothing).  The whole wave runs every tr read (EXEC all ones): rows
// beyond the brick read zero g rows.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ s16x4 tr_read(const h16_t *lds_elem) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(lds_elem));
}

// one 8-element MFMA operand from two transposed reads (whole-vector shuffle + bit cast; an
// element-wise build is mis-scheduled into duplicated halves)
__device__ __forceinline__ hx8 cat_bf16(s16x4 lo, s16x4 hi) {
    return __builtin_bit_cast(hx8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int CP, int NTM, int NPW>
__global__ __launch_bounds__(256) void k_wgrad_mfma(MArgs a, const h16_t *__restrict__ x,
                                                   const h16_t *__restrict__ x2, const h16_t *__restrict__ g,
                                                   int nbricks, const float *__restrict__ w,
                                                   const float *__restrict__ escale, float *dw, float *dscale,
                                                   float *dbias, float *dcbias, int lds_image, float *part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int G = CP / 8;
    constexpr int MT = NTM * 16;  // co rows of the g tile (padded)
    __shared__ float red8[8];
    const int K3 = a.k * a.k * a.k;
    const int npos = a.hh * a.hw * a.hd;
    const int nvb = a.bh * a.bw * a.bd;
    const int nvp = (nvb + 31) / 32 * 32;
    const int Ctot = a.Ca + a.Cb;
    const int c0 = blockIdx.z * CP;
    hx8 *halo = reinterpret_cast<hx8 *>(smem);                  // [npos][G]
    h16_t *gs = reinterpret_cast<h16_t *>(halo + npos * G);          // [nvp][MT]
    float *img = reinterpret_cast<float *>(smem);                      // dW image after the loop
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int grp = lane >> 4, li = lane & 15, q = li >> 2, p = li & 3;
    const int KK = K3 * CP;                 // (tap, c) columns of this channel chunk
    const int nt0 = blockIdx.y * 4 * NPW;   // this block's first tile
    const Prologue pro = make_prologue(a.pro_kind, a.pro_a, a.pro_b);
    Prologue none;
    none.kind = VQ3D_PRO_NONE;
    none.a = none.b = 0.f;
    const bool do_bias = blockIdx.y == 0 && blockIdx.z == 0 && (dbias || dcbias);

    // this lane's column chunk (4 consecutive (tap, c)) for each of the wave's N tiles
    int coff[NPW];
#pragma unroll
    for (int t = 0; t < NPW; ++t) {
        const int nt = nt0 + wave + 4 * t;
        int kk0 = nt * 16 + 4 * p;
        if (kk0 >= KK) kk0 = 0;  // padded columns read a valid address, are never written
        const int tap = kk0 / CP, c = kk0 - tap * CP;
        const int kd = tap % a.k, kw = (tap / a.k) % a.k, kh = tap / (a.k * a.k);
        coff[t] = ((kh * a.hw + kw) * a.hd + kd) * CP + c;  // element offset from the voxel's base position
    }
    f32x4 acc[NTM][NPW];
#pragma unroll
    for (int m = 0; m < NTM; ++m)
#pragma unroll
        for (int t = 0; t < NPW; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float gsum = 0.f;

    const TileSched bsc = xcd_sched(nbricks);
    for (int brick = bsc.t; brick < bsc.end; brick += bsc.step) {
        int bi = brick;
        const int bzd = bi % a.nbd; bi /= a.nbd;
        const int bzw = bi % a.nbw; bi /= a.nbw;
        const int bzh = bi % a.nbh;
        const int b = bi / a.nbh;
        const int oh0 = bzh * a.bh, ow0 = bzw * a.bw, od0 = bzd * a.bd;
        __syncthreads();
        stage_halo<CP, true>(a, x, x2, b, oh0 * a.s - a.p, ow0 * a.s - a.p, od0 * a.s - a.p, c0, pro, halo);
        // g tile [nvp][MT] bf16, zero outside the grid / beyond the brick / beyond N
        for (int e = tid; e < nvp * (MT / 8); e += 256) {
            const int cg = e % (MT / 8), v = e / (MT / 8);
            hx8 val = hx8{};
            if (v < nvb) {
                const int ld_ = v & (a.bd - 1), lw_ = (v >> a.lbd) & (a.bw - 1), lh_ = v >> (a.lbd + a.lbw);
                const int oh = oh0 + lh_, ow = ow0 + lw_, od = od0 + ld_;
                if (oh < a.oH && ow < a.oW && od < a.oD && cg * 8 < a.N) {
                    const int64_t vox = ((int64_t(b) * a.oH + oh) * a.oW + ow) * a.oD + od;
                    val = load8<false>(g, nullptr, a.N, 0, vox, cg * 8, none);
                }
            }
            reinterpret_cast<hx8 *>(gs)[e] = val;
        }
        __syncthreads();
        if (do_bias && tid < a.N) {
            for (int v = 0; v < nvb; ++v) gsum += ld(gs + v * MT + tid);
        }
        for (int ks = 0; ks < nvp / 32; ++ks) {
            const int v1 = ks * 32 + 8 * grp + q, v2 = v1 + 4;
            // A = g^T: rows v1 / v2 of the g tile, columns 4p..4p+3 of each 16-co tile
            hx8 af[NTM];
#pragma unroll
            for (int m = 0; m < NTM; ++m)
                af[m] = cat_bf16(tr_read(gs + v1 * MT + m * 16 + 4 * p), tr_read(gs + v2 * MT + m * 16 + 4 * p));
            // B rows: the voxels' base halo positions (clamped into the brick for padded rows)
            const int u1 = v1 < nvb ? v1 : 0, u2 = v2 < nvb ? v2 : 0;
            const int pb1 = (((u1 >> (a.lbd + a.lbw)) * a.s) * a.hw + ((u1 >> a.lbd) & (a.bw - 1)) * a.s) * a.hd +
                            (u1 & (a.bd - 1)) * a.s;
            const int pb2 = (((u2 >> (a.lbd + a.lbw)) * a.s) * a.hw + ((u2 >> a.lbd) & (a.bw - 1)) * a.s) * a.hd +
                            (u2 & (a.bd - 1)) * a.s;
            const h16_t *hb = reinterpret_cast<const h16_t *>(halo);
#pragma unroll
            for (int t = 0; t < NPW; ++t) {
                const hx8 bfr = cat_bf16(tr_read(hb + pb1 * CP + coff[t]), tr_read(hb + pb2 * CP + coff[t]));
#pragma unroll
                for (int m = 0; m < NTM; ++m)
                    acc[m][t] = VQ3D_MFMA_16X16X32(af[m], bfr, acc[m][t], 0, 0, 0);
            }
        }
    }
    // D layout: lane column li -> kk = nt*16 + li, rows grp*4 + i -> co.  With room, stage the
    // block's columns in an LDS image [co][kk - kb] and issue the atomics in the reference
    // [co][ci][tap] order (tap fastest, consecutive addresses); else atomics from registers.
    const float sc = escale ? *escale : 1.f;
    float wg = 0.f;
    constexpr int KB = 64 * NPW;
    const int kb = nt0 * 16, ke = min(KK, kb + KB);
    if (part) {  // this workgroup's [co][KB] image into the workspace (k_wgrad_gen_reduce sums them)
        float *img = part + (size_t(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (a.N * KB);
#pragma unroll
        for (int t = 0; t < NPW; ++t) {
            const int kl = (wave + 4 * t) * 16 + li;
#pragma unroll
            for (int m = 0; m < NTM; ++m)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int co = m * 16 + grp * 4 + i;
                    if (co < a.N) img[co * KB + kl] = acc[m][t][i];
                }
        }
        if (do_bias && tid < a.N)
            part[size_t(gridDim.z) * gridDim.y * gridDim.x * (a.N * KB) + size_t(blockIdx.x) * a.N + tid] = gsum;
        return;
    }
    if (lds_image) {
        __syncthreads();
        for (int e = tid; e < a.N * KB; e += 256) img[e] = 0.f;
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < NPW; ++t) {
        const int kk = (nt0 + wave + 4 * t) * 16 + li;
        const int tap = kk / CP, c = kk - tap * CP;
        const bool colok = kk < KK && c0 + c < Ctot;
#pragma unroll
        for (int m = 0; m < NTM; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int co = m * 16 + grp * 4 + i;
                if (co >= a.N || !colok) continue;
                if (lds_image) {
                    img[co * KB + kk - kb] = acc[m][t][i];
                } else {
                    const int64_t e = (int64_t(co) * a.wCt + c0 + c) * K3 + tap;
                    const float v = acc[m][t][i];
                    if (dw) atomicAdd(dw + e, escale ? v * sc : v);
                    if (dscale) wg = fmaf(w[e], v, wg);
                }
            }
    }
    if (lds_image) {
        __syncthreads();
        const int cc = min(CP, Ctot - c0);
        for (int e = tid; e < a.N * cc * K3; e += 256) {
            const int tap = e % K3, r = e / K3, c = r % cc, co = r / cc;
            const int kk = tap * CP + c;
            if (kk < kb || kk >= ke) continue;
            const float v = img[co * KB + kk - kb];
            const int64_t ge = (int64_t(co) * a.wCt + c0 + c) * K3 + tap;
            if (dw) atomicAdd(dw + ge, escale ? v * sc : v);
            if (dscale) wg = fmaf(w[ge], v, wg);
        }
    }
    if (dscale) {
        wg = block_sum<float, 256>(wg, red8);
        if (tid == 0) atomicAdd(dscale, wg);
    }
    if (do_bias) {
        if (dcbias && tid < a.N) atomicAdd(dcbias + tid, gsum);
        if (dbias) {
            const float tt = block_sum<float, 256>(tid < a.N ? gsum : 0.f, red8 + 4);
            if (tid == 0) atomicAdd(dbias, tt);
        }
    }
}

static int launch_wgrad_mfma(MPlan m, const h16_t *x, const h16_t *x2, const h16_t *g, const float *w,
                             const float *escale, float *dw, float *dscale, float *dbias, float *dcbias,
                             float *part, hipStream_t s) {
    const MArgs &a = m.a;
    const GenW gw = gen_wgrad_geom(m);
    const int ntm = gw.ntm, NPW = gw.npw;
    const int nbricks = int(m.blocks);
    const int lds_image = size_t(a.N) * 64 * NPW * 4 <= m.lds ? 1 : 0;
    dim3 grid((unsigned)gw.nbx, (unsigned)gw.ytiles, (unsigned)gw.nchunks);
#define WGM(CP, NTM, NPW_)                                                                                      \
    k_wgrad_mfma<CP, NTM, NPW_><<<grid, 256, m.lds, s>>>(m.a, x, x2, g, nbricks, w, escale, dw, dscale, dbias, \
                                                         dcbias, lds_image, part)
#define NPWS(CP, NTM)                                                                                         \
    if (NPW == 2) WGM(CP, NTM, 2);                                                                            \
    else if (NPW == 4) WGM(CP, NTM, 4);                                                                       \
    else if (NPW == 7) WGM(CP, NTM, 7);                                                                       \
    else WGM(CP, NTM, 14);
#define NPWS7(CP, NTM)                                                                                        \
    if (NPW == 2) WGM(CP, NTM, 2);                                                                            \
    else if (NPW == 4) WGM(CP, NTM, 4);                                                                       \
    else WGM(CP, NTM, 7);
#define NTMS(CP)                                                                                              \
    if (ntm == 1) { NPWS(CP, 1) } else if (ntm == 2) { NPWS(CP, 2) } else if (ntm == 3) { NPWS7(CP, 3) }    \
    else { NPWS7(CP, 4) }
    switch (m.cp) {
    case 8: NTMS(8) break;
    case 16: NTMS(16) break;
    case 24: NTMS(24) break;
    default: NTMS(32) break;
    }
#undef NTMS
#undef NPWS
#undef NPWS7
#undef WGM
    if (int r = check_launch("conv3d_bwd_weight(mfma)")) return r;
    return launch_wgrad_gen_reduce(m, gw, part, w, escale, dw, dscale, dbias, dcbias, s);
}

}  // namespace vq3d
