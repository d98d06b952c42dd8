// tm_adm_kernels.h -- gfx950 kernels of VMAF's ADM feature (libturbometrics_adm.so, include/turbo_metrics_adm.h).
//
// The definition is DESIGN.md section 11; its literal CPU restatement is tests/adm_ref.py.  Per pair and per scale s = 0 .. 3: a db2
// wavelet step of both pictures in f32 (vertical pass first; bands a, v, h, d of half the size), the decoupling of the distorted
// picture's detail bands into a restored part r and an additive part a (a division and an angle test per pixel), the masking
// threshold (a 3 x 3 sum over the three |rf a_b| planes) and, over the centre 80 % of the plane, the sums of cubes N[b] of
// max(|rf r_b| - thr, 0) and Dn[b] of |rf o_b| in double.  The pictures of scale s + 1 are the a bands of scale s.
//
//   k_adm<FMT, S>   grid (tiles of scale S, slots)   block 256   one workgroup per tile of 32 x 16 band pixels of one pair.  It stages
//                   the (2 * 32 + 6) x (2 * 16 + 6) inputs of both pictures that the tile and its one-pixel ring read as f32 in LDS
//                   (4-aligned groups of 4 samples per lane; the mirror is applied while staging, so every pass is a plain stencil),
//                   runs the vertical pass LDS -> LDS (L and Hh of both pictures, 18 rows), then per ring pixel the horizontal
//                   pass (8-byte LDS reads: a lane's four taps are two aligned pairs), the decoupling in registers and |rf a_b|
//                   to LDS (over the staged samples, which are dead by then); after one more barrier the 3 x 3 threshold, the cubes
//                   and the sums.  The twelve band planes, r, a and thr never go through memory: the only planes written are the
//                   two a bands (f32), which the launch of scale S + 1 reads.  S = 0 is instantiated per luma layout.
//                   Sums: per-lane doubles, shuffles over the wave, the four waves through LDS in wave order, and ONE cell of six
//                   doubles per workgroup written by lane 0 -- no floating-point atomics.
//   k_adm_finish    grid (4, slots)   block 256   adds the cells of one scale of one pair in a fixed order (lane i takes cells
//                   i, i + 256, ...; then the same tree as above): two computes of the same input give the same bits.
//
// Every f32 operation below is written one rounding at a time, in the definition's order; the library is built with
// -ffp-contract=off, so that the kernel, its emulation and the restatement take the same branches on the same bits.
#pragma once
#include <math.h>
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::Src / sample1 / load4: the loaders of the XPSNR, motion and VIF kernels

#define TMA_THREADS 256
#define TMA_TX 32                       /* band pixels per tile row */
#define TMA_TY 16                       /* band rows per tile */
#define TMA_RW (TMA_TX + 2)             /* the tile and its ring */
#define TMA_RH (TMA_TY + 2)
#define TMA_NG ((2 * TMA_TX + 8) / 4)   /* staged groups of 4 per row: source columns 2 bx0 - 4 .. 2 bx0 + 2 TX + 3 */
#define TMA_SW (4 * TMA_NG)             /* LDS row, floats (even: pairs are 8-byte aligned); LDS column c = source 2 bx0 - 3 + c */
#define TMA_SH (2 * TMA_TY + 6)         /* staged rows: source rows 2 by0 - 3 .. 2 by0 + 2 TY + 2 */
#define TMA_VC (2 * TMA_RW + 2)         /* columns of the vertical pass */
#define TMA_NI ((TMA_RW * TMA_RH + TMA_THREADS - 1) / TMA_THREADS) /* ring pixels per lane */
#define TMA_SCALES 4

// layouts of include/turbo_metrics_adm.h (the luma planes of the XPSNR layouts)
enum { TMA_Y8 = 0, TMA_Y16_MSB = 1, TMA_Y16_LOW = 2, TMA_Y10_PACKED = 3 };

// one pair of a slot: [0] reference, [1] distorted
struct TmAdmDesc {
    const void *p[2];
    unsigned long long pitch[2]; // bytes
    int vec[2];                  // base and pitch 16-byte aligned: the wide loads are allowed
};

struct TmAdmGeom {
    int w[TMA_SCALES], h[TMA_SCALES];      // the pictures of scale s
    int bw[TMA_SCALES], bh[TMA_SCALES];    // its bands
    int left[TMA_SCALES], top[TMA_SCALES], right[TMA_SCALES], bottom[TMA_SCALES]; // the region the sums run over
    int tiles_x[TMA_SCALES], tiles[TMA_SCALES];
    int cell0[TMA_SCALES];                 // first cell (six doubles) of scale s inside a slot's cells
    int cells;                             // cells per slot
    int bits;                              // D
    int fmt;                               // TMX_F_* of the luma samples
    int shift;                             // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;                         // TMX_F_U16_LOW: sample = v & mask
    float inv;                             // 1 / 2^(D - 8)
    float rf[TMA_SCALES][3];               // the weights of h, v, d
    float cos2;                            // (float)(cos(pi / 180)^2)
    unsigned long long ppitch[TMA_SCALES]; // floats per row of a scale-s picture (s >= 1; a multiple of 4)
    unsigned long long poff[TMA_SCALES];   // first float of scale s's two pictures inside a slot's block
    unsigned long long pslot;              // floats per slot
};

// rf_s[b] = (float)(1 / Q(s, theta)), theta = 1 for h and v, 2 for d; in double
static inline float tma_weight(int lambda, int theta)
{
    static const double A[4][4] = {{0.62171, 0.67234, 0.72709, 0.67234}, {0.34537, 0.41317, 0.49428, 0.41317},
                                   {0.18004, 0.22727, 0.28688, 0.22727}, {0.091401, 0.11792, 0.15214, 0.11792}};
    static const double gt[4] = {1.501, 1.0, 0.534, 1.0};
    const double r = 3.0 * 1080.0 * 3.14159265358979323846 / 180.0;
    const double t = log10(pow(2.0, lambda + 1) * 0.401 * gt[theta] / r);
    const double Q = 2.0 * 0.495 * pow(10.0, 0.466 * t * t) / A[lambda][theta];
    return (float)(1.0 / Q);
}

// sizes of the four scales and the region of the sums; what tm_adm_scores needs of a geometry
static inline void tma_sizes(unsigned w, unsigned h, TmAdmGeom *g)
{
    for (int s = 0; s < TMA_SCALES; ++s) {
        g->w[s] = s ? g->bw[s - 1] : (int)w;
        g->h[s] = s ? g->bh[s - 1] : (int)h;
        g->bw[s] = (g->w[s] + 1) / 2;
        g->bh[s] = (g->h[s] + 1) / 2;
        g->left[s] = (int)(g->bw[s] * 0.1 - 0.5);
        g->top[s] = (int)(g->bh[s] * 0.1 - 0.5);
        g->right[s] = g->bw[s] - g->left[s];
        g->bottom[s] = g->bh[s] - g->top[s];
    }
}

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 32, D outside 8 .. 16 or not one the layout carries
static inline int tma_make_geom(TmAdmGeom *g, unsigned w, unsigned h, int layout, unsigned bits)
{
    memset(g, 0, sizeof *g);
    if (w < 32 || h < 32 || w > (1u << 20) || h > (1u << 20) || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMA_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMA_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMA_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMA_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->bits = (int)bits;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->inv = 1.0f / (float)(1u << (bits - 8));
    const double c = cos(3.14159265358979323846 / 180.0);
    g->cos2 = (float)(c * c);
    tma_sizes(w, h, g);
    for (int s = 0; s < TMA_SCALES; ++s) {
        g->rf[s][0] = g->rf[s][1] = tma_weight(s, 1);
        g->rf[s][2] = tma_weight(s, 2);
        g->tiles_x[s] = (g->bw[s] + TMA_TX - 1) / TMA_TX;
        g->tiles[s] = g->tiles_x[s] * ((g->bh[s] + TMA_TY - 1) / TMA_TY);
        g->cell0[s] = g->cells;
        g->cells += g->tiles[s];
        if (s) {
            g->ppitch[s] = (unsigned long long)(g->w[s] + 3) / 4 * 4;
            g->poff[s] = g->pslot;
            g->pslot += 2 * g->ppitch[s] * (unsigned long long)g->h[s];
        }
    }
    return 0;
}

// ---- sum of six doubles over the workgroup in a fixed order: true on the lane that holds the totals ---------------------------
#ifdef TM_EMULATE
// tests/adm_emul: the lanes of a workgroup are host threads; the harness sums through memory, in lane order
bool tm_adm_block_sum6(double (&a)[6]);
#define TM_ADM_WANT_PLANES 1
#ifndef TM_ADM_PLANE_HOOK
#define TM_ADM_PLANE_HOOK(scale, slot, x, y, r, a, a_ref, a_dis) ((void)0)
#define TM_ADM_THR_HOOK(scale, slot, x, y, thr) ((void)0)
#endif
#else
__device__ __forceinline__ bool tm_adm_block_sum6(double (&a)[6])
{
    __shared__ double red[6][TMA_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] += __shfl_down(a[k], off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) red[k][threadIdx.x >> 6] = a[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = ((red[k][0] + red[k][1]) + red[k][2]) + red[k][3];
    }
    return threadIdx.x == 0;
}
// the test tier reads the r, a, thr and a-band planes here; the product has no such output and computes them only where a sum
// needs them
#define TM_ADM_WANT_PLANES 0
#define TM_ADM_PLANE_HOOK(scale, slot, x, y, r, a, a_ref, a_dis) ((void)0)
#define TM_ADM_THR_HOOK(scale, slot, x, y, thr) ((void)0)
#endif

namespace tma {

// the db2 analysis pair of the definition; every use has a compile-time k: an immediate operand
__host__ __device__ __forceinline__ constexpr float lo(int k)
{
    return k == 0 ? 0.482962913144690f : (k == 1 ? 0.836516303737469f : (k == 2 ? 0.224143868041857f : -0.129409522550921f));
}
__host__ __device__ __forceinline__ constexpr float hi(int k)
{
    return k == 0 ? -0.129409522550921f : (k == 1 ? -0.224143868041857f : (k == 2 ? 0.836516303737469f : -0.482962913144690f));
}

// the definition's border rule: below 0 the edge sample is not repeated, at and beyond n it is (neither motion's nor VIF's mirror)
__host__ __device__ __forceinline__ int mirror(int p, int n) { return p < 0 ? -p : (p >= n ? 2 * n - p - 1 : p); }

// the two tap sums of four samples, each product and each sum rounded on its own
__host__ __device__ __forceinline__ void taps(float x0, float x1, float x2, float x3, float &l, float &h)
{
    float a = lo(0) * x0;
    a = a + lo(1) * x1;
    a = a + lo(2) * x2;
    a = a + lo(3) * x3;
    float b = hi(0) * x0;
    b = b + hi(1) * x1;
    b = b + hi(2) * x2;
    b = b + hi(3) * x3;
    l = a;
    h = b;
}

// The decoupling of one band pixel: o, t = the reference's and the distorted's (h, v, d); r = restored, a = additive.
__host__ __device__ __forceinline__ void decouple(const float (&o)[3], const float (&t)[3], float cos2, float (&r)[3], float (&a)[3])
{
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        float k = t[b] / (o[b] + 1e-30f);
        k = fminf(fmaxf(k, 0.0f), 1.0f);
        r[b] = k * o[b];
    }
    const float p0 = o[0] * t[0], p1 = o[1] * t[1];
    const float dp = p0 + p1;
    const float o0 = o[0] * o[0], o1 = o[1] * o[1];
    const float om = o0 + o1;
    const float t0 = t[0] * t[0], t1 = t[1] * t[1];
    const float tm = t0 + t1;
    const float lhs = dp * dp;
    const float rhs = (cos2 * om) * tm;
    if (dp >= 0.0f && lhs >= rhs) { // within one degree of the reference's direction: an enhancement, gain limited to 100
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float e = r[b] * 100.0f;
            if (r[b] > 0.0f) r[b] = fminf(e, t[b]);
            else if (r[b] < 0.0f) r[b] = fmaxf(e, t[b]);
        }
    }
#pragma unroll
    for (int b = 0; b < 3; ++b) a[b] = t[b] - r[b];
}

__host__ __device__ __forceinline__ double cube(float x)
{
    const double d = (double)x;
    return (d * d) * d;
}

} // namespace tma

template <int FMT, int S>
__global__ void __launch_bounds__(TMA_THREADS) k_adm(TmAdmGeom g, const TmAdmDesc *__restrict__ desc, float *__restrict__ PL,
                                                    double *__restrict__ CELL)
{
    using namespace tma;
    constexpr int SRC = TMA_SH * TMA_SW;  // floats of one staged picture
    constexpr int VER = TMA_RH * TMA_SW;  // floats of one vertical-pass plane
    constexpr int RING = TMA_RH * TMA_RW; // ring pixels
    static_assert(3 * RING <= 2 * SRC, "the |rf a_b| planes lie over the staged samples");
    // [0, 2 SRC): the staged samples of reference and distorted, later the three |rf a_b| planes; then L, Hh of both pictures
    alignas(16) __shared__ float lds[2 * SRC + 4 * VER];
    float *const src = lds, *const ver = lds + 2 * SRC, *const cpl = lds;

    const int tid = threadIdx.x, tile = blockIdx.x, slot = blockIdx.y;
    const int W = g.w[S], H = g.h[S], BW = g.bw[S], BH = g.bh[S];
    const int bx0 = (tile % g.tiles_x[S]) * TMA_TX, by0 = (tile / g.tiles_x[S]) * TMA_TY;
    float *const pl = PL + (size_t)slot * g.pslot;

    // ---- staging: source rows 2 by0 - 3 + r, columns 2 bx0 - 3 + c, mirrored; what no band pixel inside the plane reads is 0
    {
        tmx::Src sp[2];
        const float *fp[2];
        if (S == 0) {
            const TmAdmDesc d = desc[slot];
#pragma unroll
            for (int p = 0; p < 2; ++p) sp[p] = {(const char *)d.p[p], d.pitch[p], FMT, d.vec[p]};
        } else {
#pragma unroll
            for (int p = 0; p < 2; ++p) fp[p] = pl + g.poff[S] + (size_t)p * g.ppitch[S] * H;
        }
        const size_t fpitch = g.ppitch[S];
        for (int it = tid; it < TMA_SH * TMA_NG; it += TMA_THREADS) {
            const int r = it / TMA_NG, gx = it % TMA_NG;
            const int yy = 2 * by0 - 3 + r, xx = 2 * bx0 - 4 + 4 * gx;
            const bool on = yy >= -1 && yy <= 2 * BH && xx + 3 >= -1 && xx <= 2 * BW;
            const int ym = on ? mirror(yy, H) : 0;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                if (on) {
                    if (S == 0) {
                        unsigned q[4] = {0, 0, 0, 0};
                        bool have[4] = {true, true, true, true};
                        if (xx >= 0 && xx + 4 <= W) tmx::load4(sp[p], xx, ym, W, g.shift, g.mask, q);
                        else {
                            const char *row = sp[p].p + (size_t)ym * sp[p].pitch;
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int x = xx + k;
                                have[k] = x >= -1 && x <= 2 * BW;
                                if (have[k]) q[k] = tmx::sample1(row, sp[p].fmt, mirror(x, W), g.shift, g.mask);
                            }
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k) v[k] = have[k] ? (float)q[k] * g.inv - 128.0f : 0.0f;
                    } else {
                        const float *row = fp[p] + (size_t)ym * fpitch;
                        if (xx >= 0 && xx + 4 <= W) {
                            const tm_f4 q = *(const tm_f4 *)(row + xx);
                            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int x = xx + k;
                                if (x >= -1 && x <= 2 * BW) v[k] = row[mirror(x, W)];
                            }
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = 4 * gx + k - 1;
                    if (c >= 0) src[p * SRC + r * TMA_SW + c] = v[k];
                }
            }
        }
    }
    TM_LDS_BARRIER();

    // ---- vertical pass: ring row i from staged rows 2 i .. 2 i + 3; L and Hh of both pictures
    for (int it = tid; it < TMA_RH * TMA_VC; it += TMA_THREADS) {
        const int i = it / TMA_VC, c = it % TMA_VC;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float *s = src + p * SRC + (2 * i) * TMA_SW + c;
            float l, h;
            taps(s[0], s[TMA_SW], s[2 * TMA_SW], s[3 * TMA_SW], l, h);
            ver[(2 * p) * VER + i * TMA_SW + c] = l;
            ver[(2 * p + 1) * VER + i * TMA_SW + c] = h;
        }
    }
    TM_LDS_BARRIER();

    // ---- horizontal pass, decoupling, |rf a_b| of every ring pixel; the a bands and Dn of the tile's own pixels
    const float rf[3] = {g.rf[S][0], g.rf[S][1], g.rf[S][2]};
    float rr[TMA_NI][3];
    unsigned sums = 0, mine = 0; // per ring pixel of this lane: inside the region of the sums; a pixel of the tile inside the plane
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}; // N[h, v, d], Dn[h, v, d]
#pragma unroll
    for (int n = 0; n < TMA_NI; ++n) {
        const int it = tid + n * TMA_THREADS;
        rr[n][0] = rr[n][1] = rr[n][2] = 0.0f;
        if (it >= RING) continue;
        const int ip = it / TMA_RW, jp = it % TMA_RW;
        const int i = by0 - 1 + ip, j = bx0 - 1 + jp;
        float cb[3] = {0.0f, 0.0f, 0.0f}; // a neighbour outside the plane contributes nothing
        if (i >= 0 && i < BH && j >= 0 && j < BW) {
            float band[2][4]; // a, v, h, d
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const float *L = ver + (2 * p) * VER + ip * TMA_SW + 2 * jp, *Hh = L + VER;
                const tm_g2 l01 = *(const tm_g2 *)L, l23 = *(const tm_g2 *)(L + 2);
                const tm_g2 h01 = *(const tm_g2 *)Hh, h23 = *(const tm_g2 *)(Hh + 2);
                taps(l01.x, l01.y, l23.x, l23.y, band[p][0], band[p][1]);
                taps(h01.x, h01.y, h23.x, h23.y, band[p][2], band[p][3]);
            }
            const float o[3] = {band[0][2], band[0][1], band[0][3]}, t[3] = {band[1][2], band[1][1], band[1][3]}; // h, v, d
            float r[3], a[3];
            decouple(o, t, g.cos2, r, a);
#pragma unroll
            for (int b = 0; b < 3; ++b) cb[b] = fabsf(rf[b] * a[b]);
            if (ip >= 1 && ip <= TMA_TY && jp >= 1 && jp <= TMA_TX) {
                mine |= 1u << n;
                if (S < 3) {
                    constexpr int S2 = S < 3 ? S + 1 : 3;
                    float *dst = pl + g.poff[S2] + (size_t)i * g.ppitch[S2] + j;
                    dst[0] = band[0][0];
                    dst[(size_t)g.ppitch[S2] * BH] = band[1][0];
                }
                TM_ADM_PLANE_HOOK(S, slot, j, i, r, a, band[0][0], band[1][0]);
                if (i >= g.top[S] && i < g.bottom[S] && j >= g.left[S] && j < g.right[S]) {
                    sums |= 1u << n;
#pragma unroll
                    for (int b = 0; b < 3; ++b) {
                        rr[n][b] = r[b];
                        acc[3 + b] += cube(fabsf(rf[b] * o[b]));
                    }
                }
            }
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) cpl[b * RING + it] = cb[b];
    }
    TM_LDS_BARRIER();

    // ---- the threshold (b outermost, rows, then columns, one accumulator) and N
    const float wc = (float)(1.0 / 15.0), wn = (float)(1.0 / 30.0);
#pragma unroll
    for (int n = 0; n < TMA_NI; ++n) {
        if (!(((TM_ADM_WANT_PLANES ? mine : sums) >> n) & 1u)) continue;
        const int it = tid + n * TMA_THREADS;
        float thr = 0.0f;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) thr = thr + ((dy | dx) ? wn : wc) * cpl[b * RING + it + dy * TMA_RW + dx];
            }
        }
        TM_ADM_THR_HOOK(S, slot, bx0 - 1 + it % TMA_RW, by0 - 1 + it / TMA_RW, thr);
        if ((sums >> n) & 1u) {
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[b] += cube(fmaxf(fabsf(rf[b] * rr[n][b]) - thr, 0.0f));
        }
    }
    if (tm_adm_block_sum6(acc)) {
        double *cell = CELL + ((size_t)slot * g.cells + g.cell0[S] + tile) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) cell[k] = acc[k];
    }
}

// RES[slot][scale] = {N[h, v, d], Dn[h, v, d]}: the cells of one scale of one pair, added in a fixed order
__global__ void __launch_bounds__(TMA_THREADS) k_adm_finish(TmAdmGeom g, const double *__restrict__ CELL, double *__restrict__ RES)
{
    const int s = blockIdx.x, slot = blockIdx.y;
    const double *cell = CELL + ((size_t)slot * g.cells + g.cell0[s]) * 6;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < g.tiles[s]; i += TMA_THREADS) {
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[k] += cell[6 * i + k];
    }
    if (tm_adm_block_sum6(acc)) {
#pragma unroll
        for (int k = 0; k < 6; ++k) RES[((size_t)slot * TMA_SCALES + s) * 6 + k] = acc[k];
    }
}
