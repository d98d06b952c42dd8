// tm_vif_kernels.h -- gfx950 kernels of VMAF's VIF feature (libturbometrics_vif.so, include/turbo_metrics_vif.h).
//
// The definition is DESIGN.md section 10; its literal CPU restatement is tests/vif_ref.py.  Per pair and per scale s = 0 .. 3: five
// Gaussian-filtered integer moment planes of the two luma pictures (filters of 17, 9, 5, 3 taps, vertical pass first, symmetric
// mirror at the borders), a per-pixel statistic in double from the three variance / covariance integers, and the sums of its two
// terms.  The pictures of scale s + 1 are those of scale s filtered with F_{s+1} and sampled at even positions.
//
//   k_vif<FMT, S>   grid (tiles of scale S, slots)   block 256   one workgroup per tile of 48 x 16 pixels of one pair.  It stages
//                   the tile of both pictures plus the filter's halo in LDS as uint16 (4-aligned groups of 4 samples per lane;
//                   the mirror is applied while staging, so every pass is a plain stencil), runs the vertical pass LDS -> LDS
//                   (16 bytes per pixel: mu_ref | mu_dis, ref^2, dis^2, ref.dis), then the horizontal pass, the statistic and
//                   the sums from LDS in registers: a moment plane never goes through memory.  Between the same two barriers
//                   it also decimates: the staged tile already holds the halo of the NEXT scale's (shorter) filter, so the
//                   workgroup filters the even rows and columns of its tile with F_{S+1} and writes its 24 x 8 samples of the
//                   scale S + 1 pictures (uint16), the only planes that go through memory.  S = 0 is instantiated per luma
//                   layout, S = 1 .. 3 read the uint16 pictures.  One launch per scale: scale S + 1 reads what every tile of
//                   scale S wrote.
//                   Sums: per-lane doubles, shuffles over the wave, the four waves through LDS in wave order, and ONE
//                   (num, den) cell per workgroup written by lane 0 -- no floating-point atomics.
//   k_vif_finish    grid (4, slots)   block 256   adds the cells of one scale of one pair in a fixed order (lane i takes cells
//                   i, i + 256, ...; then the same tree as above): two computes of the same input give the same bits.
#pragma once
#include <math.h>
#include <string.h>
#include <type_traits>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::Src / sample1 / load4: the loaders of the XPSNR and motion kernels

#define TMV_THREADS 256
#define TMV_TW 48                                /* pixels per tile row (LDS row at scale 0: 48 + 2 * 8 = 64 samples) */
#define TMV_TH 16                                /* tile rows */
#define TMV_RPL 4                                /* consecutive rows one lane filters in the vertical pass (sliding window) */
#define TMV_SCALES 4

// layouts of include/turbo_metrics_vif.h (the luma planes of the XPSNR layouts)
enum { TMV_Y8 = 0, TMV_Y16_MSB = 1, TMV_Y16_LOW = 2, TMV_Y10_PACKED = 3 };

// one pair of a slot: [0] reference, [1] distorted
struct TmVifDesc {
    const void *p[2];
    unsigned long long pitch[2]; // bytes
    int vec[2];                  // base and pitch 16-byte aligned: the wide loads are allowed
};

struct TmVifGeom {
    int w[TMV_SCALES], h[TMV_SCALES];
    int tiles_x[TMV_SCALES], tiles[TMV_SCALES];
    int cell0[TMV_SCALES];                 // first (num, den) cell of scale s inside a slot's cells
    int cells;                             // cells per slot
    int bits;                              // D
    int fmt;                               // TMX_F_* of the luma samples
    int shift;                             // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;                         // TMX_F_U16_LOW: sample = v & mask
    unsigned long long ppitch[TMV_SCALES]; // samples per row of a scale-s picture (s >= 1; a multiple of 8)
    unsigned long long poff[TMV_SCALES];   // first sample of scale s's two pictures inside a slot's block
    unsigned long long pslot;              // samples per slot
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 32 (so that w3, h3 >= 4 and no mirror leaves a
// plane), D outside 8 .. 16 or not one the layout carries
static inline int tmv_make_geom(TmVifGeom *g, unsigned w, unsigned h, int layout, unsigned bits)
{
    memset(g, 0, sizeof *g);
    if (w < 32 || h < 32 || w > (1u << 20) || h > (1u << 20) || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMV_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMV_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMV_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMV_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->bits = (int)bits;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    for (int s = 0; s < TMV_SCALES; ++s) {
        g->w[s] = s ? g->w[s - 1] / 2 : (int)w;
        g->h[s] = s ? g->h[s - 1] / 2 : (int)h;
        g->tiles_x[s] = (g->w[s] + TMV_TW - 1) / TMV_TW;
        g->tiles[s] = g->tiles_x[s] * ((g->h[s] + TMV_TH - 1) / TMV_TH);
        g->cell0[s] = g->cells;
        g->cells += g->tiles[s];
        if (s) {
            g->ppitch[s] = (unsigned long long)(g->w[s] + 7) / 8 * 8;
            g->poff[s] = g->pslot;
            g->pslot += 2 * g->ppitch[s] * (unsigned long long)g->h[s];
        }
    }
    return 0;
}

// ---- sum of (a, b) over the workgroup in a fixed order: true on the lane that holds the totals -------------------------------
#ifdef TM_EMULATE
// tests/vif_emul: the lanes of a workgroup are host threads; the harness sums through memory, in lane order
bool tm_vif_block_sum2(double &a, double &b);
#ifndef TM_VIF_PLANE_HOOK
#define TM_VIF_PLANE_HOOK(scale, slot, x, y, s1, s2, s12) ((void)0)
#endif
#else
__device__ __forceinline__ bool tm_vif_block_sum2(double &a, double &b)
{
    __shared__ double red[2][TMV_THREADS / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
    return threadIdx.x == 0;
}
// the test tier reads the three integer planes here; the product has no such output
#define TM_VIF_PLANE_HOOK(scale, slot, x, y, s1, s2, s12) ((void)0)
#endif

namespace tmv {

__host__ __device__ constexpr int ntaps(int s) { return s == 0 ? 17 : (s == 1 ? 9 : (s == 2 ? 5 : 3)); }

// the four filters of the definition, Q16, each summing to 65536; every use has a compile-time (s, k): an immediate operand
__host__ __device__ __forceinline__ constexpr unsigned coef(int s, int k)
{
    constexpr unsigned F0[17] = {489, 935, 1640, 2640, 3896, 5274, 6547, 7455, 7784, 7455, 6547, 5274, 3896, 2640, 1640, 935, 489};
    constexpr unsigned F1[9] = {1244, 3663, 7925, 12590, 14692, 12590, 7925, 3663, 1244};
    constexpr unsigned F2[5] = {3571, 16004, 26386, 16004, 3571};
    constexpr unsigned F3[3] = {10904, 43728, 10904};
    return s == 0 ? F0[k] : (s == 1 ? F1[k] : (s == 2 ? F2[k] : F3[k]));
}

// the definition's border rule: symmetric, the edge sample is not repeated on either side (NOT motion's mirror)
__host__ __device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// vertical pass of one pixel: mu_ref | mu_dis << 16, then ref^2, dis^2, ref.dis on the 32-bit scale of the definition
struct alignas(16) Ver { unsigned mu, xx, yy, xy; };

// The statistic of one pixel from the three integers (Q16 on an 8-bit sample scale), operations in the definition's order.  Every
// branch is decided on integers.
__host__ __device__ __forceinline__ void stat(int s1, int s2, int s12, double &num, double &den)
{
    const int a = s1 > 0 ? s1 : 0, b = s2 > 0 ? s2 : 0, c = s12;
    const double A = (double)a / 65536.0, B = (double)b / 65536.0, C = (double)c / 65536.0;
    if (a < 131072) { // the reference's variance is below the noise variance 2
        num = 1.0 - B * (4.0 / 65025.0);
        den = 1.0;
        return;
    }
    den = log2(1.0 + A / 2.0);
    if (c <= 0 || b == 0) {
        num = 0.0;
        return;
    }
    double g = C / (A + 1e-10);
    double sv = B - g * C;
    sv = sv > 1e-10 ? sv : 1e-10;
    g = g < 100.0 ? g : 100.0;
    num = log2(1.0 + g * g * A / (sv + 2.0));
}

} // namespace tmv

template <int FMT, int S>
__global__ void __launch_bounds__(TMV_THREADS) k_vif(TmVifGeom g, const TmVifDesc *__restrict__ desc, unsigned short *__restrict__ PL,
                                                    double *__restrict__ CELL)
{
    using namespace tmv;
    constexpr int N = ntaps(S), HL = N / 2;     // taps and halo of this scale's filter
    constexpr int HP = (HL + 3) / 4 * 4;        // halo in whole groups of 4: staged columns x0 - HP .. x0 + TW + HP - 1
    constexpr int LW = TMV_TW + 2 * HP;         // LDS row, samples
    constexpr int NG = LW / 4;                  // groups per staged row
    constexpr int SH = TMV_TH + 2 * HL;         // staged rows y0 - HL .. y0 + TH + HL - 1
    constexpr bool WIDE = S > 0 || FMT != TMX_F_U8; // sum F x x beyond 32 bits (8-bit samples: 65536 * 255^2 < 2^32)
    constexpr int S2 = S < 3 ? S + 1 : 3;       // the scale this launch decimates to (S = 3: none)
    constexpr int N2 = ntaps(S2), HL2 = N2 / 2;
    constexpr int DW = TMV_TW + 2 * HL2;        // columns of the decimation's vertical pass
    typedef typename std::conditional<WIDE, unsigned long long, unsigned>::type Acc;

    alignas(8) __shared__ unsigned short src[2][SH * LW]; // the staged samples of reference and distorted
    __shared__ Ver ver[TMV_TH * LW];                      // the vertical pass of the moments
    __shared__ unsigned short dec[2][(TMV_TH / 2) * LW];  // the vertical pass of the decimation: even tile rows

    const int tid = threadIdx.x, tile = blockIdx.x, slot = blockIdx.y;
    const int W = g.w[S], H = g.h[S];
    const int x0 = (tile % g.tiles_x[S]) * TMV_TW, y0 = (tile / g.tiles_x[S]) * TMV_TH;
    const int in = S == 0 ? g.bits : 16; // bits of this scale's samples
    const int sh = S == 0 ? g.shift : 0;
    const unsigned mk = S == 0 ? g.mask : 0xFFFFu;
    unsigned short *const pl = PL + (size_t)slot * g.pslot;

    // ---- staging: rows and columns outside the plane mirrored; what no pass of a pixel inside the plane reads is 0
    tmx::Src sp[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (S == 0) {
            const TmVifDesc d = desc[slot];
            sp[p] = {(const char *)d.p[p], d.pitch[p], FMT, d.vec[p]};
        } else {
            sp[p] = {(const char *)(pl + g.poff[S] + (size_t)p * g.ppitch[S] * H), g.ppitch[S] * 2, TMX_F_HIST, 1};
        }
    }
    for (int it = tid; it < SH * NG; it += TMV_THREADS) {
        const int r = it / NG, gx = it % NG;
        const int yy = y0 - HL + r, xx = x0 - HP + 4 * gx;
        const bool on = yy <= H - 1 + HL && xx + 3 >= -HL && xx <= W - 1 + HL;
        const int ym = on ? mirror(yy, H) : 0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            unsigned v[4] = {0, 0, 0, 0};
            if (on) {
                if (xx >= 0 && xx + 4 <= W) tmx::load4(sp[p], xx, ym, W, sh, mk, v);
                else {
                    const char *row = sp[p].p + (size_t)ym * sp[p].pitch;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int x = xx + k;
                        if (x >= -HL && x <= W - 1 + HL) v[k] = tmx::sample1(row, sp[p].fmt, mirror(x, W), sh, mk);
                    }
                }
            }
            *(tm_u2 *)&src[p][r * LW + 4 * gx] = tm_u2{v[0] | v[1] << 16, v[2] | v[3] << 16};
        }
    }
    TM_LDS_BARRIER();

    // ---- vertical pass of the moments: column c, tile rows r0 .. r0 + RPL - 1 from staged rows r0 .. r0 + RPL + N - 2
    {
        const unsigned rnd1 = 1u << (in - 1);
        const int q = S == 0 ? 2 * (g.bits - 8) : 16;
        const Acc rnd2 = q ? (Acc)1 << (q - 1) : (Acc)0;
        for (int it = tid; it < LW * (TMV_TH / TMV_RPL); it += TMV_THREADS) {
            const int c = it % LW, r0 = (it / LW) * TMV_RPL;
            unsigned xs[TMV_RPL + N - 1], ys[TMV_RPL + N - 1];
#pragma unroll
            for (int j = 0; j < TMV_RPL + N - 1; ++j) {
                xs[j] = src[0][(r0 + j) * LW + c];
                ys[j] = src[1][(r0 + j) * LW + c];
            }
#pragma unroll
            for (int o = 0; o < TMV_RPL; ++o) {
                unsigned a1 = 0, a2 = 0;
                Acc axx = 0, ayy = 0, axy = 0;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const unsigned f = coef(S, k), x = xs[o + k], y = ys[o + k];
                    a1 += f * x; // below 2^32: 65536 * 65535 + 32768
                    a2 += f * y;
                    axx += (Acc)f * (x * x);
                    ayy += (Acc)f * (y * y);
                    axy += (Acc)f * (x * y);
                }
                Ver o4;
                o4.mu = ((a1 + rnd1) >> in) | ((a2 + rnd1) >> in) << 16;
                o4.xx = (unsigned)((axx + rnd2) >> q);
                o4.yy = (unsigned)((ayy + rnd2) >> q);
                o4.xy = (unsigned)((axy + rnd2) >> q);
                ver[(r0 + o) * LW + c] = o4;
            }
        }
        // ---- vertical pass of the decimation: the even tile rows, filtered with the NEXT scale's filter, rounded to 16 bits
        if (S < 3) {
            for (int it = tid; it < (TMV_TH / 2) * DW; it += TMV_THREADS) {
                const int r = it / DW, c = HP - HL2 + it % DW;
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    unsigned a = 0;
#pragma unroll
                    for (int k = 0; k < N2; ++k) a += coef(S2, k) * src[p][(HL + 2 * r - HL2 + k) * LW + c];
                    dec[p][r * LW + c] = (unsigned short)((a + rnd1) >> in);
                }
            }
        }
    }
    TM_LDS_BARRIER();

    // ---- horizontal pass, the three integers and the statistic
    double num = 0.0, den = 0.0;
    for (int it = tid; it < TMV_TW * TMV_TH; it += TMV_THREADS) {
        const int r = it / TMV_TW, c = it % TMV_TW;
        if (y0 + r >= H || x0 + c >= W) continue;
        unsigned m1 = 0, m2 = 0;
        unsigned long long xx = 0, yy = 0, xy = 0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const Ver v = ver[r * LW + c + HP - HL + k];
            const unsigned f = coef(S, k);
            m1 += f * (v.mu & 0xFFFFu);
            m2 += f * (v.mu >> 16);
            xx += (unsigned long long)f * v.xx;
            yy += (unsigned long long)f * v.yy;
            xy += (unsigned long long)f * v.xy;
        }
        const unsigned exx = (unsigned)((xx + 32768u) >> 16), eyy = (unsigned)((yy + 32768u) >> 16), exy = (unsigned)((xy + 32768u) >> 16);
        const int s1 = (int)(exx - (unsigned)(((unsigned long long)m1 * m1 + 0x80000000ull) >> 32));
        const int s2 = (int)(eyy - (unsigned)(((unsigned long long)m2 * m2 + 0x80000000ull) >> 32));
        const int s12 = (int)(exy - (unsigned)(((unsigned long long)m1 * m2 + 0x80000000ull) >> 32));
        TM_VIF_PLANE_HOOK(S, slot, x0 + c, y0 + r, s1, s2, s12);
        double n1, d1;
        stat(s1, s2, s12, n1, d1);
        num += n1;
        den += d1;
    }
    // ---- horizontal pass of the decimation: the even columns; sample (x0 / 2 + c, y0 / 2 + r) of the next scale's pictures
    if (S < 3) {
        const int W2 = g.w[S2], H2 = g.h[S2];
        for (int it = tid; it < (TMV_TW / 2) * (TMV_TH / 2); it += TMV_THREADS) {
            const int r = it / (TMV_TW / 2), c = it % (TMV_TW / 2);
            const int xo = x0 / 2 + c, yo = y0 / 2 + r;
            if (yo >= H2 || xo >= W2) continue;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                unsigned a = 0;
#pragma unroll
                for (int k = 0; k < N2; ++k) a += coef(S2, k) * dec[p][r * LW + HP + 2 * c - HL2 + k];
                pl[g.poff[S2] + ((size_t)p * H2 + yo) * g.ppitch[S2] + xo] = (unsigned short)((a + 32768u) >> 16);
            }
        }
    }
    if (tm_vif_block_sum2(num, den)) {
        double *cell = CELL + ((size_t)slot * g.cells + g.cell0[S] + tile) * 2;
        cell[0] = num;
        cell[1] = den;
    }
}

// RES[slot][scale] = {num, den}: the cells of one scale of one pair, added in a fixed order
__global__ void __launch_bounds__(TMV_THREADS) k_vif_finish(TmVifGeom g, const double *__restrict__ CELL, double *__restrict__ RES)
{
    const int s = blockIdx.x, slot = blockIdx.y;
    const double *cell = CELL + ((size_t)slot * g.cells + g.cell0[s]) * 2;
    double num = 0.0, den = 0.0;
    for (int i = threadIdx.x; i < g.tiles[s]; i += TMV_THREADS) {
        num += cell[2 * i];
        den += cell[2 * i + 1];
    }
    if (tm_vif_block_sum2(num, den)) {
        RES[((size_t)slot * TMV_SCALES + s) * 2] = num;
        RES[((size_t)slot * TMV_SCALES + s) * 2 + 1] = den;
    }
}
