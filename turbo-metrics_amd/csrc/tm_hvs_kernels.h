// tm_hvs_kernels.h -- gfx950 kernels of PSNR-HVS and PSNR-HVS-M (libturbometrics_hvs.so, include/turbo_metrics_hvs.h).
//
// The definition is DESIGN.md section 16; its float64 restatement is tests/hvs_ref.py.  Per pair of luma planes: over the
// non-overlapping 8x8 blocks, the orthonormal DCT of A and of the integer difference A - B, the contrast masking of both pictures and
// the two sums S2 (PSNR-HVS) and S1 (PSNR-HVS-M) of the CSF-weighted squared coefficients.
//
//   k_hvs<FMT>     grid (tiles, slots)   block 256   one workgroup per tile of TMH_TW x TMH_TH samples = 16 x 2 blocks of one slot's pair.
//                  A wave owns eight neighbouring blocks of one block row; lane (r, bx) = lane r * 8 + bx of the wave owns row r of block
//                  bx: eight consecutive lanes load 64 consecutive samples of one picture row, the two waves of a block row 128.  Every
//                  sample of a block leaves memory once; the right and bottom remainder is never addressed.
//                    1. the lane's row: integer half-row sums of z and z^2 of A and B (exact), the 8-point DCT of the row of A and of the
//                       row of A - B (the difference taken on the integers), both in registers;
//                    2. transpose through LDS (rows of 9 floats: no bank conflicts either way); lane c of the block then owns column c:
//                       the second 8-point DCT gives T(A)[k][c] and T(A - B)[k][c], k = 0 .. 7, and T(B) = T(A) - T(A - B);
//                    3. the lane's share of the two AC energies goes to LDS; lanes 0 / 1 of a block add the eight shares in lane order,
//                       take the variance numerators of block and quadrants from the half-row sums (uint64, exact) and write maskeff(A) /
//                       maskeff(B);
//                    4. every lane: M, its eight thresholded coefficients, its share of the block's 64 products (f32, k = 0 .. 7 in order);
//                    5. thread b < 32 adds block b's eight shares in lane order (f32) -- the block's two sums -- and widens them to f64;
//                       thread 0 adds the 32 blocks in order and writes the tile's OWN cell with plain stores.
//                  A block beyond the picture's last full block computes on zeros, which gives zeros.
//   k_hvs_finish   grid (slots)   block 256   lane i adds cells i, i + 256, ... in order, then a fixed two-level tree.
//
// The 8-point DCT is an even / odd factorisation: four sums and four differences, the even half as a 4-point butterfly, the odd half as
// four rows of explicit fmaf() -- 9 multiplies, 14 fused multiply-adds and 14 additions instead of 64 multiply-adds.  The factor
// sqrt(1 / 8) of the DC output is applied after both passes (dct8, scale2d), which keeps the DC path in exact integers.  Under the
// Makefile's -ffp-contract=off these fmaf() calls are the only fused operations.  The order written here IS the definition's f32
// expression; the emulation (tests/hvs_emul) runs this same source.
//
// No atomics; every cell is written by every compute, so nothing is zeroed and nothing is kept between computes.
#pragma once
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::sample1 / load4_raw / unpack4

#define TMH_THREADS 256
#define TMH_BX 16             /* blocks per tile row */
#define TMH_BY 2              /* block rows per tile */
#define TMH_TW (8 * TMH_BX)   /* samples */
#define TMH_TH (8 * TMH_BY)
#define TMH_BLOCKS (TMH_BX * TMH_BY)
#define TMH_MAX_DIM 32768u    /* largest w, h: keeps every byte offset inside a row in an int */

// luma layouts of include/turbo_metrics_hvs.h (VIF's numbering)
enum { TMH_Y8 = 0, TMH_Y16_MSB = 1, TMH_Y16_LOW = 2, TMH_Y10_PACKED = 3 };

// the two published 8x8 tables, [k][l] = [vertical][horizontal frequency], six decimals: CSF = 25.73509 / Q, MASK = (10 / Q)^2 with Q
// the JPEG luminance quantiser
#define TMH_CSF_VALUES                                                                                  \
    {1.608443f, 2.339554f, 2.573509f, 1.608443f, 1.072295f, 0.643377f, 0.504610f, 0.421887f,            \
     2.144591f, 2.144591f, 1.838221f, 1.354478f, 0.989811f, 0.443708f, 0.428918f, 0.467911f,            \
     1.838221f, 1.979622f, 1.608443f, 1.072295f, 0.643377f, 0.451493f, 0.372972f, 0.459555f,            \
     1.838221f, 1.513829f, 1.169777f, 0.887417f, 0.504610f, 0.295806f, 0.321689f, 0.415082f,            \
     1.429727f, 1.169777f, 0.695543f, 0.459555f, 0.378457f, 0.236102f, 0.249855f, 0.334222f,            \
     1.072295f, 0.735288f, 0.467911f, 0.402111f, 0.317717f, 0.247453f, 0.227744f, 0.279729f,            \
     0.525206f, 0.402111f, 0.329937f, 0.295806f, 0.249855f, 0.212687f, 0.214459f, 0.254803f,            \
     0.357432f, 0.279729f, 0.270896f, 0.262603f, 0.229778f, 0.257351f, 0.249855f, 0.259950f}
#define TMH_MASK_VALUES                                                                                 \
    {0.390625f, 0.826446f, 1.000000f, 0.390625f, 0.173611f, 0.062500f, 0.038447f, 0.026874f,            \
     0.694444f, 0.694444f, 0.510204f, 0.277008f, 0.147929f, 0.029727f, 0.027778f, 0.033058f,            \
     0.510204f, 0.591716f, 0.390625f, 0.173611f, 0.062500f, 0.030779f, 0.021004f, 0.031888f,            \
     0.510204f, 0.346021f, 0.206612f, 0.118906f, 0.038447f, 0.013212f, 0.015625f, 0.026015f,            \
     0.308642f, 0.206612f, 0.073046f, 0.031888f, 0.021626f, 0.008417f, 0.009426f, 0.016866f,            \
     0.173611f, 0.081633f, 0.033058f, 0.024414f, 0.015242f, 0.009246f, 0.007831f, 0.011815f,            \
     0.041649f, 0.024414f, 0.016437f, 0.013212f, 0.009426f, 0.006830f, 0.006944f, 0.009803f,            \
     0.019290f, 0.011815f, 0.011080f, 0.010412f, 0.007972f, 0.010000f, 0.009426f, 0.010203f}

// one pair of a slot
struct TmHvsDesc {
    const void *p[2];             // the luma planes: reference, distorted
    unsigned long long pitch[2];  // bytes per row
    int vec;                      // both bases and pitches 16-byte aligned: the wide loads are allowed
    int pad_;
};

// what a tile leaves and what a slot ends with: the f64 sums of the blocks' S2 (PSNR-HVS) and S1 (PSNR-HVS-M)
struct TmHvsCell {
    double s_hvs, s_hvsm;
};

struct TmHvsGeom {
    unsigned w, h;
    int bits, layout;
    int fmt;             // TMX_F_* of the samples
    int shift;           // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;       // TMX_F_U16_LOW: sample = v & mask
    unsigned bw, bh;     // 8x8 blocks
    unsigned tx, ty;     // tiles
    unsigned cells;      // tx * ty: workgroups and cells per slot
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 8 (no block) or above TMH_MAX_DIM, D outside 8 .. 16 or
// not one the layout carries
static inline int tmh_make_geom(TmHvsGeom *g, unsigned w, unsigned h, int layout, unsigned bits)
{
    memset(g, 0, sizeof *g);
    if (w < 8 || h < 8 || w > TMH_MAX_DIM || h > TMH_MAX_DIM || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMH_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMH_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMH_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMH_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->w = w; g->h = h; g->bits = (int)bits; g->layout = layout;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->bw = w >> 3; g->bh = h >> 3;
    g->tx = (g->bw + TMH_BX - 1) / TMH_BX; g->ty = (g->bh + TMH_BY - 1) / TMH_BY;
    g->cells = g->tx * g->ty;
    return 0;
}

namespace tmh {

static __device__ const float kCsf[64] = TMH_CSF_VALUES;
static __device__ const float kMask[64] = TMH_MASK_VALUES;

// a_k cos(k pi / 16): a_0 = sqrt(1 / 8) (which is also cos(4 pi / 16) / 2), a_k = 1 / 2
#define TMH_A0 0.3535533906f
#define TMH_H1 0.4903926402f
#define TMH_H2 0.4619397663f
#define TMH_H3 0.4157348062f
#define TMH_H5 0.2777851165f
#define TMH_H6 0.1913417162f
#define TMH_H7 0.0975451610f

// The orthonormal 8-point DCT-II of x, in place, with ONE output left unscaled: x[0] is the plain sum of the eight inputs, a_0 = sqrt(1 / 8)
// times which is the DC output.  The caller applies that factor after the second pass (scale2d): the row sums of integer samples and
// the sums and differences the column pass takes of them then stay exact integers (64 * 65535 < 2^24), so that the AC coefficients of a
// bright, nearly flat block are not differences of rounded numbers of the size of its DC.
__device__ __forceinline__ void dct8(float (&x)[8])
{
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const float e0 = s0 + s3, e1 = s1 + s2, e2 = s1 - s2, e3 = s0 - s3;
    x[0] = e0 + e1;
    x[4] = TMH_A0 * (e0 - e1);
    x[2] = fmaf(TMH_H6, e2, TMH_H2 * e3);
    x[6] = fmaf(-TMH_H2, e2, TMH_H6 * e3);
    x[1] = fmaf(TMH_H7, d3, fmaf(TMH_H5, d2, fmaf(TMH_H3, d1, TMH_H1 * d0)));
    x[3] = fmaf(-TMH_H5, d3, fmaf(-TMH_H1, d2, fmaf(-TMH_H7, d1, TMH_H3 * d0)));
    x[5] = fmaf(TMH_H3, d3, fmaf(TMH_H7, d2, fmaf(-TMH_H1, d1, TMH_H5 * d0)));
    x[7] = fmaf(-TMH_H1, d3, fmaf(TMH_H3, d2, fmaf(-TMH_H5, d1, TMH_H7 * d0)));
}

// the factors dct8 left out, for column c of the block after both passes: a_0 on row 0 and on column 0, a_0^2 = 1 / 8 on the DC
__device__ __forceinline__ void scale2d(float (&x)[8], unsigned c)
{
    const float rest = c == 0 ? TMH_A0 : 1.0f; // times 1 is exact
    x[0] = x[0] * (c == 0 ? 0.125f : TMH_A0);
#pragma unroll
    for (int k = 1; k < 8; ++k) x[k] = x[k] * rest;
}

struct Lds {
    float ra[TMH_THREADS / 64][64][9], rd[TMH_THREADS / 64][64][9]; // [wave][block of the wave * 8 + row][k]: the row passes of A and A - B
    unsigned s[2][TMH_BLOCKS][8][2];                                // [picture][block][row][half]: sum of z
    unsigned long long ss[2][TMH_BLOCKS][8][2];                     // ... of z^2
    float m[2][TMH_BLOCKS][8];                                      // [picture][block][lane]: shares of the AC energy
    float mk[2][TMH_BLOCKS];                                        // maskeff(A), maskeff(B)
    float p[2][TMH_BLOCKS][8];                                      // [S2, S1][block][lane]: shares of the 64 products
    double blk[2][TMH_BLOCKS];                                      // the blocks' S2, S1
};

// samples x .. x+7 of a row (x a multiple of 8)
template <int FMT>
__device__ __forceinline__ void load_row8(const char *row, bool vec, int x, int shift, unsigned mask, unsigned (&v)[8])
{
    if (vec) {
        const tmx::Raw4 q0 = tmx::load4_raw(row, FMT, x), q1 = tmx::load4_raw(row, FMT, x + 4);
        unsigned lo[4], hi[4];
        tmx::unpack4(q0, FMT, x, shift, mask, lo);
        tmx::unpack4(q1, FMT, x + 4, shift, mask, hi);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = lo[k]; v[4 + k] = hi[k]; }
    } else { // an unaligned picture: sample by sample
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = tmx::sample1(row, FMT, x + k, shift, mask);
    }
}

// 63 * (the four quadrants' variance numerators) over 15 * (the block's): the ratio of the definition's `vari` values, from the
// half-row sums of one picture of one block; 0 for a block of zero variance
__device__ __forceinline__ float pop_of(const unsigned (&s)[8][2], const unsigned long long (&ss)[8][2])
{
    unsigned long long qs = 0, S = 0, SS = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { // rows 4 (q >> 1) .. + 3, half q & 1
        unsigned long long a = 0, b = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) { a += s[4 * (q >> 1) + r][q & 1]; b += ss[4 * (q >> 1) + r][q & 1]; }
        qs += 16ull * b - a * a;
        S += a; SS += b;
    }
    const unsigned long long n64 = 64ull * SS - S * S;
    if (n64 == 0) return 0.0f;
    return (float)(63ull * qs) / (float)(15ull * n64);
}

} // namespace tmh

// desc: [slot]; cells: [slot][g.cells]
template <int FMT>
__global__ void __launch_bounds__(TMH_THREADS) k_hvs(TmHvsGeom g, const TmHvsDesc *__restrict__ desc, TmHvsCell *__restrict__ cells)
{
    using namespace tmh;
    __shared__ Lds L;
    const unsigned tid = threadIdx.x, slot = blockIdx.y, t = blockIdx.x;
    const unsigned wv = tid >> 6, r = (tid >> 3) & 7, bx = tid & 7;
    const unsigned blk = wv * 8 + bx; // the tile's blocks row by row: 16 per block row, a wave owns 8 neighbours
    const unsigned gbx = (t % g.tx) * TMH_BX + (blk % TMH_BX), gby = (t / g.tx) * TMH_BY + blk / TMH_BX;
    const bool has = gbx < g.bw && gby < g.bh;
    const TmHvsDesc d = desc[slot];

    // ---- 1. the lane's row of both pictures
    unsigned a[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = b[k] = 0u;
    if (has) {
        const size_t y = (size_t)(8u * gby + r);
        load_row8<FMT>((const char *)d.p[0] + y * d.pitch[0], d.vec != 0, (int)(8u * gbx), g.shift, g.mask, a);
        load_row8<FMT>((const char *)d.p[1] + y * d.pitch[1], d.vec != 0, (int)(8u * gbx), g.shift, g.mask, b);
    }
    float fa[8], fd[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        unsigned sa = 0, sb = 0;
        unsigned long long qa = 0, qb = 0;
#pragma unroll
        for (int k = 4 * h; k < 4 * h + 4; ++k) {
            sa += a[k]; sb += b[k];
            // samples are below 2^16: the 24-bit multiply gives the whole product
            qa += (unsigned long long)tm_mul24(a[k], a[k]); qb += (unsigned long long)tm_mul24(b[k], b[k]);
        }
        L.s[0][blk][r][h] = sa; L.s[1][blk][r][h] = sb;
        L.ss[0][blk][r][h] = qa; L.ss[1][blk][r][h] = qb;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { fa[k] = (float)a[k]; fd[k] = (float)((int)a[k] - (int)b[k]); }
    dct8(fa);
    dct8(fd);
#pragma unroll
    for (int k = 0; k < 8; ++k) { L.ra[wv][bx * 8 + r][k] = fa[k]; L.rd[wv][bx * 8 + r][k] = fd[k]; }
    TM_LDS_BARRIER();

    // ---- 2. the lane's column: c = r
    const unsigned c = r;
#pragma unroll
    for (int k = 0; k < 8; ++k) { fa[k] = L.ra[wv][bx * 8 + k][c]; fd[k] = L.rd[wv][bx * 8 + k][c]; }
    dct8(fa);
    dct8(fd);
    scale2d(fa, c); // T(A)[k][c]
    scale2d(fd, c); // T(A - B)[k][c]
    float csf[8], msk[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { csf[k] = kCsf[8 * k + c]; msk[k] = kMask[8 * k + c]; }

    // ---- 3. masking
    {
        float ma = 0.0f, mb = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float tb = fa[k] - fd[k]; // T(B)[k][c]
            float ea = (fa[k] * fa[k]) * msk[k], eb = (tb * tb) * msk[k];
            if (k == 0 && c == 0) ea = eb = 0.0f; // the DC term takes no part
            ma += ea; mb += eb;
        }
        L.m[0][blk][c] = ma; L.m[1][blk][c] = mb;
    }
    TM_LDS_BARRIER();
    if (c < 2) { // lane 0: picture A, lane 1: picture B
        float m = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) m += L.m[c][blk][j];
        const float pop = pop_of(L.s[c][blk], L.ss[c][blk]);
        L.mk[c][blk] = sqrtf(m * pop) * 0.03125f;
    }
    TM_LDS_BARRIER();

    // ---- 4. the lane's share of the 64 products
    {
        const float M = fmaxf(L.mk[0][blk], L.mk[1][blk]);
        float p2 = 0.0f, p1 = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float u = fabsf(fd[k]);
            float v = fmaxf(u - M / msk[k], 0.0f);
            if (k == 0 && c == 0) v = u; // the DC term is never masked
            const float t2 = u * csf[k], t1 = v * csf[k];
            p2 += t2 * t2; p1 += t1 * t1;
        }
        L.p[0][blk][c] = p2; L.p[1][blk][c] = p1;
    }
    TM_LDS_BARRIER();

    // ---- 5. blocks, then the tile
    if (tid < TMH_BLOCKS) {
        float s2 = 0.0f, s1 = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) { s2 += L.p[0][tid][j]; s1 += L.p[1][tid][j]; }
        L.blk[0][tid] = (double)s2; L.blk[1][tid] = (double)s1;
    }
    TM_LDS_BARRIER();
    if (tid == 0) {
        TmHvsCell cell = {0.0, 0.0};
        for (int j = 0; j < TMH_BLOCKS; ++j) { cell.s_hvs += L.blk[0][j]; cell.s_hvsm += L.blk[1][j]; }
        cells[(size_t)slot * g.cells + t] = cell;
    }
}

// the launch of the instantiation for g.fmt: the one place that maps a geometry to a kernel (library and emulation)
#define TMH_DISPATCH(g, LAUNCH)                         \
    do {                                                \
        switch ((g).fmt) {                              \
        case TMX_F_U8: LAUNCH(TMX_F_U8); break;         \
        case TMX_F_U16_MSB: LAUNCH(TMX_F_U16_MSB); break; \
        case TMX_F_U16_LOW: LAUNCH(TMX_F_U16_LOW); break; \
        default: LAUNCH(TMX_F_P10); break;              \
        }                                               \
    } while (0)

// grid (slots), block 256: the sum of the slot's cells in a fixed order: lane i adds cells i, i + 256, ..., then 16 sums of 16
// neighbouring lanes, then their sum, each level in index order
__global__ void __launch_bounds__(TMH_THREADS) k_hvs_finish(TmHvsGeom g, const TmHvsCell *__restrict__ cells, TmHvsCell *__restrict__ res)
{
    __shared__ double t2[TMH_THREADS], t1[TMH_THREADS];
    const unsigned tid = threadIdx.x, slot = blockIdx.x;
    const TmHvsCell *cl = cells + (size_t)slot * g.cells;
    double s2 = 0.0, s1 = 0.0;
    for (unsigned i = tid; i < g.cells; i += TMH_THREADS) { s2 += cl[i].s_hvs; s1 += cl[i].s_hvsm; }
    t2[tid] = s2; t1[tid] = s1;
    TM_LDS_BARRIER();
    if (tid < 16) {
        s2 = 0.0; s1 = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { s2 += t2[tid * 16 + k]; s1 += t1[tid * 16 + k]; }
    }
    TM_LDS_BARRIER();
    if (tid < 16) { t2[tid] = s2; t1[tid] = s1; }
    TM_LDS_BARRIER();
    if (tid == 0) {
        s2 = 0.0; s1 = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { s2 += t2[k]; s1 += t1[k]; }
        TmHvsCell out;
        out.s_hvs = s2; out.s_hvsm = s1;
        res[slot] = out;
    }
}
