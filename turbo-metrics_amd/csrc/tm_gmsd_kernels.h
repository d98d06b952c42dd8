// tm_gmsd_kernels.h -- gfx950 kernels of GMSD, the gradient magnitude similarity deviation (libturbometrics_gmsd.so,
// include/turbo_metrics_gmsd.h).
//
// The definition is DESIGN.md section 20; its float64 restatement is tests/gmsd_ref.py.  Per pair of luma planes: the 2x2 sums S of both
// pictures at every second position (four times the decimated mean), the Prewitt gradients of S with zeros beyond the decimated plane,
// A = gx^2 + gy^2 of both pictures in exact integers, then ONE f32 expression per position:
//     e = (sqrtf((float)A_r) - sqrtf((float)A_d))^2 / (float)(A_r + A_d + C),   GMS = 1 - e
// and the f64 sums of e and e^2 and the largest e over the positions.
//
//   k_gmsd<FMT>     grid (tiles, slots)   block 256   one workgroup per tile of TMG_TW x TMG_TH decimated positions = 128 x 64 samples of
//                   one slot's pair.
//                     1. S of the tile and of its halo goes to LDS for both pictures, TMG_LH rows of TMG_LW columns: decimated rows
//                        y0 - 1 .. y0 + TH, decimated columns x0 - 2 .. x0 + TW + 1 (the halo is one column; the second one comes with the
//                        4-sample group that holds the first and is never used).  An item is one group of four samples of two picture rows
//                        of both pictures -- two values of S each: a 4-byte (y8), 8-byte (16-bit) or 16-byte (packed 10-bit) load per row
//                        where base and pitch allow and the whole group lies inside the row, sample by sample otherwise.  Consecutive lanes
//                        take consecutive groups of one row pair.  A sample at column >= w or row >= h is 0 and is not fetched, and so is
//                        everything left of column 0 and above row 0: S = 0 outside the decimated plane falls out of that.
//                     2. lane (c, q) = (tid % 64, tid / 64) owns column c, rows 8 q .. 8 q + 7 of the tile and walks down: per row of S the
//                        horizontal difference d = S[x + 1] - S[x - 1] and the sum t = S[x - 1] + S[x] + S[x + 1]; then
//                        gx = d[y - 1] + d[y] + d[y + 1], gy = t[y + 1] - t[y - 1].  Ten rows of LDS reads for eight positions, consecutive
//                        lanes on consecutive words.  With maps on, the lane stores GMS of each position: a wave writes 64 consecutive
//                        floats of one map row.
//                     3. the lane's e and e^2 are added in f64 in row order; 16 lanes add 16 neighbouring lanes' sums in lane order, lane 0
//                        those 16, and writes the tile's OWN cell with plain stores.
//   k_gmsd_finish   grid (slots)   block 256   lane i adds cells i, i + 256, ... in order, then a fixed two-level tree; the largest e alike.
//
// Under the Makefile's -ffp-contract=off nothing is fused; conversions, square roots and the division are correctly rounded.  The order
// written here IS the definition's f32 expression; the emulation (tests/gmsd_emul) runs this same source.
//
// No atomics; every cell and every map value is written by every compute, so nothing is zeroed and nothing is kept between computes.
#pragma once
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::sample1 / load4_raw / unpack4

#define TMG_THREADS 256
#define TMG_TW 64                 /* decimated positions per tile row */
#define TMG_TH 32                 /* ... per tile column */
#define TMG_LW (TMG_TW + 4)       /* columns of S in LDS: x0 - 2 .. x0 + TW + 1 */
#define TMG_LH (TMG_TH + 2)       /* rows of S in LDS: y0 - 1 .. y0 + TH */
#define TMG_GROUPS (TMG_LW / 2)   /* 4-sample groups per picture row of a tile */
#define TMG_ROWS_PER_LANE (TMG_TH / (TMG_THREADS / TMG_TW))
#define TMG_MIN_DIM 4u
#define TMG_MAX_DIM 32768u        /* largest w, h: keeps every byte offset inside a row in an int */
#define TMG_T 170ull              /* the paper's constant on the 0 .. 255 scale */

// luma layouts of include/turbo_metrics_gmsd.h (VIF's numbering)
enum { TMG_Y8 = 0, TMG_Y16_MSB = 1, TMG_Y16_LOW = 2, TMG_Y10_PACKED = 3 };

// one pair of a slot
struct TmGmsdDesc {
    const void *p[2];             // the luma planes: reference, distorted
    unsigned long long pitch[2];  // bytes per row
    int vec;                      // both bases and pitches 16-byte aligned: the wide loads are allowed
    int pad_;
};

// what a tile leaves and what a slot ends with: the f64 sums of e and of e^2 and the largest e
struct TmGmsdCell {
    double e1, e2;
    float e_max;
    float pad_;
};

struct TmGmsdGeom {
    unsigned w, h;
    int bits, layout;
    int fmt;                 // TMX_F_* of the samples
    int shift;               // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;           // TMX_F_U16_LOW: sample = v & mask
    unsigned w2, h2;         // the decimated plane: ceil(w / 2), ceil(h / 2)
    unsigned tx, ty;         // tiles
    unsigned cells;          // tx * ty: workgroups and cells per slot
    int maps;                // the tiles store GMS
    unsigned long long c;    // 170 * 144 * 4^(bits - 8)
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 4 or above TMG_MAX_DIM, b outside 8 .. 16 or not one the
// layout carries
static inline int tmg_make_geom(TmGmsdGeom *g, unsigned w, unsigned h, int layout, unsigned bits, int maps)
{
    memset(g, 0, sizeof *g);
    if (w < TMG_MIN_DIM || h < TMG_MIN_DIM || w > TMG_MAX_DIM || h > TMG_MAX_DIM || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMG_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMG_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMG_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMG_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->w = w; g->h = h; g->bits = (int)bits; g->layout = layout;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->w2 = (w + 1) / 2; g->h2 = (h + 1) / 2;
    g->tx = (g->w2 + TMG_TW - 1) / TMG_TW; g->ty = (g->h2 + TMG_TH - 1) / TMG_TH;
    g->cells = g->tx * g->ty;
    g->maps = maps != 0;
    g->c = (TMG_T * 144ull) << (2 * (bits - 8));
    return 0;
}

namespace tmg {

struct Lds {
    unsigned s[2][TMG_LH][TMG_LW];   // [picture][row][column]: S
    double e1[TMG_THREADS], e2[TMG_THREADS];
    float mx[TMG_THREADS];
};

// samples x .. x+3 (x a multiple of 4, x >= 0) of one picture row; samples at or beyond w are 0 and are not fetched
template <int FMT>
__device__ __forceinline__ void load_group(const char *row, bool vec, int x, int w, int shift, unsigned mask, unsigned (&v)[4])
{
    if (vec && x + 4 <= w) {
        const tmx::Raw4 q = tmx::load4_raw(row, FMT, x);
        tmx::unpack4(q, FMT, x, shift, mask, v);
    } else { // an unaligned picture or the row's last, partial group: sample by sample
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x + k < w ? tmx::sample1(row, FMT, x + k, shift, mask) : 0u;
    }
}

// gx^2 + gy^2: |g| <= 12 * 65535 < 2^20, the sum is below 2^41
__device__ __forceinline__ unsigned long long grad2(int gx, int gy)
{
    return (unsigned long long)((long long)gx * gx) + (unsigned long long)((long long)gy * gy);
}

// the definition's one f32 expression
__device__ __forceinline__ float e_of(unsigned long long ar, unsigned long long ad, unsigned long long c)
{
    const float mr = sqrtf((float)ar), md = sqrtf((float)ad);
    const float df = mr - md;
    const float num = df * df;
    const float den = (float)(ar + ad + c);
    return num / den;
}

} // namespace tmg

// desc: [slot]; maps: [slot][g.h2][g.w2] (g.maps only); cells: [slot][g.cells]
template <int FMT>
__global__ void __launch_bounds__(TMG_THREADS) k_gmsd(TmGmsdGeom g, const TmGmsdDesc *__restrict__ desc, float *__restrict__ maps, TmGmsdCell *__restrict__ cells)
{
    using namespace tmg;
    __shared__ Lds L;
    const unsigned tid = threadIdx.x, slot = blockIdx.y, t = blockIdx.x;
    const int x0 = (int)((t % g.tx) * TMG_TW), y0 = (int)((t / g.tx) * TMG_TH); // the tile's first decimated position
    const TmGmsdDesc d = desc[slot];

    // ---- 1. S of the tile and its halo
    for (unsigned it = tid; it < TMG_LH * TMG_GROUPS; it += TMG_THREADS) {
        const int j = (int)(it / TMG_GROUPS), gq = (int)(it % TMG_GROUPS);
        const int yy = y0 - 1 + j;            // decimated row
        const int x = 2 * (x0 - 2) + 4 * gq;  // first of the group's four samples: a multiple of 4, or -4
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            unsigned a[4] = {0u, 0u, 0u, 0u}, b[4] = {0u, 0u, 0u, 0u};
            if (yy >= 0 && yy < (int)g.h2 && x >= 0 && x < (int)g.w) {
                const char *row = (const char *)d.p[p] + (size_t)(2 * yy) * d.pitch[p];
                load_group<FMT>(row, d.vec != 0, x, (int)g.w, g.shift, g.mask, a);
                if (2 * yy + 1 < (int)g.h) load_group<FMT>(row + d.pitch[p], d.vec != 0, x, (int)g.w, g.shift, g.mask, b);
            }
            L.s[p][j][2 * gq] = (a[0] + a[1]) + (b[0] + b[1]);
            L.s[p][j][2 * gq + 1] = (a[2] + a[3]) + (b[2] + b[3]);
        }
    }
    TM_LDS_BARRIER();

    // ---- 2. the lane's column: LDS column c + 2 is decimated column x0 + c, LDS row r + 1 is decimated row y0 + r
    const unsigned c = tid % TMG_TW, q = tid / TMG_TW;
    const unsigned gx_ = (unsigned)x0 + c;
    const unsigned r0 = q * TMG_ROWS_PER_LANE;
    int dd[2][3], tt[2][3]; // [picture][row y - 1, y, y + 1]: d and t
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned *s = &L.s[p][r0 + k][c + 1];
            dd[p][k + 1] = (int)s[2] - (int)s[0];
            tt[p][k + 1] = (int)(s[0] + s[1] + s[2]);
        }
    double e1 = 0.0, e2 = 0.0;
    float mx = 0.0f;
    float *mp = maps + ((size_t)slot * g.h2 + (unsigned)y0 + r0) * g.w2 + gx_;
#pragma unroll
    for (int i = 0; i < TMG_ROWS_PER_LANE; ++i) {
        unsigned long long A[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            dd[p][0] = dd[p][1]; dd[p][1] = dd[p][2];
            tt[p][0] = tt[p][1]; tt[p][1] = tt[p][2];
            const unsigned *s = &L.s[p][r0 + i + 2][c + 1];
            dd[p][2] = (int)s[2] - (int)s[0];
            tt[p][2] = (int)(s[0] + s[1] + s[2]);
            A[p] = grad2(dd[p][0] + dd[p][1] + dd[p][2], tt[p][2] - tt[p][0]);
        }
        if (gx_ < g.w2 && (unsigned)y0 + r0 + i < g.h2) {
            const float e = e_of(A[0], A[1], g.c);
            e1 += (double)e;
            e2 += (double)e * (double)e;
            mx = fmaxf(mx, e);
            if (g.maps) mp[(size_t)i * g.w2] = 1.0f - e;
        }
    }
    L.e1[tid] = e1; L.e2[tid] = e2; L.mx[tid] = mx;
    TM_LDS_BARRIER();

    // ---- 3. the tile
    if (tid < 16) {
        e1 = 0.0; e2 = 0.0; mx = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) { e1 += L.e1[tid * 16 + k]; e2 += L.e2[tid * 16 + k]; mx = fmaxf(mx, L.mx[tid * 16 + k]); }
    }
    TM_LDS_BARRIER();
    if (tid < 16) { L.e1[tid] = e1; L.e2[tid] = e2; L.mx[tid] = mx; }
    TM_LDS_BARRIER();
    if (tid == 0) {
        TmGmsdCell cell = {0.0, 0.0, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 16; ++k) { cell.e1 += L.e1[k]; cell.e2 += L.e2[k]; cell.e_max = fmaxf(cell.e_max, L.mx[k]); }
        cells[(size_t)slot * g.cells + t] = cell;
    }
}

// the launch of the instantiation for g.fmt: the one place that maps a geometry to a kernel (library and emulation)
#define TMG_DISPATCH(g, LAUNCH)                         \
    do {                                                \
        switch ((g).fmt) {                              \
        case TMX_F_U8: LAUNCH(TMX_F_U8); break;         \
        case TMX_F_U16_MSB: LAUNCH(TMX_F_U16_MSB); break; \
        case TMX_F_U16_LOW: LAUNCH(TMX_F_U16_LOW); break; \
        default: LAUNCH(TMX_F_P10); break;              \
        }                                               \
    } while (0)

// grid (slots), block 256: the sums of the slot's cells in a fixed order: lane i adds cells i, i + 256, ..., then 16 sums of 16
// neighbouring lanes, then their sum, each level in index order
__global__ void __launch_bounds__(TMG_THREADS) k_gmsd_finish(TmGmsdGeom g, const TmGmsdCell *__restrict__ cells, TmGmsdCell *__restrict__ res)
{
    __shared__ double t1[TMG_THREADS], t2[TMG_THREADS];
    __shared__ float tm[TMG_THREADS];
    const unsigned tid = threadIdx.x, slot = blockIdx.x;
    const TmGmsdCell *cl = cells + (size_t)slot * g.cells;
    double e1 = 0.0, e2 = 0.0;
    float mx = 0.0f;
    for (unsigned i = tid; i < g.cells; i += TMG_THREADS) { e1 += cl[i].e1; e2 += cl[i].e2; mx = fmaxf(mx, cl[i].e_max); }
    t1[tid] = e1; t2[tid] = e2; tm[tid] = mx;
    TM_LDS_BARRIER();
    if (tid < 16) {
        e1 = 0.0; e2 = 0.0; mx = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) { e1 += t1[tid * 16 + k]; e2 += t2[tid * 16 + k]; mx = fmaxf(mx, tm[tid * 16 + k]); }
    }
    TM_LDS_BARRIER();
    if (tid < 16) { t1[tid] = e1; t2[tid] = e2; tm[tid] = mx; }
    TM_LDS_BARRIER();
    if (tid == 0) {
        TmGmsdCell out = {0.0, 0.0, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 16; ++k) { out.e1 += t1[k]; out.e2 += t2[k]; out.e_max = fmaxf(out.e_max, tm[k]); }
        res[slot] = out;
    }
}
