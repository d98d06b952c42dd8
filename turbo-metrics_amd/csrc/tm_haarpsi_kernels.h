// tm_haarpsi_kernels.h -- gfx950 kernels of HaarPSI, the Haar wavelet-based perceptual similarity index (libturbometrics_haarpsi.so,
// include/turbo_metrics_haarpsi.h).
//
// The definition is DESIGN.md section 21; its float64 restatement is tests/haarpsi_ref.py.  Per pair of luma planes: the 2x2 sums S of both
// pictures at every second position (four times the decimated mean), the Haar coefficients Hv_k, Hh_k of S at the scales k = 1, 2, 3
// (windows of 2, 4, 8 positions, zeros beyond the decimated plane) in exact integers, then per position and orientation o ONE f32
// expression:
//     e_k = (float)(a - d)^2 / (float)(a^2 + d^2 + C_k)   (a, d = |H_k| of the two pictures, k = 1, 2)
//     s_o = 1 - (e_1 + e_2) / 2,   q_o = 1 / (1 + exp(4.2f s_o)),   W_o = max(|H_3|) of the two pictures
// and the sums Q = sum (double)q_o W_o (f64, fixed order) and WS = sum W_o (exact).
//
//   k_haarpsi<FMT>   grid (tiles, slots)   block 256   one workgroup per tile of TMP_TW x TMP_TH decimated positions = 128 x 64 samples
//                    of one slot's pair.
//                      1. S of the tile and of its halo goes to LDS for both pictures, TMP_LH rows of TMP_LW columns: decimated rows
//                         y0 - 3 .. y0 + TH + 3, decimated columns x0 - 4 .. x0 + TW + 3 (the halo is 3 before and 4 after; the fourth
//                         column before comes with the 4-sample group that holds the third and is never used).  An item is one group of
//                         four samples of two picture rows of both pictures -- two values of S each: a 4-byte (y8), 8-byte (16-bit) or
//                         16-byte (packed 10-bit) load per row where base and pitch allow and the whole group lies inside the row, sample
//                         by sample otherwise.  A sample at column >= w or row >= h is 0 and is not fetched, and so is everything left of
//                         column 0 and above row 0: S = 0 outside the decimated plane falls out of that.
//                      2. lane (c, q) = (tid % 64, tid / 64) owns column c, rows 8 q .. 8 q + 7 of the tile and walks down 15 rows of S:
//                         per row the sums l_m, r_m of the m = 1, 2, 4 columns ending at x and starting at x + 1 (shared: l_2 = S[x-1] +
//                         l_1, l_4 = S[x-3] + S[x-2] + l_2), hence the row's R_k = l + r and D_k = l - r; a position's Hv_k is the R_k of
//                         its window's upper rows minus those of its lower rows, Hh_k the D_k of all its rows.  Eight LDS words per row
//                         and picture, 30 per position and picture instead of 84 taps; consecutive lanes on consecutive words.  With maps
//                         on, the lane stores (s_v + s_h) / 2 of each position: a wave writes 64 consecutive floats of one map row.
//                      3. the lane's q W are added in f64 in row order, v before h; 16 lanes add 16 neighbouring lanes' sums in lane order,
//                         lane 0 those 16, and writes the tile's OWN cell with plain stores.
//   k_haarpsi_finish grid (slots)   block 256   lane i adds cells i, i + 256, ... in order, then a fixed two-level tree.
//
// exp() is tmp::exp_pos below: no libm call, only operations that are correctly rounded on the device and on a host (explicit fmaf,
// conversions, one multiplication by a power of two).  Under the Makefile's -ffp-contract=off nothing else is fused; conversions and
// divisions are correctly rounded.  The order written here IS the definition's f32 expression; the emulation (tests/haarpsi_emul) runs
// this same source and returns the device's bits.
//
// No atomics; every cell and every map value is written by every compute, so nothing is zeroed and nothing is kept between computes.
#pragma once
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::sample1 / load4_raw / unpack4

#define TMP_THREADS 256
#define TMP_TW 64                 /* decimated positions per tile row */
#define TMP_TH 32                 /* ... per tile column */
#define TMP_HB 3                  /* halo before a position: the 8-window reaches 3 back and 4 ahead */
#define TMP_HA 4
#define TMP_LW (TMP_TW + 8)       /* columns of S in LDS: x0 - 4 .. x0 + TW + 3 */
#define TMP_LH (TMP_TH + TMP_HB + TMP_HA) /* rows of S in LDS: y0 - 3 .. y0 + TH + 3 */
#define TMP_GROUPS (TMP_LW / 2)   /* 4-sample groups per picture row of a tile */
#define TMP_ROWS_PER_LANE (TMP_TH / (TMP_THREADS / TMP_TW))
#define TMP_MIN_DIM 4u
#define TMP_MAX_DIM 32768u        /* largest w, h: keeps every byte offset inside a row in an int */
#define TMP_C 30ull               /* the paper's constant on the 0 .. 255 scale */
#define TMP_A 4.2f                /* the paper's alpha, as the f32 the device multiplies by */

// luma layouts of include/turbo_metrics_haarpsi.h (VIF's numbering)
enum { TMP_Y8 = 0, TMP_Y16_MSB = 1, TMP_Y16_LOW = 2, TMP_Y10_PACKED = 3 };

// one pair of a slot
struct TmHaarpsiDesc {
    const void *p[2];             // the luma planes: reference, distorted
    unsigned long long pitch[2];  // bytes per row
    int vec;                      // both bases and pitches 16-byte aligned: the wide loads are allowed
    int pad_;
};

// what a tile leaves and what a slot ends with: Q = sum q W in f64 and WS = sum W, exact
struct TmHaarpsiCell {
    double q;
    unsigned long long ws;
};

struct TmHaarpsiGeom {
    unsigned w, h;
    int bits, layout;
    int fmt;                 // TMX_F_* of the samples
    int shift;               // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;           // TMX_F_U16_LOW: sample = v & mask
    unsigned w2, h2;         // the decimated plane: ceil(w / 2), ceil(h / 2)
    unsigned tx, ty;         // tiles
    unsigned cells;          // tx * ty: workgroups and cells per slot
    int maps;                // the tiles store the local similarity
    unsigned long long c[2]; // C_k = 30 * 16 * 4^k * 4^(bits - 8), k = 1, 2
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 4 or above TMP_MAX_DIM, b outside 8 .. 16 or not one the
// layout carries
static inline int tmp_make_geom(TmHaarpsiGeom *g, unsigned w, unsigned h, int layout, unsigned bits, int maps)
{
    memset(g, 0, sizeof *g);
    if (w < TMP_MIN_DIM || h < TMP_MIN_DIM || w > TMP_MAX_DIM || h > TMP_MAX_DIM || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMP_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMP_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMP_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMP_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->w = w; g->h = h; g->bits = (int)bits; g->layout = layout;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->w2 = (w + 1) / 2; g->h2 = (h + 1) / 2;
    g->tx = (g->w2 + TMP_TW - 1) / TMP_TW; g->ty = (g->h2 + TMP_TH - 1) / TMP_TH;
    g->cells = g->tx * g->ty;
    g->maps = maps != 0;
    g->c[0] = (TMP_C * 16ull * 4ull) << (2 * (bits - 8));
    g->c[1] = (TMP_C * 16ull * 16ull) << (2 * (bits - 8));
    return 0;
}

namespace tmp {

struct Lds {
    unsigned s[2][TMP_LH][TMP_LW];   // [picture][row][column]: S
    double q[TMP_THREADS];
    unsigned long long ws[TMP_THREADS];
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

// e_k of one orientation and scale from the two coefficients: |H_2| <= 16 * 4 * 65535 < 2^22, so |a - d| < 2^22 is exact in f32 and
// a^2 + d^2 + C < 2^46
__device__ __forceinline__ float e_of(int hr, int hd, unsigned long long c)
{
    const int a = hr < 0 ? -hr : hr, d = hd < 0 ? -hd : hd;
    const float df = (float)(a - d);
    const float num = df * df;
    const float den = (float)((unsigned long long)((long long)a * a) + (unsigned long long)((long long)d * d) + c);
    return num / den;
}

// exp(z) for z in [0, 4.2]: n = round(z log2 e), r = z - n ln 2 by a two-constant Cody-Waite reduction (|r| <= 0.3466 + 1e-6: n ln2_hi
// is exact, n <= 6 and ln2_hi has 9 trailing zero bits), the degree-7 Taylor polynomial of exp(r) (remainder below r^8 / 8! = 5.2e-9
// relative) and 2^n by exponent arithmetic.  Every operation is an fmaf, a conversion or a multiplication: correctly rounded wherever
// it runs.
__device__ __forceinline__ float exp_pos(float z)
{
    const int n = (int)(z * 1.44269502f + 0.5f);
    const float nf = (float)n;
    float r = fmaf(-nf, 0.693145752f, z);   // 0x3F317200
    r = fmaf(-nf, 1.42860677e-6f, r);       // ln 2 - 0x3F317200
    float p = 1.0f / 5040.0f;
    p = fmaf(p, r, 1.0f / 720.0f);
    p = fmaf(p, r, 1.0f / 120.0f);
    p = fmaf(p, r, 1.0f / 24.0f);
    p = fmaf(p, r, 1.0f / 6.0f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    return p * __uint_as_float((unsigned)(n + 127) << 23);
}

// the local similarity s_o of one orientation from its scale-1 and scale-2 coefficients of both pictures
__device__ __forceinline__ float s_of(int r1, int d1, int r2, int d2, unsigned long long c1, unsigned long long c2)
{
    const float e1 = e_of(r1, d1, c1), e2 = e_of(r2, d2, c2);
    return 1.0f - 0.5f * (e1 + e2);
}

// q_o = 1 - sigmoid(A s_o)
__device__ __forceinline__ float q_of(float s)
{
    return 1.0f / (1.0f + exp_pos(TMP_A * s));
}

// W_o: the larger |H_3|, below 2^25
__device__ __forceinline__ unsigned w_of(int hr, int hd)
{
    const unsigned a = (unsigned)(hr < 0 ? -hr : hr), d = (unsigned)(hd < 0 ? -hd : hd);
    return a > d ? a : d;
}

} // namespace tmp

// desc: [slot]; maps: [slot][g.h2][g.w2] (g.maps only); cells: [slot][g.cells]
template <int FMT>
__global__ void __launch_bounds__(TMP_THREADS) k_haarpsi(TmHaarpsiGeom g, const TmHaarpsiDesc *__restrict__ desc, float *__restrict__ maps, TmHaarpsiCell *__restrict__ cells)
{
    using namespace tmp;
    __shared__ Lds L;
    const unsigned tid = threadIdx.x, slot = blockIdx.y, t = blockIdx.x;
    const int x0 = (int)((t % g.tx) * TMP_TW), y0 = (int)((t / g.tx) * TMP_TH); // the tile's first decimated position
    const TmHaarpsiDesc d = desc[slot];

    // ---- 1. S of the tile and its halo
    for (unsigned it = tid; it < TMP_LH * TMP_GROUPS; it += TMP_THREADS) {
        const int j = (int)(it / TMP_GROUPS), gq = (int)(it % TMP_GROUPS);
        const int yy = y0 - TMP_HB + j;       // decimated row
        const int x = 2 * (x0 - 4) + 4 * gq;  // first of the group's four samples: a multiple of 4, or negative
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

    // ---- 2. the lane's column: LDS column c + 4 is decimated column x0 + c, LDS row r + 3 is decimated row y0 + r.  Ring slot j % 8
    // holds R_k, D_k of LDS row r0 + j; position i of the lane (LDS row r0 + i + 3) is complete once row r0 + i + 7 is in
    const unsigned c = tid % TMP_TW, q = tid / TMP_TW;
    const unsigned gx_ = (unsigned)x0 + c;
    const unsigned r0 = q * TMP_ROWS_PER_LANE;
    int R[2][3][8], D[2][3][8]; // [picture][k - 1][ring]
    double qs = 0.0;
    unsigned long long ws = 0ull;
#pragma unroll
    for (int j = 0; j < TMP_ROWS_PER_LANE + 7; ++j) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const unsigned *s = &L.s[p][r0 + j][c + 1]; // s[0 .. 7]: decimated columns x - 3 .. x + 4
            const int l1 = (int)s[3], r1 = (int)s[4];
            const int l2 = (int)s[2] + l1, r2 = r1 + (int)s[5];
            const int l4 = ((int)s[0] + (int)s[1]) + l2, r4 = r2 + ((int)s[6] + (int)s[7]);
            R[p][0][j & 7] = l1 + r1; D[p][0][j & 7] = l1 - r1;
            R[p][1][j & 7] = l2 + r2; D[p][1][j & 7] = l2 - r2;
            R[p][2][j & 7] = l4 + r4; D[p][2][j & 7] = l4 - r4;
        }
        if (j < 7) continue;
        const int i = j - 7; // ring slots of LDS rows r0 + i .. r0 + i + 7: (i + m) & 7
        int hv[2][3], hh[2][3];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#define TMP_AT(A, k, m) A[p][k][(i + (m)) & 7]
            hv[p][0] = TMP_AT(R, 0, 3) - TMP_AT(R, 0, 4);
            hh[p][0] = TMP_AT(D, 0, 3) + TMP_AT(D, 0, 4);
            hv[p][1] = (TMP_AT(R, 1, 2) + TMP_AT(R, 1, 3)) - (TMP_AT(R, 1, 4) + TMP_AT(R, 1, 5));
            hh[p][1] = (TMP_AT(D, 1, 2) + TMP_AT(D, 1, 3)) + (TMP_AT(D, 1, 4) + TMP_AT(D, 1, 5));
            hv[p][2] = ((TMP_AT(R, 2, 0) + TMP_AT(R, 2, 1)) + (TMP_AT(R, 2, 2) + TMP_AT(R, 2, 3))) - ((TMP_AT(R, 2, 4) + TMP_AT(R, 2, 5)) + (TMP_AT(R, 2, 6) + TMP_AT(R, 2, 7)));
            hh[p][2] = ((TMP_AT(D, 2, 0) + TMP_AT(D, 2, 1)) + (TMP_AT(D, 2, 2) + TMP_AT(D, 2, 3))) + ((TMP_AT(D, 2, 4) + TMP_AT(D, 2, 5)) + (TMP_AT(D, 2, 6) + TMP_AT(D, 2, 7)));
#undef TMP_AT
        }
        if (gx_ < g.w2 && (unsigned)y0 + r0 + i < g.h2) {
            const float sv = s_of(hv[0][0], hv[1][0], hv[0][1], hv[1][1], g.c[0], g.c[1]);
            const float sh = s_of(hh[0][0], hh[1][0], hh[0][1], hh[1][1], g.c[0], g.c[1]);
            const unsigned wv = w_of(hv[0][2], hv[1][2]), wh = w_of(hh[0][2], hh[1][2]);
            qs += (double)q_of(sv) * (double)wv;
            qs += (double)q_of(sh) * (double)wh;
            ws += (unsigned long long)wv + wh;
            if (g.maps) maps[((size_t)slot * g.h2 + (unsigned)y0 + r0 + i) * g.w2 + gx_] = 0.5f * (sv + sh);
        }
    }
    L.q[tid] = qs; L.ws[tid] = ws;
    TM_LDS_BARRIER();

    // ---- 3. the tile
    if (tid < 16) {
        qs = 0.0; ws = 0ull;
#pragma unroll
        for (int k = 0; k < 16; ++k) { qs += L.q[tid * 16 + k]; ws += L.ws[tid * 16 + k]; }
    }
    TM_LDS_BARRIER();
    if (tid < 16) { L.q[tid] = qs; L.ws[tid] = ws; }
    TM_LDS_BARRIER();
    if (tid == 0) {
        TmHaarpsiCell cell = {0.0, 0ull};
#pragma unroll
        for (int k = 0; k < 16; ++k) { cell.q += L.q[k]; cell.ws += L.ws[k]; }
        cells[(size_t)slot * g.cells + t] = cell;
    }
}

// the launch of the instantiation for g.fmt: the one place that maps a geometry to a kernel (library and emulation)
#define TMP_DISPATCH(g, LAUNCH)                         \
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
__global__ void __launch_bounds__(TMP_THREADS) k_haarpsi_finish(TmHaarpsiGeom g, const TmHaarpsiCell *__restrict__ cells, TmHaarpsiCell *__restrict__ res)
{
    __shared__ double tq[TMP_THREADS];
    __shared__ unsigned long long tw[TMP_THREADS];
    const unsigned tid = threadIdx.x, slot = blockIdx.x;
    const TmHaarpsiCell *cl = cells + (size_t)slot * g.cells;
    double qs = 0.0;
    unsigned long long ws = 0ull;
    for (unsigned i = tid; i < g.cells; i += TMP_THREADS) { qs += cl[i].q; ws += cl[i].ws; }
    tq[tid] = qs; tw[tid] = ws;
    TM_LDS_BARRIER();
    if (tid < 16) {
        qs = 0.0; ws = 0ull;
#pragma unroll
        for (int k = 0; k < 16; ++k) { qs += tq[tid * 16 + k]; ws += tw[tid * 16 + k]; }
    }
    TM_LDS_BARRIER();
    if (tid < 16) { tq[tid] = qs; tw[tid] = ws; }
    TM_LDS_BARRIER();
    if (tid == 0) {
        TmHaarpsiCell out = {0.0, 0ull};
#pragma unroll
        for (int k = 0; k < 16; ++k) { out.q += tq[k]; out.ws += tw[k]; }
        res[slot] = out;
    }
}
