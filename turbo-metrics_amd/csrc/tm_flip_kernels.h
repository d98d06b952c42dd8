// tm_flip_kernels.h -- gfx950 kernels of LDR-FLIP (libturbometrics_flip.so, include/turbo_metrics_flip.h).
//
// The definition is DESIGN.md section 14; its float64 restatement is tests/flip_ref.py.  Per pair of packed sRGB8 pictures: three f32
// maps (FLIP, the colour difference dEc, the feature difference dEf) and, per picture, the f64 sum, the minimum and the maximum of the
// FLIP map.  All arithmetic of a pixel is f32 with the operations written here (the build has -ffp-contract=off: nothing is fused),
// except pow_pos (f64 inside, one rounding) and the f64 sums.
//
//   k_flip_tile     grid (tiles, slots)   block 256   one workgroup per TMF_TW x TMF_TH = 64 x 16 tile of one slot's pair.  One side
//                   after the other (the LDS of one side is 73 KB, so two workgroups share a CU; both sides at once would be one):
//                     load     the tile and a halo of TMF_HALO = 10, 84 x 36 pixels, coordinates clamped into the picture (edge
//                              replication happens HERE and nowhere else), sRGB8 -> linear through a 256-entry table -> y, Cx, Cz in LDS
//                              (Y = 116 y - 16 is formed from y where it is read: the same operation on the same value)
//                     rows     the four spatial filters (Y, Cx, Cz1, Cz2) of the 36 x 64 positions a column pass reads, into LDS
//                     columns  the same filters down the columns, 4 rows of one column per lane, in registers; then YCxCz -> linear RGB,
//                              clamp, -> Hunt-adjusted Lab, kept in registers
//                     rows     G, G', G'' of y into the same LDS planes;  columns: the edge and point responses and their norms
//                   then per pixel HyAB, the power 0.7, the redistribution, dEf, FLIP; three plain f32 stores; the workgroup's f64
//                   sum / min / max of its FLIP values go through a fixed LDS tree to the tile's own cell.
//                   A tap loop always runs the 21 taps of the halo: a smaller radius has zero weights outside (w x = +-0 adds nothing).
//   k_flip_finish   grid (slots)   block 256   lane l adds cells l, l + 256, ... in that order, then the same fixed tree: every cell is
//                   written by every compute, nothing is zeroed, no float atomics, and two computes give identical bits.
#pragma once
#include <math.h>
#include <string.h>

#include "tm_platform.h"
#include "tm_device_math.h"
#include "tm_math_tables.inc"

#define TMF_THREADS 256
#define TMF_TW 64
#define TMF_TH 16
#define TMF_HALO 10                      /* the largest radius a tile's halo holds */
#define TMF_TAPS (2 * TMF_HALO + 1)
#define TMF_IW (TMF_TW + 2 * TMF_HALO)   /* 84 */
#define TMF_IH (TMF_TH + 2 * TMF_HALO)   /* 36 */
#define TMF_ROWS_PER_LANE (TMF_TW * TMF_TH / TMF_THREADS) /* 4 */
#define TMF_PPD_MIN 8.0
#define TMF_PPD_MAX 256.0
#define TMF_DEFAULT_PPD 67.02064327658226 /* 0.7 * 3840 / 0.7 * pi / 180 */

enum { TMF_RGB8 = 0 };
enum { TMF_MAP = 0, TMF_MAP_COLOR = 1, TMF_MAP_FEATURE = 2, TMF_MAPS = 3 };

// one pair of a slot
struct TmFlipDesc {
    const unsigned char *p[2];   // reference, distorted
    unsigned long long pitch[2]; // bytes
};

// everything a workgroup needs that is not a picture: a kernel argument (constant memory; the unrolled tap loops read it with scalar loads)
struct TmFlipGeom {
    unsigned w, h, tiles_x, tiles_y;
    unsigned r_spatial, r_feature;
    float ws[4][TMF_TAPS]; // Y, Cx, Cz1, Cz2: tap k - TMF_HALO at index k, 0 outside the radius
    float wf[3][TMF_TAPS]; // G, G', G''
    float mn[3][3];        // linear RGB -> XYZ / illuminant
    float mi[3][3];        // XYZ / illuminant -> linear RGB
    float pccmax;          // pc cmax
    float k_lo;            // pt / (pc cmax)
    float k_hi;            // (1 - pt) / (cmax - pc cmax)
    float pt;
    double cmax;           // host only
    double n;              // w h
};

struct TmFlipTables {
    double pow_tab[TM_TAB_POW_DOUBLES]; // pow_pos
    float lut[256];                     // sRGB8 -> linear
};

struct TmFlipCell { double sum; float mn, mx; };
struct TmFlipRes { double mean, mn, mx; };

// ---- host side of the definition (f64, rounded once to f32) -----------------------------------------------------------------------
static inline void tmf_radius(double ppd, unsigned *r_spatial, unsigned *r_feature)
{
    const double pi = 3.14159265358979323846;
    *r_spatial = (unsigned)ceil(3.0 * sqrt(0.04 / (2.0 * pi * pi)) * ppd);
    *r_feature = (unsigned)ceil(3.0 * 0.5 * 0.082 * ppd);
}

static inline double tmf_lab_f(double t)
{
    const double d = 6.0 / 29.0;
    return t > d * d * d ? cbrt(t) : t / (3.0 * d * d) + 4.0 / 29.0;
}

// Hunt-adjusted Lab of XYZ / illuminant
static inline void tmf_hunt(const double n[3], double out[3])
{
    const double fx = tmf_lab_f(n[0]), fy = tmf_lab_f(n[1]), fz = tmf_lab_f(n[2]);
    const double L = 116.0 * fy - 16.0;
    out[0] = L; out[1] = 0.01 * L * 500.0 * (fx - fy); out[2] = 0.01 * L * 200.0 * (fy - fz);
}

// 0; -1: what the library refuses as TM_ERR_UNSUPPORTED (a size of 0 or above 2^31 samples, another layout, a ppd outside 8 .. 256 or
// one whose spatial radius the halo does not hold)
static inline int tmf_make_geom(TmFlipGeom *g, TmFlipTables *t, unsigned w, unsigned h, int layout, double ppd)
{
    memset(g, 0, sizeof *g);
    if (w == 0 || h == 0 || (unsigned long long)w * h > (1ull << 31) || layout != TMF_RGB8) return -1;
    if (!(ppd >= TMF_PPD_MIN && ppd <= TMF_PPD_MAX)) return -1;
    unsigned rs, rf;
    tmf_radius(ppd, &rs, &rf);
    if (rs > TMF_HALO || rf > TMF_HALO) return -1;
    g->w = w; g->h = h;
    g->tiles_x = (w + TMF_TW - 1) / TMF_TW; g->tiles_y = (h + TMF_TH - 1) / TMF_TH;
    g->r_spatial = rs; g->r_feature = rf;
    g->n = (double)w * (double)h;
    const double pi = 3.14159265358979323846;
    const int R = (int)rs, F = (int)rf;

    // spatial filters: g_b(d) = exp(-pi^2 d^2 / b), d = k / ppd; every 2-D filter sums to 1
    double gy[TMF_TAPS] = {0}, gx[TMF_TAPS] = {0}, g1[TMF_TAPS] = {0}, g2[TMF_TAPS] = {0};
    double sy = 0, sx = 0, s1 = 0, s2 = 0;
    for (int k = -R; k <= R; ++k) {
        const double d2 = ((double)k / ppd) * ((double)k / ppd), p2 = pi * pi;
        sy += gy[k + TMF_HALO] = exp(-p2 * d2 / 0.0047);
        sx += gx[k + TMF_HALO] = exp(-p2 * d2 / 0.0053);
        s1 += g1[k + TMF_HALO] = exp(-p2 * d2 / 0.04);
        s2 += g2[k + TMF_HALO] = exp(-p2 * d2 / 0.025);
    }
    const double a1 = 34.1 * sqrt(pi / 0.04), a2 = 13.5 * sqrt(pi / 0.025);
    const double S = a1 * s1 * s1 + a2 * s2 * s2; // the sum of the joint 2-D Cz filter; each separable term carries sqrt(a_i / S) per pass
    for (int k = 0; k < TMF_TAPS; ++k) {
        g->ws[0][k] = (float)(gy[k] / sy);
        g->ws[1][k] = (float)(gx[k] / sx);
        g->ws[2][k] = (float)(g1[k] * sqrt(a1 / S));
        g->ws[3][k] = (float)(g2[k] * sqrt(a2 / S));
    }

    // feature filters, in pixel units
    const double sd = 0.5 * 0.082 * ppd;
    double G[TMF_TAPS] = {0}, G1[TMF_TAPS] = {0}, G2[TMF_TAPS] = {0};
    double sg = 0;
    for (int k = -F; k <= F; ++k) sg += G[k + TMF_HALO] = exp(-(double)(k * k) / (2.0 * sd * sd));
    double p1 = 0, n1 = 0, p2s = 0, n2 = 0;
    for (int k = -F; k <= F; ++k) {
        const int i = k + TMF_HALO;
        G[i] /= sg;
        G1[i] = -(double)k * G[i];
        G2[i] = ((double)(k * k) / (sd * sd) - 1.0) * G[i];
        if (G1[i] > 0) p1 += G1[i]; else n1 -= G1[i];
        if (G2[i] > 0) p2s += G2[i]; else n2 -= G2[i];
    }
    for (int k = 0; k < TMF_TAPS; ++k) {
        g->wf[0][k] = (float)G[k];
        g->wf[1][k] = (float)(G1[k] > 0 ? G1[k] / p1 : (G1[k] < 0 ? G1[k] / n1 : 0.0));
        g->wf[2][k] = (float)(G2[k] > 0 ? G2[k] / p2s : (G2[k] < 0 ? G2[k] / n2 : 0.0));
    }

    // colour: linear RGB -> XYZ (the rows sum to the illuminant), over the illuminant; and the inverse
    const double M[3][3] = {{10135552.0 / 24577794.0, 8788810.0 / 24577794.0, 4435075.0 / 24577794.0},
                            {2613072.0 / 12288897.0, 8788810.0 / 12288897.0, 887015.0 / 12288897.0},
                            {1425312.0 / 73733382.0, 8788810.0 / 73733382.0, 70074185.0 / 73733382.0}};
    const double ill[3] = {0.950428545, 1.0, 1.088900371};
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                       M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    double I[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const int a = (j + 1) % 3, b = (j + 2) % 3, c = (i + 1) % 3, d = (i + 2) % 3;
            I[i][j] = (M[a][c] * M[b][d] - M[a][d] * M[b][c]) / det;
        }
    double Mn[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            Mn[i][j] = M[i][j] / ill[i];
            g->mn[i][j] = (float)Mn[i][j];
            g->mi[i][j] = (float)(I[i][j] * ill[j]);
        }

    // cmax = HyAB(hunt(lab(green)), hunt(lab(blue)))^0.7
    const double ng[3] = {Mn[0][1], Mn[1][1], Mn[2][1]}, nb[3] = {Mn[0][2], Mn[1][2], Mn[2][2]};
    double hg[3], hb[3];
    tmf_hunt(ng, hg);
    tmf_hunt(nb, hb);
    const double cmax = pow(fabs(hg[0] - hb[0]) + sqrt((hg[1] - hb[1]) * (hg[1] - hb[1]) + (hg[2] - hb[2]) * (hg[2] - hb[2])), 0.7);
    const double pc = 0.4, pt = 0.95;
    g->cmax = cmax;
    g->pccmax = (float)(pc * cmax);
    g->k_lo = (float)(pt / (pc * cmax));
    g->k_hi = (float)((1.0 - pt) / (cmax - pc * cmax));
    g->pt = (float)pt;

    if (t) {
        const double rcp[32] = {TM_POW_RCP}, nlog[32] = {TM_POW_NLOG}, ex[32] = {TM_POW_EXP2};
        for (int i = 0; i < 32; ++i) { t->pow_tab[i] = rcp[i]; t->pow_tab[32 + i] = nlog[i]; t->pow_tab[64 + i] = ex[i]; }
        for (int v = 0; v < 256; ++v) {
            const double c = (double)v / 255.0;
            t->lut[v] = (float)(c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4));
        }
    }
    return 0;
}

namespace tmf {

// CIELab's f: the cube root above (6/29)^3, the line below
__device__ __forceinline__ float lab_f(float t)
{
    return t > 0.0088564516790356308f /* (6/29)^3 */ ? tmdev::cbrt_pos(t) : t * 7.7870370370370370f /* 841/108 */ + 0.13793103448275862f /* 4/29 */;
}

// filtered Y, Cx, Cz -> Hunt-adjusted Lab (step 3)
__device__ __forceinline__ void hunt_lab(const TmFlipGeom &g, float Y, float Cx, float Cz, float (&out)[3])
{
    const float y = (Y + 16.0f) / 116.0f, x = y + Cx / 500.0f, z = y - Cz / 200.0f;
    float rgb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) rgb[i] = tmdev::clamp01(g.mi[i][0] * x + g.mi[i][1] * y + g.mi[i][2] * z);
    float f[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) f[i] = lab_f(g.mn[i][0] * rgb[0] + g.mn[i][1] * rgb[1] + g.mn[i][2] * rgb[2]);
    const float L = 116.0f * f[1] - 16.0f, a = 500.0f * (f[0] - f[1]), b = 200.0f * (f[1] - f[2]);
    out[0] = L; out[1] = (0.01f * L) * a; out[2] = (0.01f * L) * b;
}

// one filter down column c of a row-pass plane: out[j] = sum over k = 0 .. 20, in that order, of wt[k] plane[r0 + j + k][c];
// CENTRED (the zero-sum filters G', G''): of wt[k] (plane[r0 + j + k][c] - plane[r0 + j + 10][c])
template <bool CENTRED>
__device__ __forceinline__ void column(const float (*plane)[TMF_TW], unsigned r0, unsigned c, const float (&wt)[TMF_TAPS], float (&out)[TMF_ROWS_PER_LANE])
{
    float v[TMF_ROWS_PER_LANE + TMF_TAPS - 1];
#pragma unroll
    for (int t = 0; t < TMF_ROWS_PER_LANE + TMF_TAPS - 1; ++t) v[t] = plane[r0 + t][c];
#pragma unroll
    for (int j = 0; j < TMF_ROWS_PER_LANE; ++j) {
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < TMF_TAPS; ++k) a = a + wt[k] * (CENTRED ? v[j + k] - v[j + TMF_HALO] : v[j + k]);
        out[j] = a;
    }
}

} // namespace tmf

__global__ void __launch_bounds__(TMF_THREADS) TM_WAVES_PER_SIMD(2) k_flip_tile(TmFlipGeom g, const TmFlipTables *__restrict__ tabs, const TmFlipDesc *__restrict__ desc,
                                                           float *__restrict__ maps, TmFlipCell *__restrict__ cells)
{
    __shared__ float s_in[3][TMF_IH][TMF_IW];  // y, Cx, Cz of one side
    __shared__ float s_row[4][TMF_IH][TMF_TW]; // the row pass: Y, Cx, Cz1, Cz2, then G, G', G'' of y
    __shared__ double s_pow[TM_TAB_POW_DOUBLES];
    __shared__ float s_lut[256];
    __shared__ double s_sum[TMF_THREADS];
    __shared__ float s_mn[TMF_THREADS], s_mx[TMF_THREADS];

    const unsigned tid = threadIdx.x, tile = blockIdx.x, slot = blockIdx.y;
    const unsigned tx = tile % g.tiles_x, ty = tile / g.tiles_x;
    const long long x0 = (long long)tx * TMF_TW, y0 = (long long)ty * TMF_TH;
    const unsigned c = tid & (TMF_TW - 1), q = tid / TMF_TW; // this lane's column and its rows 4 q .. 4 q + 3 of the tile
    const TmFlipDesc d = desc[slot];

    s_lut[tid] = tabs->lut[tid];
    if (tid < TM_TAB_POW_DOUBLES) s_pow[tid] = tabs->pow_tab[tid];

    float lab[2][TMF_ROWS_PER_LANE][3], edge[2][TMF_ROWS_PER_LANE], point[2][TMF_ROWS_PER_LANE];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        TM_LDS_BARRIER(); // the tables; and the column pass of the side before has read s_row
        const unsigned char *base = d.p[side];
        const size_t pitch = (size_t)d.pitch[side];
#pragma unroll 1
        for (unsigned i = tid; i < TMF_IH * TMF_IW; i += TMF_THREADS) {
            const unsigned r = i / TMF_IW, cc = i % TMF_IW;
            long long px = x0 + (long long)cc - TMF_HALO, py = y0 + (long long)r - TMF_HALO;
            px = px < 0 ? 0 : (px > (long long)g.w - 1 ? (long long)g.w - 1 : px);
            py = py < 0 ? 0 : (py > (long long)g.h - 1 ? (long long)g.h - 1 : py);
            const unsigned char *p = base + (size_t)py * pitch + (size_t)px * 3u;
            const float R = s_lut[p[0]], G = s_lut[p[1]], B = s_lut[p[2]];
            const float x = g.mn[0][0] * R + g.mn[0][1] * G + g.mn[0][2] * B;
            const float y = g.mn[1][0] * R + g.mn[1][1] * G + g.mn[1][2] * B;
            const float z = g.mn[2][0] * R + g.mn[2][1] * G + g.mn[2][2] * B;
            s_in[0][r][cc] = y;
            s_in[1][r][cc] = 500.0f * (x - y);
            s_in[2][r][cc] = 200.0f * (y - z);
        }
        TM_LDS_BARRIER();
        // ---- spatial filter, rows (one channel after the other: 21 or 42 weights are live at a time)
#pragma unroll 1
        for (unsigned i = tid; i < TMF_IH * TMF_TW; i += TMF_THREADS) {
            const unsigned r = i / TMF_TW, cc = i % TMF_TW;
            float aY = 0.0f, aX = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
            for (int k = 0; k < TMF_TAPS; ++k) aY = aY + g.ws[0][k] * (116.0f * s_in[0][r][cc + k] - 16.0f);
            s_row[0][r][cc] = aY;
#pragma unroll
            for (int k = 0; k < TMF_TAPS; ++k) aX = aX + g.ws[1][k] * s_in[1][r][cc + k];
            s_row[1][r][cc] = aX;
#pragma unroll
            for (int k = 0; k < TMF_TAPS; ++k) {
                const float Cz = s_in[2][r][cc + k];
                a1 = a1 + g.ws[2][k] * Cz;
                a2 = a2 + g.ws[3][k] * Cz;
            }
            s_row[2][r][cc] = a1; s_row[3][r][cc] = a2;
        }
        TM_LDS_BARRIER();
        // ---- spatial filter, columns; then Hunt-adjusted Lab
        {
            float f[4][TMF_ROWS_PER_LANE];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) tmf::column<false>(s_row[ch], q * TMF_ROWS_PER_LANE, c, g.ws[ch], f[ch]);
#pragma unroll
            for (int j = 0; j < TMF_ROWS_PER_LANE; ++j) tmf::hunt_lab(g, f[0][j], f[1][j], f[2][j] + f[3][j], lab[side][j]);
        }
        TM_LDS_BARRIER();
        // ---- feature filters of the unfiltered y, rows
#pragma unroll 1
        for (unsigned i = tid; i < TMF_IH * TMF_TW; i += TMF_THREADS) {
            const unsigned r = i / TMF_TW, cc = i % TMF_TW;
            // G' and G'' sum to zero: they act on the differences from the centre sample, which are exactly 0 on a flat row, where
            // sum w y would leave the products' rounding -- 1e-8, which the square root of step 5 turns into 1e-4
            const float yc = s_in[0][r][cc + TMF_HALO];
            float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
#pragma unroll
            for (int k = 0; k < TMF_TAPS; ++k) {
                const float y = s_in[0][r][cc + k];
                b0 = b0 + g.wf[0][k] * y;
                b1 = b1 + g.wf[1][k] * (y - yc);
                b2 = b2 + g.wf[2][k] * (y - yc);
            }
            s_row[0][r][cc] = b0; s_row[1][r][cc] = b1; s_row[2][r][cc] = b2;
        }
        TM_LDS_BARRIER();
        // ---- columns: edge = (G'x G y, G x G'y), point = (G''x G y, G x G''y)
        {
            float ex[TMF_ROWS_PER_LANE], ey[TMF_ROWS_PER_LANE], px[TMF_ROWS_PER_LANE], py[TMF_ROWS_PER_LANE];
            tmf::column<false>(s_row[1], q * TMF_ROWS_PER_LANE, c, g.wf[0], ex);
            tmf::column<true>(s_row[0], q * TMF_ROWS_PER_LANE, c, g.wf[1], ey);
            tmf::column<false>(s_row[2], q * TMF_ROWS_PER_LANE, c, g.wf[0], px);
            tmf::column<true>(s_row[0], q * TMF_ROWS_PER_LANE, c, g.wf[2], py);
#pragma unroll
            for (int j = 0; j < TMF_ROWS_PER_LANE; ++j) {
                edge[side][j] = sqrtf(ex[j] * ex[j] + ey[j] * ey[j]);
                point[side][j] = sqrtf(px[j] * px[j] + py[j] * py[j]);
            }
        }
    }

    // ---- steps 4 - 6 per pixel
    double sum = 0.0;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    const size_t plane = (size_t)g.w * g.h;
    float *out = maps + (size_t)slot * TMF_MAPS * plane;
#pragma unroll
    for (int j = 0; j < TMF_ROWS_PER_LANE; ++j) {
        const long long px = x0 + c, py = y0 + q * TMF_ROWS_PER_LANE + j;
        const float dL = fabsf(lab[0][j][0] - lab[1][j][0]), da = lab[0][j][1] - lab[1][j][1], db = lab[0][j][2] - lab[1][j][2];
        const float hyab = dL + sqrtf(da * da + db * db);
        const float e = tmdev::pow_pos(hyab, 0.7, s_pow);
        const float dEc = e < g.pccmax ? e * g.k_lo : g.pt + (e - g.pccmax) * g.k_hi;
        const float fd = fmaxf(fabsf(edge[0][j] - edge[1][j]), fabsf(point[0][j] - point[1][j]));
        const float dEf = sqrtf(fd * 0.70710678118654752f /* 1 / sqrt 2 */);
        const float flip = dEc > 0.0f ? exp2f((1.0f - dEf) * log2f(dEc)) : 0.0f;
        if (px < (long long)g.w && py < (long long)g.h) {
            const size_t o = (size_t)py * g.w + (size_t)px;
            out[o] = flip;
            out[plane + o] = dEc;
            out[2 * plane + o] = dEf;
            sum += (double)flip;
            mn = fminf(mn, flip);
            mx = fmaxf(mx, flip);
        }
    }
    s_sum[tid] = sum; s_mn[tid] = mn; s_mx[tid] = mx;
    for (unsigned s = TMF_THREADS / 2; s > 0; s >>= 1) {
        TM_LDS_BARRIER();
        if (tid < s) {
            s_sum[tid] = s_sum[tid] + s_sum[tid + s];
            s_mn[tid] = fminf(s_mn[tid], s_mn[tid + s]);
            s_mx[tid] = fmaxf(s_mx[tid], s_mx[tid + s]);
        }
    }
    if (tid == 0) {
        TmFlipCell cell;
        cell.sum = s_sum[0]; cell.mn = s_mn[0]; cell.mx = s_mx[0];
        cells[(size_t)slot * g.tiles_x * g.tiles_y + tile] = cell;
    }
}

// grid (slots), block 256: the picture's mean, min and max from its tiles' cells, in a fixed order
__global__ void __launch_bounds__(TMF_THREADS) k_flip_finish(TmFlipGeom g, const TmFlipCell *__restrict__ cells, TmFlipRes *__restrict__ res)
{
    __shared__ double s_sum[TMF_THREADS];
    __shared__ float s_mn[TMF_THREADS], s_mx[TMF_THREADS];
    const unsigned tid = threadIdx.x, slot = blockIdx.x;
    const size_t tiles = (size_t)g.tiles_x * g.tiles_y;
    const TmFlipCell *cl = cells + (size_t)slot * tiles;
    double sum = 0.0;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (size_t i = tid; i < tiles; i += TMF_THREADS) {
        const TmFlipCell v = cl[i];
        sum += v.sum;
        mn = fminf(mn, v.mn);
        mx = fmaxf(mx, v.mx);
    }
    s_sum[tid] = sum; s_mn[tid] = mn; s_mx[tid] = mx;
    for (unsigned s = TMF_THREADS / 2; s > 0; s >>= 1) {
        TM_LDS_BARRIER();
        if (tid < s) {
            s_sum[tid] = s_sum[tid] + s_sum[tid + s];
            s_mn[tid] = fminf(s_mn[tid], s_mn[tid + s]);
            s_mx[tid] = fmaxf(s_mx[tid], s_mx[tid + s]);
        }
    }
    if (tid == 0) {
        TmFlipRes r;
        r.mean = s_sum[0] / g.n; r.mn = (double)s_mn[0]; r.mx = (double)s_mx[0];
        res[slot] = r;
    }
}
