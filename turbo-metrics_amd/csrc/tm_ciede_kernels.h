// tm_ciede_kernels.h -- gfx950 kernels of CIEDE2000 of 4:2:0 pairs (libturbometrics_ciede.so, include/turbo_metrics_ciede.h).
//
// The definition is DESIGN.md section 17; its float64 restatement is tests/ciede_ref.py.  Per luma position of a pair: limited-range
// Y'CbCr -> R'G'B' -> linear -> XYZ -> Lab on both sides (tmc::lab_of: ONE function, so that equal samples give equal bits), then the
// dE00 of Sharma, Wu and Dalal (tmc::de00).  The chroma of (x, y) is the chroma sample (x >> 1, y >> 1).
//
//   k_ciede<LAYOUT, FMT>   grid (tiles, slots)   block 256   one workgroup per tile of TMC_TW x TMC_TH = 128 x 32 luma positions of one
//                   slot's pair.  Lane (lx, ly) = (tid % 16, tid / 16) owns a horizontal run of TMC_CELLS = 4 chroma cells: luma columns
//                   8 lx .. 8 lx + 7 of rows 2 ly, 2 ly + 1 and the four chroma samples above them.  Where the run lies inside the
//                   picture and the planes are 16-byte aligned, that is two 4-sample loads per luma row and one (planar) or two
//                   (interleaved: Cb and Cr together) per chroma row and side (tmx::load4_raw: 4, 8 or 16 bytes each); neighbouring
//                   lanes read neighbouring bytes.  A run cut by the right edge, and every run of an unaligned picture, is read sample
//                   by sample, only the samples that exist; a bottom row that does not exist is never addressed.
//                   The kernel is bound by VALU work: per position six powf, six cbrtf, two atan2f, an expf, six sinf / cosf and a
//                   dozen divisions and square roots.  The pixel loop is kept rolled (one copy of the code in the instruction cache);
//                   the lane's samples stay in registers and are picked with selects.  The chroma terms of the matrix are computed
//                   once per cell and side.
//                   Sums in a fixed order: f32 over the lane's up to 16 positions (cell, row, column), f64 over the workgroup in a
//                   two-level LDS tree (16 x 16), the maximum beside it; lane 0 writes the tile's OWN cell with plain stores.
//   k_ciede_finish  grid (slots)   block 256   lane i adds cells i, i + 256, ... in order, then the same tree.
//
// Under the Makefile's -ffp-contract=off nothing is fused.  The emulation (tests/ciede_emul) runs this same source; the host's libm
// stands in for the device's powf / cbrtf / atan2f / expf / sinf / cosf there, which are not bit-identical.
//
// No atomics; every cell and every map value is written by every compute, so nothing is zeroed and nothing is kept between computes.
#pragma once
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::sample1 / load4_raw / unpack4

#define TMC_THREADS 256
#define TMC_LX 16                       /* lanes per tile row */
#define TMC_LY 16                       /* lane rows per tile */
#define TMC_CELLS 4                     /* 2x2 chroma cells of a lane's run */
#define TMC_TW (2 * TMC_CELLS * TMC_LX) /* luma positions */
#define TMC_TH (2 * TMC_LY)
#define TMC_MAX_DIM 32768u              /* largest w, h: keeps every byte offset inside a row in an int */

// layouts of include/turbo_metrics_ciede.h (the YUV library's numbering)
enum { TMC_NV12 = 0, TMC_P016 = 1, TMC_I420 = 2, TMC_I420P10 = 3 };

// the matrices of include/turbo_metrics_ciede.h: R = y + c0 v, G = y - c1 u - c2 v, B = y + c3 u
#define TMC_MATRICES 3
#define TMC_MATRIX_VALUES                                   \
    {{1.5748, 0.187324, 0.468124, 1.8556},  /* BT.709 */    \
     {1.402, 0.344136, 0.714136, 1.772},    /* BT.601 */    \
     {1.28033, 0.21482, 0.38059, 2.12798}}  /* libvmaf's, as recalled */

// one picture of a slot
struct TmCiedeDesc {
    const void *p0, *p1, *p2;          // Y, Cb (or CbCr), Cr (or null)
    unsigned long long pitch, pitch2;  // bytes per luma / chroma row
    int vec;                           // bases and pitches 16-byte aligned: the wide loads are allowed
    int pad_;
};

// what a tile leaves and what a slot ends with: the f64 sum and the maximum of its positions' dE00
struct TmCiedeCell {
    double sum;
    float max;
    float pad_;
};

struct TmCiedeGeom {
    unsigned w, h;
    int bits, layout;
    int fmt;             // TMX_F_* of the samples
    int shift;           // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;       // TMX_F_U16_LOW: sample = v & mask
    unsigned cw, ch;     // chroma samples
    unsigned tx, ty;     // tiles
    unsigned cells;      // tx * ty: workgroups and cells per slot
    int yoff, coff;      // 16 s, 128 s with s = 2^(D - 8)
    float ydiv, cdiv;    // 219 s, 224 s
    float c[4];          // the matrix
    float kl, kc, kh;
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 2 or above TMC_MAX_DIM, D outside 8 .. 16 or not one the
// layout carries.  The matrix and the factors: tmc_set_params.
static inline int tmc_make_geom(TmCiedeGeom *g, unsigned w, unsigned h, int layout, unsigned bits)
{
    memset(g, 0, sizeof *g);
    if (w < 2 || h < 2 || w > TMC_MAX_DIM || h > TMC_MAX_DIM || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMC_NV12: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMC_P016: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMC_I420: g->fmt = bits == 8 ? TMX_F_U8 : TMX_F_U16_LOW; break;
    case TMC_I420P10: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->w = w; g->h = h; g->bits = (int)bits; g->layout = layout;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->cw = (w + 1) / 2; g->ch = (h + 1) / 2;
    g->tx = (w + TMC_TW - 1) / TMC_TW; g->ty = (h + TMC_TH - 1) / TMC_TH;
    g->cells = g->tx * g->ty;
    const int s = 1 << (bits - 8);
    g->yoff = 16 * s; g->coff = 128 * s;
    g->ydiv = (float)(219 * s); g->cdiv = (float)(224 * s);
    return 0;
}

// 0, or -1: an unknown matrix, a factor that is not a finite number above 0
static inline int tmc_set_params(TmCiedeGeom *g, int matrix, double kl, double kc, double kh)
{
    static const double m[TMC_MATRICES][4] = TMC_MATRIX_VALUES;
    if (matrix < 0 || matrix >= TMC_MATRICES) return -1;
    if (!(kl > 0 && kc > 0 && kh > 0) || !(kl < 1e30 && kc < 1e30 && kh < 1e30)) return -1;
    for (int k = 0; k < 4; ++k) g->c[k] = (float)m[matrix][k];
    g->kl = (float)kl; g->kc = (float)kc; g->kh = (float)kh;
    return 0;
}

namespace tmc {

struct Lab {
    float L, a, b;
};

#define TMC_DEG2RAD 0.017453292519943295f
#define TMC_RAD2DEG 57.29577951308232f
#define TMC_POW25_7 6103515625.0f

// the sRGB curve's inverse; a negative value takes the linear branch
__device__ __forceinline__ float srgb_linear(float c)
{
    return c <= 0.04045f ? c / 12.92f : powf((c + 0.055f) / 1.055f, 2.4f);
}

__device__ __forceinline__ float lab_f(float t)
{
    return t > (216.0f / 24389.0f) ? cbrtf(t) : ((24389.0f / 27.0f) * t + 16.0f) / 116.0f;
}

// normalised luma and the chroma terms of the matrix (rv = c0 vn, gu = c1 un, gv = c2 vn, bu = c3 un) -> Lab.  Both sides of a pair
// go through this one function.
__device__ __forceinline__ Lab lab_of(float yn, float rv, float gu, float gv, float bu)
{
    const float R = srgb_linear(yn + rv), G = srgb_linear((yn - gu) - gv), B = srgb_linear(yn + bu);
    const float X = (0.4124564f * R + 0.3575761f * G) + 0.1804375f * B;
    const float Y = (0.2126729f * R + 0.7151522f * G) + 0.0721750f * B;
    const float Z = (0.0193339f * R + 0.1191920f * G) + 0.9503041f * B;
    const float fx = lab_f(X / 0.95047f), fy = lab_f(Y), fz = lab_f(Z / 1.08883f);
    Lab o;
    o.L = 116.0f * fy - 16.0f;
    o.a = 500.0f * (fx - fy);
    o.b = 200.0f * (fy - fz);
    return o;
}

// atan2(b, a) in degrees in [0, 360]; 0 for a = b = 0
__device__ __forceinline__ float hue_deg(float b, float a)
{
    if (a == 0.0f && b == 0.0f) return 0.0f;
    const float h = atan2f(b, a) * TMC_RAD2DEG;
    return h < 0.0f ? h + 360.0f : h;
}

__device__ __forceinline__ float pow7(float c)
{
    const float c2 = c * c, c4 = c2 * c2;
    return (c4 * c2) * c;
}

// dE00 of Sharma, Wu and Dalal (2005) with the parametric factors kl, kc, kh; exactly 0 for equal triples
__device__ __forceinline__ float de00(const Lab &p, const Lab &q, float kl, float kc, float kh)
{
    const float c1 = sqrtf(p.a * p.a + p.b * p.b), c2 = sqrtf(q.a * q.a + q.b * q.b);
    const float cb7 = pow7((c1 + c2) * 0.5f);
    const float G = 0.5f * (1.0f - sqrtf(cb7 / (cb7 + TMC_POW25_7)));
    const float a1 = (1.0f + G) * p.a, a2 = (1.0f + G) * q.a;
    const float C1 = sqrtf(a1 * a1 + p.b * p.b), C2 = sqrtf(a2 * a2 + q.b * q.b);
    const float h1 = hue_deg(p.b, a1), h2 = hue_deg(q.b, a2);
    const float dL = q.L - p.L, dC = C2 - C1;
    const float prod = C1 * C2;
    float dh = 0.0f;
    if (prod != 0.0f) {
        dh = h2 - h1;
        if (dh > 180.0f) dh -= 360.0f;
        else if (dh < -180.0f) dh += 360.0f;
    }
    const float dH = 2.0f * sqrtf(prod) * sinf((dh * 0.5f) * TMC_DEG2RAD);
    const float Lb = (p.L + q.L) * 0.5f, Cb = (C1 + C2) * 0.5f;
    const float hs = h1 + h2;
    float hb = hs;
    if (prod != 0.0f) {
        if (fabsf(h1 - h2) <= 180.0f) hb = hs * 0.5f;
        else if (hs < 360.0f) hb = hs * 0.5f + 180.0f;
        else hb = hs * 0.5f - 180.0f;
    }
    const float T = (((1.0f - 0.17f * cosf((hb - 30.0f) * TMC_DEG2RAD)) + 0.24f * cosf((2.0f * hb) * TMC_DEG2RAD)) +
                     0.32f * cosf((3.0f * hb + 6.0f) * TMC_DEG2RAD)) - 0.20f * cosf((4.0f * hb - 63.0f) * TMC_DEG2RAD);
    const float e = (hb - 275.0f) / 25.0f;
    const float dth = 30.0f * expf(-(e * e));
    const float Cb7 = pow7(Cb);
    const float RC = 2.0f * sqrtf(Cb7 / (Cb7 + TMC_POW25_7));
    const float l50 = Lb - 50.0f, l2 = l50 * l50;
    const float SL = 1.0f + (0.015f * l2) / sqrtf(20.0f + l2);
    const float SC = 1.0f + 0.045f * Cb, SH = 1.0f + (0.015f * Cb) * T;
    const float RT = -sinf((2.0f * dth) * TMC_DEG2RAD) * RC;
    const float x = dL / (kl * SL), y = dC / (kc * SC), z = dH / (kh * SH);
    const float r = ((x * x + y * y) + z * z) + (RT * y) * z;
    return sqrtf(fmaxf(r, 0.0f));
}

// v[i] without a dynamically indexed (scratch) array
template <int N>
__device__ __forceinline__ unsigned pick(const unsigned (&v)[N], unsigned i)
{
    unsigned r = v[0];
#pragma unroll
    for (int k = 1; k < N; ++k) r = i == (unsigned)k ? v[k] : r;
    return r;
}

// The lane's run of one picture: luma columns x0 .. x0 + 7 (x0 a multiple of 8) of rows y0 and, where nrows == 2, y0 + 1, and the chroma
// samples x0 / 2 .. x0 / 2 + 3 of chroma row y0 / 2.  wide: the run lies inside the picture and the planes are aligned.  What does not
// exist reads as 0 and is never addressed.
template <int LAYOUT, int FMT>
__device__ __forceinline__ void load_run(const TmCiedeGeom &g, const TmCiedeDesc &d, bool wide, unsigned x0, unsigned y0, int nrows,
                                         unsigned (&Y)[2][8], unsigned (&U)[TMC_CELLS], unsigned (&V)[TMC_CELLS])
{
    constexpr bool BI = LAYOUT == TMC_NV12 || LAYOUT == TMC_P016;
    const unsigned cx0 = x0 >> 1;
    const char *ry = (const char *)d.p0 + (size_t)y0 * d.pitch;
    const char *ru = (const char *)d.p1 + (size_t)(y0 >> 1) * d.pitch2;
    const char *rv = BI ? ru : (const char *)d.p2 + (size_t)(y0 >> 1) * d.pitch2;
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 8; ++k) Y[r][k] = 0u;
#pragma unroll
    for (int k = 0; k < TMC_CELLS; ++k) U[k] = V[k] = 0u;
    if (wide) {
        tmx::Raw4 qy[2][2], qc[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            qy[r][0] = qy[r][1] = tmx::Raw4{{0, 0, 0, 0}};
            if (r < nrows) {
                qy[r][0] = tmx::load4_raw(ry + (size_t)r * d.pitch, FMT, (int)x0);
                qy[r][1] = tmx::load4_raw(ry + (size_t)r * d.pitch, FMT, (int)x0 + 4);
            }
        }
        if (BI) { // Cb at the even, Cr at the odd elements
            qc[0] = tmx::load4_raw(ru, FMT, (int)x0);
            qc[1] = tmx::load4_raw(ru, FMT, (int)x0 + 4);
        } else {
            qc[0] = tmx::load4_raw(ru, FMT, (int)cx0);
            qc[1] = tmx::load4_raw(rv, FMT, (int)cx0);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= nrows) continue;
            unsigned lo[4], hi[4];
            tmx::unpack4(qy[r][0], FMT, (int)x0, g.shift, g.mask, lo);
            tmx::unpack4(qy[r][1], FMT, (int)x0 + 4, g.shift, g.mask, hi);
#pragma unroll
            for (int k = 0; k < 4; ++k) { Y[r][k] = lo[k]; Y[r][4 + k] = hi[k]; }
        }
        unsigned e0[4], e1[4];
        if (BI) {
            tmx::unpack4(qc[0], FMT, (int)x0, g.shift, g.mask, e0);
            tmx::unpack4(qc[1], FMT, (int)x0 + 4, g.shift, g.mask, e1);
            U[0] = e0[0]; V[0] = e0[1]; U[1] = e0[2]; V[1] = e0[3];
            U[2] = e1[0]; V[2] = e1[1]; U[3] = e1[2]; V[3] = e1[3];
        } else {
            tmx::unpack4(qc[0], FMT, (int)cx0, g.shift, g.mask, e0);
            tmx::unpack4(qc[1], FMT, (int)cx0, g.shift, g.mask, e1);
#pragma unroll
            for (int k = 0; k < 4; ++k) { U[k] = e0[k]; V[k] = e1[k]; }
        }
    } else { // sample by sample, the samples that exist
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r >= nrows) continue;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (x0 + k < g.w) Y[r][k] = tmx::sample1(ry + (size_t)r * d.pitch, FMT, (int)(x0 + k), g.shift, g.mask);
        }
#pragma unroll
        for (int k = 0; k < TMC_CELLS; ++k)
            if (cx0 + k < g.cw) {
                U[k] = tmx::sample1(ru, FMT, (int)(BI ? 2 * (cx0 + k) : cx0 + k), g.shift, g.mask);
                V[k] = tmx::sample1(rv, FMT, (int)(BI ? 2 * (cx0 + k) + 1 : cx0 + k), g.shift, g.mask);
            }
    }
}

// the two-level tree: 256 values -> 16 sums of 16 neighbours -> their sum, each level in index order; the maximum beside it.  Lane 0
// holds the result.  All lanes of the workgroup call it.
struct Tree {
    double sum[TMC_THREADS];
    float max[TMC_THREADS];
};
__device__ __forceinline__ void tree_sum(Tree &t, unsigned tid, double &sum, float &mx)
{
    t.sum[tid] = sum; t.max[tid] = mx;
    TM_LDS_BARRIER();
    if (tid < 16) {
        double a = 0.0;
        float m = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) { a += t.sum[tid * 16 + k]; m = fmaxf(m, t.max[tid * 16 + k]); }
        sum = a; mx = m;
    }
    TM_LDS_BARRIER();
    if (tid < 16) { t.sum[tid] = sum; t.max[tid] = mx; }
    TM_LDS_BARRIER();
    if (tid == 0) {
        double a = 0.0;
        float m = 0.0f;
#pragma unroll
        for (int k = 0; k < 16; ++k) { a += t.sum[k]; m = fmaxf(m, t.max[k]); }
        sum = a; mx = m;
    }
}

} // namespace tmc

// desc: [slot][side]; maps: null, or [slot][g.h][g.w]; cells: [slot][g.cells].  FMT: the TMX_F_* the layout's samples have at this depth
// (I420: bytes at D = 8, else 16-bit words): five instantiations, the host picks one.  The matrix and the factors are in g.
template <int LAYOUT, int FMT>
__global__ void __launch_bounds__(TMC_THREADS) k_ciede(TmCiedeGeom g, const TmCiedeDesc *__restrict__ desc, float *__restrict__ maps, TmCiedeCell *__restrict__ cells)
{
    using namespace tmc;
    __shared__ Tree tree;
    const unsigned tid = threadIdx.x, slot = blockIdx.y, t = blockIdx.x;
    const unsigned x0 = ((t % g.tx) * TMC_LX + tid % TMC_LX) * (2 * TMC_CELLS), y0 = ((t / g.tx) * TMC_LY + tid / TMC_LX) * 2;
    float sum = 0.0f, mx = 0.0f;
    if (x0 < g.w && y0 < g.h) {
        const TmCiedeDesc da = desc[2 * slot], db = desc[2 * slot + 1];
        const int nrows = y0 + 1 < g.h ? 2 : 1;
        const bool wide = da.vec && db.vec && x0 + 2 * TMC_CELLS <= g.w;
        unsigned Ya[2][8], Ua[TMC_CELLS], Va[TMC_CELLS], Yb[2][8], Ub[TMC_CELLS], Vb[TMC_CELLS];
        load_run<LAYOUT, FMT>(g, da, wide, x0, y0, nrows, Ya, Ua, Va);
        load_run<LAYOUT, FMT>(g, db, wide, x0, y0, nrows, Yb, Ub, Vb);
        float *m = maps ? maps + (size_t)slot * g.w * g.h : nullptr;
#pragma unroll 1
        for (unsigned c = 0; c < TMC_CELLS; ++c) {
            if (x0 + 2 * c >= g.w) break;
            // the chroma terms of the cell, once per side
            const float ua = (float)((int)pick(Ua, c) - g.coff) / g.cdiv, va = (float)((int)pick(Va, c) - g.coff) / g.cdiv;
            const float ub = (float)((int)pick(Ub, c) - g.coff) / g.cdiv, vb = (float)((int)pick(Vb, c) - g.coff) / g.cdiv;
            const float rva = g.c[0] * va, gua = g.c[1] * ua, gva = g.c[2] * va, bua = g.c[3] * ua;
            const float rvb = g.c[0] * vb, gub = g.c[1] * ub, gvb = g.c[2] * vb, bub = g.c[3] * ub;
#pragma unroll 1
            for (unsigned i = 0; i < 4; ++i) { // row i >> 1, column i & 1 of the cell
                const unsigned r = i >> 1, k = 2 * c + (i & 1);
                if ((int)r >= nrows || x0 + k >= g.w) continue;
                const unsigned sa = r ? pick(Ya[1], k) : pick(Ya[0], k), sb = r ? pick(Yb[1], k) : pick(Yb[0], k);
                const float ya = (float)((int)sa - g.yoff) / g.ydiv, yb = (float)((int)sb - g.yoff) / g.ydiv;
                const Lab p = lab_of(ya, rva, gua, gva, bua), q = lab_of(yb, rvb, gub, gvb, bub);
                const float de = de00(p, q, g.kl, g.kc, g.kh);
                sum += de;
                mx = fmaxf(mx, de);
                if (m) m[(size_t)(y0 + r) * g.w + (x0 + k)] = de;
            }
        }
    }
    double s64 = (double)sum;
    tree_sum(tree, tid, s64, mx);
    if (tid == 0) {
        TmCiedeCell cell;
        cell.sum = s64; cell.max = mx; cell.pad_ = 0.0f;
        cells[(size_t)slot * g.cells + t] = cell;
    }
}

// the launch of the instantiation for g.layout / g.fmt: the one place that maps a geometry to a kernel (library and emulation)
#define TMC_DISPATCH(g, LAUNCH)                                                   \
    do {                                                                          \
        switch ((g).layout) {                                                     \
        case TMC_NV12: LAUNCH(TMC_NV12, TMX_F_U8); break;                         \
        case TMC_P016: LAUNCH(TMC_P016, TMX_F_U16_MSB); break;                    \
        case TMC_I420:                                                            \
            if ((g).fmt == TMX_F_U8) LAUNCH(TMC_I420, TMX_F_U8);                  \
            else LAUNCH(TMC_I420, TMX_F_U16_LOW);                                 \
            break;                                                                \
        default: LAUNCH(TMC_I420P10, TMX_F_P10); break;                           \
        }                                                                         \
    } while (0)

// grid (slots), block 256: the sum and the maximum of the slot's cells in a fixed order
__global__ void __launch_bounds__(TMC_THREADS) k_ciede_finish(TmCiedeGeom g, const TmCiedeCell *__restrict__ cells, TmCiedeCell *__restrict__ res)
{
    __shared__ tmc::Tree tree;
    const unsigned tid = threadIdx.x, slot = blockIdx.x;
    const TmCiedeCell *cl = cells + (size_t)slot * g.cells;
    double sum = 0.0;
    float mx = 0.0f;
    for (unsigned i = tid; i < g.cells; i += TMC_THREADS) { sum += cl[i].sum; mx = fmaxf(mx, cl[i].max); }
    tmc::tree_sum(tree, tid, sum, mx);
    if (tid == 0) {
        TmCiedeCell out;
        out.sum = sum; out.max = mx; out.pad_ = 0.0f;
        res[slot] = out;
    }
}
