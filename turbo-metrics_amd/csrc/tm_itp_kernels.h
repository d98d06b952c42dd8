// tm_itp_kernels.h -- gfx950 kernel of the BT.2124 colour difference dE ITP of 4:2:0 HDR pairs (libturbometrics_itp.so,
// include/turbo_metrics_itp.h).
//
// The definition is DESIGN.md section 22; its float64 restatement is tests/itp_ref.py.  Per luma position of a pair: limited-range
// Y'CbCr -> BT.2020 R'G'B' clamped to [0, 1] -> display light (PQ, or HLG at 1000 cd/m2) -> LMS -> PQ signal -> ICtCp on both sides
// (tmi::ictcp_of: ONE function, so that equal samples give equal bits), then 720 sqrt(dI^2 + (dCt / 2)^2 + dCp^2).  The chroma of (x, y)
// is the chroma sample (x >> 1, y >> 1).
//
// The geometry, the load paths, the sums and the finish kernel are section 17's and are taken from tm_ciede_kernels.h as they are:
// TmCiedeGeom / TmCiedeDesc / TmCiedeCell, tmc::load_run, tmc::tree_sum, k_ciede_finish.  What is new is the colour math:
//
//   k_itp<LAYOUT, FMT>   grid (tiles, slots)   block 256   one workgroup per tile of 128 x 32 luma positions of one slot's pair; lane
//                   (tid % 16, tid / 16) owns four 2x2 chroma cells: wide loads where the run is inside the picture and the planes are
//                   aligned, sample by sample otherwise, nothing beyond an odd edge addressed.  The chroma terms of the matrix once
//                   per cell and side; the pixel loop rolled: it takes the run's FIRST cell and moves the others down by register
//                   copies with constant indices (a select chain indexed by the loop counters becomes a scratch array).  f32 lane sums in a fixed order, the f64 LDS tree and the maximum, the
//                   tile's OWN cell with plain stores.  The transfer is a kernel ARGUMENT (g.transfer, uniform over the grid).
//
// The math (namespace tmi).  A position costs 24 pow(); none is a libm call.  log2, exp2 and pow are written from fma, +, -, x, the
// correctly rounded division and integer bit operations IN F64: the PQ inverse raises a base in [0.836, 1] to m2 = 78.84, so the
// logarithm has to be good to 2^-32 to keep the result's f32 rounding the only error, and the base itself must not be rounded to f32
// either.  An f32 hi + lo pair reaches that with about four times the operations of the f64 form, on a device whose f64 FMA runs at
// half the f32 rate; so the stages keep their values in f64 from an f32 input to an f32 output (pq_eotf, hlg_display, pq_inv) and
// everything between the stages -- the normalisation, the matrices, the difference -- is f32.  Every operation is correctly rounded on
// the device and on a host, under the Makefile's -ffp-contract=off nothing else is fused: the emulation (tests/itp_emul) runs this
// same source and gives the same bits.
//
// No atomics; every cell and every map value is written by every compute.
#pragma once
#include "tm_ciede_kernels.h"

// layouts of include/turbo_metrics_itp.h (the YUV library's numbering): TMC_NV12 .. TMC_I420P10
enum { TMI_PQ = 0, TMI_HLG = 1, TMI_TRANSFERS = 2 };

// BT.2020 non-constant luminance: R = y + c0 v, G = y - c1 u - c2 v, B = y + c3 u
#define TMI_MATRIX_VALUES {1.4746, 0.16455, 0.57135, 1.8814}

struct TmItpGeom {
    TmCiedeGeom b;   // the picture, the tiles, the normalisation, the matrix in b.c (kl, kc, kh unused)
    int transfer;    // TMI_PQ / TMI_HLG
    int pad_;
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED (tmc_make_geom's rules); the transfer is checked by the caller
static inline int tmi_make_geom(TmItpGeom *g, unsigned w, unsigned h, int layout, unsigned bits, int transfer)
{
    static const double m[4] = TMI_MATRIX_VALUES;
    memset(g, 0, sizeof *g);
    if (tmc_make_geom(&g->b, w, h, layout, bits)) return -1;
    for (int k = 0; k < 4; ++k) g->b.c[k] = (float)m[k];
    g->transfer = transfer;
    return 0;
}

namespace tmi {

#define TMI_M1 (2610.0 / 16384.0)
#define TMI_M2 (2523.0 / 32.0)
#define TMI_INV_M1 (16384.0 / 2610.0)
#define TMI_INV_M2 (32.0 / 2523.0)
#define TMI_C1 (3424.0 / 4096.0)
#define TMI_C2 (2413.0 / 128.0)
#define TMI_C3 (2392.0 / 128.0)
#define TMI_LOG2_10000 13.287712379549449
#define TMI_HLG_A 0.17883277
#define TMI_HLG_B 0.28466892          /* 1 - 4 a */
#define TMI_HLG_C 0.559910729529562   /* 0.5 - a ln(4 a) */
#define TMI_LOG2E 1.4426950408889634
#define TMI_LN2 0.6931471805599453
// below this a display light counts as 0: no f32 subnormal leaves a stage
#define TMI_TINY 1e-30

// log2(x) for a normal x > 0: x = 2^k m with m in (sqrt(1/2), sqrt(2)], s = (m - 1) / (m + 1) (|s| <= 0.1716), ln m = 2 s (1 + z / 3 +
// ... + z^8 / 17) with z = s^2 (the next term is below 1e-15 of the sum).
__device__ __forceinline__ double log2_d(double x)
{
    const long long bits = __double_as_longlong(x);
    int k = (int)(bits >> 52) - 1023;
    double m = __longlong_as_double((bits & 0x000FFFFFFFFFFFFFll) | 0x3FF0000000000000ll);
    if (m > 1.4142135623730951) { m *= 0.5; ++k; }
    const double s = (m - 1.0) / (m + 1.0), z = s * s;
    double p = 1.0 / 17.0;
    p = fma(p, z, 1.0 / 15.0);
    p = fma(p, z, 1.0 / 13.0);
    p = fma(p, z, 1.0 / 11.0);
    p = fma(p, z, 1.0 / 9.0);
    p = fma(p, z, 1.0 / 7.0);
    p = fma(p, z, 1.0 / 5.0);
    p = fma(p, z, 1.0 / 3.0);
    p = fma(p, z, 1.0);
    return fma(s * (2.0 * TMI_LOG2E), p, (double)k);
}

// 2^t for t in [-1020, 1020]; 0 below: n = round(t), r = t - n exactly, the degree-12 Taylor polynomial of exp(r ln 2) (|r ln 2| <=
// 0.3466: remainder below 2e-16) and 2^n by exponent arithmetic
__device__ __forceinline__ double exp2_d(double t)
{
    if (t < -1020.0) return 0.0;
    const int n = (int)(t + (t < 0.0 ? -0.5 : 0.5));
    const double u = (t - (double)n) * TMI_LN2;
    double p = 1.0 / 479001600.0;
    p = fma(p, u, 1.0 / 39916800.0);
    p = fma(p, u, 1.0 / 3628800.0);
    p = fma(p, u, 1.0 / 362880.0);
    p = fma(p, u, 1.0 / 40320.0);
    p = fma(p, u, 1.0 / 5040.0);
    p = fma(p, u, 1.0 / 720.0);
    p = fma(p, u, 1.0 / 120.0);
    p = fma(p, u, 1.0 / 24.0);
    p = fma(p, u, 1.0 / 6.0);
    p = fma(p, u, 0.5);
    p = fma(p, u, 1.0);
    p = fma(p, u, 1.0);
    return p * __longlong_as_double((long long)(n + 1023) << 52);
}

// x^e for x >= 0 (normal or 0) and e > 0; pow(0, e) = 0 exactly, pow(1, e) = 1 exactly
__device__ __forceinline__ double pow_d(double x, double e)
{
    return x > 0.0 ? exp2_d(e * log2_d(x)) : 0.0;
}

// the f32 forms the tests measure: arguments in [0, 1] (f32 subnormals count as 0)
__device__ __forceinline__ float log2_f(float x) { return (float)log2_d((double)x); }
__device__ __forceinline__ float exp2_f(float t) { return (float)exp2_d((double)t); }
__device__ __forceinline__ float pow_f(float x, double e) { return x >= 1.17549435e-38f ? (float)pow_d((double)x, e) : 0.0f; }

__device__ __forceinline__ float out_light(double f) { return f < TMI_TINY ? 0.0f : (float)f; }

// BT.2100 PQ EOTF: signal in [0, 1] -> cd/m2
__device__ __forceinline__ float pq_eotf(float e)
{
    if (!(e >= 1.17549435e-38f)) return 0.0f;
    const double p = exp2_d(TMI_INV_M2 * log2_d((double)e));
    const double num = p - TMI_C1;
    if (!(num > 0.0)) return 0.0f;
    const double q = num / (TMI_C2 - TMI_C3 * p);
    return out_light(exp2_d(fma(TMI_INV_M1, log2_d(q), TMI_LOG2_10000)));
}

// BT.2100 PQ inverse EOTF: cd/m2 (>= 0) -> signal.  The base stays in f64: m2 multiplies its relative error by 79.
__device__ __forceinline__ float pq_inv(float f)
{
    const double y = f >= 1.17549435e-38f ? exp2_d(TMI_M1 * (log2_d((double)f) - TMI_LOG2_10000)) : 0.0;
    const double base = fma(TMI_C2, y, TMI_C1) / fma(TMI_C3, y, 1.0);
    return (float)exp2_d(TMI_M2 * log2_d(base));
}

// BT.2100 HLG: the inverse OETF per channel, then the OOTF of a 1000 cd/m2 display (system gamma 1.2): F = 1000 Ys^0.2 E
__device__ __forceinline__ double hlg_scene(float e)
{
    const double x = (double)e;
    if (e <= 0.5f) return (x * x) / 3.0;
    return (exp2_d((x - TMI_HLG_C) * (TMI_LOG2E / TMI_HLG_A)) + TMI_HLG_B) / 12.0;
}
__device__ __forceinline__ void hlg_display(float r, float g, float b, float &fr, float &fg, float &fb)
{
    const double R = hlg_scene(r), G = hlg_scene(g), B = hlg_scene(b);
    const double ys = fma(0.0593, B, fma(0.6780, G, 0.2627 * R));
    const double k = 1000.0 * pow_d(ys, 0.2); // 0 where Ys = 0
    fr = out_light(k * R); fg = out_light(k * G); fb = out_light(k * B);
}

struct Itp {
    float i, t, p;
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// normalised luma and the chroma terms of the matrix (rv = c0 vn, gu = c1 un, gv = c2 vn, bu = c3 un) -> ICtCp.  Both sides of a pair
// go through this one function.
__device__ __forceinline__ Itp ictcp_of(float yn, float rv, float gu, float gv, float bu, int transfer)
{
    const float r = clamp01(yn + rv), g = clamp01((yn - gu) - gv), b = clamp01(yn + bu);
    float R, G, B;
    if (transfer == TMI_HLG) hlg_display(r, g, b, R, G, B);
    else { R = pq_eotf(r); G = pq_eotf(g); B = pq_eotf(b); }
    const float L = ((1688.0f / 4096.0f) * R + (2146.0f / 4096.0f) * G) + (262.0f / 4096.0f) * B;
    const float M = ((683.0f / 4096.0f) * R + (2951.0f / 4096.0f) * G) + (462.0f / 4096.0f) * B;
    const float S = ((99.0f / 4096.0f) * R + (309.0f / 4096.0f) * G) + (3688.0f / 4096.0f) * B;
    const float l = pq_inv(L), m = pq_inv(M), s = pq_inv(S);
    Itp o;
    o.i = (l + m) * 0.5f;
    o.t = ((6610.0f / 4096.0f) * l - (13613.0f / 4096.0f) * m) + (7003.0f / 4096.0f) * s;
    o.p = ((17933.0f / 4096.0f) * l - (17390.0f / 4096.0f) * m) - (543.0f / 4096.0f) * s;
    return o;
}

// dE ITP; exactly 0 for equal triples, the same bits with the sides exchanged
__device__ __forceinline__ float de_itp(const Itp &a, const Itp &b)
{
    const float di = b.i - a.i, dt = (b.t - a.t) * 0.5f, dp = b.p - a.p;
    return 720.0f * sqrtf((di * di + dt * dt) + dp * dp);
}

} // namespace tmi

// desc: [slot][side]; maps: null, or [slot][h][w]; cells: [slot][g.b.cells].  FMT as in k_ciede: five instantiations (TMC_DISPATCH).
template <int LAYOUT, int FMT>
__global__ void __launch_bounds__(TMC_THREADS) k_itp(TmItpGeom gi, const TmCiedeDesc *__restrict__ desc, float *__restrict__ maps, TmCiedeCell *__restrict__ cells)
{
    using namespace tmi;
    __shared__ tmc::Tree tree;
    const TmCiedeGeom &g = gi.b;
    const unsigned tid = threadIdx.x, slot = blockIdx.y, t = blockIdx.x;
    const unsigned x0 = ((t % g.tx) * TMC_LX + tid % TMC_LX) * (2 * TMC_CELLS), y0 = ((t / g.tx) * TMC_LY + tid / TMC_LX) * 2;
    float sum = 0.0f, mx = 0.0f;
    if (x0 < g.w && y0 < g.h) {
        const TmCiedeDesc da = desc[2 * slot], db = desc[2 * slot + 1];
        const int nrows = y0 + 1 < g.h ? 2 : 1;
        const bool wide = da.vec && db.vec && x0 + 2 * TMC_CELLS <= g.w;
        unsigned Ya[2][8], Ua[TMC_CELLS], Va[TMC_CELLS], Yb[2][8], Ub[TMC_CELLS], Vb[TMC_CELLS];
        tmc::load_run<LAYOUT, FMT>(g, da, wide, x0, y0, nrows, Ya, Ua, Va);
        tmc::load_run<LAYOUT, FMT>(g, db, wide, x0, y0, nrows, Yb, Ub, Vb);
        float *m = maps ? maps + (size_t)slot * g.w * g.h : nullptr;
#pragma unroll 1
        for (unsigned c = 0; c < TMC_CELLS; ++c) { // the run's first cell; the others move down behind it
            if (x0 + 2 * c >= g.w) break;
            // the chroma terms of the cell, once per side
            const float ua = (float)((int)Ua[0] - g.coff) / g.cdiv, va = (float)((int)Va[0] - g.coff) / g.cdiv;
            const float ub = (float)((int)Ub[0] - g.coff) / g.cdiv, vb = (float)((int)Vb[0] - g.coff) / g.cdiv;
            const float rva = g.c[0] * va, gua = g.c[1] * ua, gva = g.c[2] * va, bua = g.c[3] * ua;
            const float rvb = g.c[0] * vb, gub = g.c[1] * ub, gvb = g.c[2] * vb, bub = g.c[3] * ub;
            unsigned a0 = Ya[0][0], a1 = Ya[0][1], a2 = Ya[1][0], a3 = Ya[1][1];
            unsigned b0 = Yb[0][0], b1 = Yb[0][1], b2 = Yb[1][0], b3 = Yb[1][1];
#pragma unroll 1
            for (unsigned i = 0; i < 4; ++i) { // row i >> 1, column i & 1 of the cell
                const unsigned sa = a0, sb = b0;
                a0 = a1; a1 = a2; a2 = a3;
                b0 = b1; b1 = b2; b2 = b3;
                const unsigned r = i >> 1, k = 2 * c + (i & 1);
                if ((int)r >= nrows || x0 + k >= g.w) continue;
                const float ya = (float)((int)sa - g.yoff) / g.ydiv, yb = (float)((int)sb - g.yoff) / g.ydiv;
                const Itp p = ictcp_of(ya, rva, gua, gva, bua, gi.transfer), q = ictcp_of(yb, rvb, gub, gvb, bub, gi.transfer);
                const float de = de_itp(p, q);
                sum += de;
                mx = fmaxf(mx, de);
                if (m) m[(size_t)(y0 + r) * g.w + (x0 + k)] = de;
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) { Ya[0][k] = Ya[0][k + 2]; Ya[1][k] = Ya[1][k + 2]; Yb[0][k] = Yb[0][k + 2]; Yb[1][k] = Yb[1][k + 2]; }
#pragma unroll
            for (int k = 0; k < TMC_CELLS - 1; ++k) { Ua[k] = Ua[k + 1]; Va[k] = Va[k + 1]; Ub[k] = Ub[k + 1]; Vb[k] = Vb[k + 1]; }
        }
    }
    double s64 = (double)sum;
    tmc::tree_sum(tree, tid, s64, mx);
    if (tid == 0) {
        TmCiedeCell cell;
        cell.sum = s64; cell.max = mx; cell.pad_ = 0.0f;
        cells[(size_t)slot * g.cells + t] = cell;
    }
}
