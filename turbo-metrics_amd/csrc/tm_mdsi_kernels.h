// tm_mdsi_kernels.h -- gfx950 kernels of MDSI, the mean deviation similarity index of 4:2:0 pairs (libturbometrics_mdsi.so,
// include/turbo_metrics_mdsi.h).
//
// The definition is DESIGN.md section 23; its float64 restatement is tests/mdsi_ref.py.  Per pair: the f x f box sums SY, SU, SV of the
// luma samples and of the chroma sample each luma position takes, at every f-th position (windows centred as conv2 'same' centres them,
// zeros outside the picture, n_in positions inside), the planes L, H, M as one affine map of those exact integers, Prewitt on L with
// zeros beyond the decimated plane, then ONE expression per position (tmm::gcs_of) in `tmm::real`; the map holds GCS rounded to f32,
// and both pooling passes take z = GCS^(1/4) from that f32 value (tmm::z_of, f64).
//
//   k_mdsi<LAYOUT, FMT>   grid (tiles, slots)   block 256   one workgroup per tile of TMM_TW x TMM_TH decimated positions of one slot's
//                   pair.
//                     1. an item is one decimated position of the tile or of its one-position halo (TMM_LH rows of TMM_LW columns): the
//                        lane walks the rows of the position's window and, per row, the 4-sample groups that overlap it -- a 4-byte
//                        (bytes), 8-byte (16-bit) or 16-byte (packed 10-bit) load where the planes are 16-byte aligned and the whole
//                        group lies inside the row, sample by sample otherwise -- then the chroma rows under the window, every chroma
//                        sample weighted by the number of window positions that take it (1, 2 or 4).  Nothing outside the picture is
//                        addressed: those samples are the definition's zeros.  The windows of neighbouring positions are disjoint, so
//                        a sample inside the tile leaves HBM once; a group that straddles two windows is asked for by two lanes of
//                        the same workgroup and the second request is served by the cache.  L, H, M of both pictures go to LDS;
//                        positions beyond the decimated plane are 0 there.
//                     2. lane (c, q) = (tid % 32, tid / 32) owns column c, rows 2 q and 2 q + 1 of the tile: Prewitt of both pictures
//                        from nine LDS values each, gcs_of, the map value (a wave writes two runs of 32 consecutive floats), z_of.
//                     3. the lane's Re z, Im z and its count of negative positions, in row order; 16 lanes add 16 neighbouring lanes'
//                        sums in lane order, lane 0 those 16, and writes the tile's OWN cell with plain stores.
//   k_mdsi_finish   grid (slots)   block 256   lane i adds cells i, i + 256, ... in order, then the same two-level tree.  stage 0 writes
//                   sum_re, sum_im and negatives of the slot, stage 1 writes dev.
//   k_mdsi_dev      grid (chunks, slots)   block 256   the dependent second pass: mu = (sum_re, sum_im) / N of the slot, then |z - mu| of
//                   TMM_DEV_PER_LANE x 256 consecutive map values per workgroup (lane i takes values i, i + 256, ... in order), the
//                   same tree, the chunk's own cell.
//
// Under the Makefile's -ffp-contract=off nothing is fused; conversions, square roots and divisions are correctly rounded.  The order
// written here IS the definition's operation order; the emulation (tests/mdsi_emul) runs this same source.
//
// No atomics; every cell, every result field and every map value is written by every compute, so nothing is zeroed and nothing is
// kept between computes.
#pragma once
#include "tm_ciede_kernels.h" // TmCiedeGeom / TmCiedeDesc, the layouts, the matrices, TMC_DISPATCH; tm_sample_load.h

// the type of the per-position expression: decided by the measured tolerance
#ifndef TMM_REAL
#define TMM_REAL float
#endif

#define TMM_THREADS 256
#define TMM_TW 32                 /* decimated positions per tile row */
#define TMM_TH 16                 /* ... per tile column */
#define TMM_LW (TMM_TW + 2)       /* columns in LDS: x0 - 1 .. x0 + TW */
#define TMM_LH (TMM_TH + 2)       /* rows in LDS: y0 - 1 .. y0 + TH */
#define TMM_ITEMS (TMM_LW * TMM_LH)
#define TMM_ROWS_PER_LANE (TMM_TH / (TMM_THREADS / TMM_TW))
#define TMM_DEV_PER_LANE 8        /* map values per lane of k_mdsi_dev */
#define TMM_MAX_FACTOR 128u
#define TMM_MIN_POSITIONS 4ull

// the paper's constants on the 0 .. 255 scale
#define TMM_C1 140.0
#define TMM_C2 55.0
#define TMM_C3 550.0
#define TMM_ALPHA 0.6

// matrices of include/turbo_metrics_mdsi.h: tm_ciede's BT.709 and BT.601, or the one the height picks
enum { TMM_BT709 = 0, TMM_BT601 = 1, TMM_BY_HEIGHT = 2 };

// what a tile or a chunk leaves
struct TmMdsiCell {
    double a, b;              // k_mdsi: the sums of Re z and Im z; k_mdsi_dev: the sum of |z - mu|, 0
    unsigned long long n;     // k_mdsi: positions with GCS < 0
};

// what a slot ends with
struct TmMdsiRes {
    double re, im, dev;
    unsigned long long neg;
};

struct TmMdsiGeom {
    TmCiedeGeom b;            // the picture and its samples (b.tx, b.ty, b.cells and the f32 constants are not used)
    unsigned f;               // the factor
    unsigned wd, hd;          // the decimated plane: ceil(w / f), ceil(h / f)
    unsigned tx, ty;          // tiles
    unsigned cells;           // tx * ty: workgroups and cells per slot of k_mdsi
    unsigned cells2;          // chunks: workgroups and cells per slot of k_mdsi_dev
    int matrix;               // TMM_BT709 / TMM_BT601, resolved
    unsigned long long n;     // wd * hd
    double k[3][4];           // L, H, M: the coefficients of SY, SU, SV and n_in
    double ff;                // f^2
};

// max(1, round(min(w, h) / 256)), halves away from zero
static inline unsigned tmm_auto_factor(unsigned w, unsigned h)
{
    const unsigned m = w < h ? w : h;
    const unsigned f = (unsigned)((2ull * m + 256ull) / 512ull);
    return f < 1 ? 1 : f;
}

// 0; -1 for what the library refuses as TM_ERR_UNSUPPORTED (tmc_make_geom's rules, fewer than 4 decimated positions); -2 for
// TM_ERR_INVALID_ARG (an unknown matrix, a factor above 128).  factor 0: automatic.
static inline int tmm_make_geom(TmMdsiGeom *g, unsigned w, unsigned h, int layout, unsigned bits, int matrix, unsigned factor)
{
    static const double m[TMC_MATRICES][4] = TMC_MATRIX_VALUES;
    static const double plane[3][3] = {{0.2989, 0.5870, 0.1140}, {0.30, 0.04, -0.35}, {0.34, -0.60, 0.17}};
    memset(g, 0, sizeof *g);
    if (matrix < 0 || matrix > TMM_BY_HEIGHT || factor > TMM_MAX_FACTOR) return -2;
    if (tmc_make_geom(&g->b, w, h, layout, bits)) return -1;
    g->f = factor ? factor : tmm_auto_factor(w, h);
    g->wd = (w + g->f - 1) / g->f; g->hd = (h + g->f - 1) / g->f;
    g->n = (unsigned long long)g->wd * g->hd;
    if (g->n < TMM_MIN_POSITIONS) return -1;
    g->tx = (g->wd + TMM_TW - 1) / TMM_TW; g->ty = (g->hd + TMM_TH - 1) / TMM_TH;
    g->cells = g->tx * g->ty;
    g->cells2 = (unsigned)((g->n + (unsigned long long)TMM_THREADS * TMM_DEV_PER_LANE - 1) / ((unsigned long long)TMM_THREADS * TMM_DEV_PER_LANE));
    g->matrix = matrix == TMM_BY_HEIGHT ? (h >= 720 ? TMM_BT709 : TMM_BT601) : matrix;
    g->ff = (double)g->f * (double)g->f;
    // R = ky (Y - 16 s) + kc c0 (V - 128 s), G = ky (Y - 16 s) - kc c1 (U - 128 s) - kc c2 (V - 128 s), B = ky (Y - 16 s) + kc c3 (U - 128 s)
    const double *c = m[g->matrix];
    const double s = (double)(1u << (bits - 8));
    const double ky = 255.0 / (219.0 * s), kc = 255.0 / (224.0 * s);
    for (int q = 0; q < 3; ++q) {
        const double a = plane[q][0], b = plane[q][1], d = plane[q][2];
        g->k[q][0] = (a + b + d) * ky;
        g->k[q][1] = (d * c[3] - b * c[1]) * kc;
        g->k[q][2] = (a * c[0] - b * c[2]) * kc;
        g->k[q][3] = -(g->k[q][0] * 16.0 * s + g->k[q][1] * 128.0 * s + g->k[q][2] * 128.0 * s);
    }
    return 0;
}

namespace tmm {

typedef TMM_REAL real;

__device__ __forceinline__ float root(float x) { return sqrtf(x); }
__device__ __forceinline__ double root(double x) { return sqrt(x); }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

struct Lds {
    real v[2][3][TMM_LH][TMM_LW];   // [picture][L, H, M][row][column]
    double a[TMM_THREADS], b[TMM_THREADS];
    unsigned n[TMM_THREADS];
};

// the exact integers of one window of one picture
struct Sums {
    unsigned y, u, v, n;
};

struct Z {
    double re, im;
};

// elements x .. x+3 (x a multiple of 4, x >= 0) of one row of `lim` elements; elements at or beyond lim are 0 and are not fetched
template <int FMT>
__device__ __forceinline__ void load_group(const char *row, bool vec, int x, int lim, int shift, unsigned mask, unsigned (&v)[4])
{
    if (vec && x + 4 <= lim) {
        const tmx::Raw4 q = tmx::load4_raw(row, FMT, x);
        tmx::unpack4(q, FMT, x, shift, mask, v);
    } else { // an unaligned picture or the row's last, partial group: sample by sample
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = x + k < lim ? tmx::sample1(row, FMT, x + k, shift, mask) : 0u;
    }
}

// window positions in [a, b] that take chroma index c
__device__ __forceinline__ unsigned weight(int a, int b, int c) { return (unsigned)(imin(b, 2 * c + 1) - imax(a, 2 * c) + 1); }

// SY, SU, SV and n_in of decimated position (i, j): luma rows j f - ceil(f / 2) + 1 .. j f + floor(f / 2) and the same span of columns,
// cut to the picture.  SY < 2^30 (128^2 samples below 2^16), SU and SV alike.
template <int LAYOUT, int FMT>
__device__ __forceinline__ Sums box_sums(const TmMdsiGeom &g, const TmCiedeDesc &d, int i, int j)
{
    constexpr bool BI = LAYOUT == TMC_NV12 || LAYOUT == TMC_P016;
    const int f = (int)g.f, lead = (f + 1) / 2 - 1;
    const int ra = imax(j * f - lead, 0), rb = imin(j * f - lead + f - 1, (int)g.b.h - 1);
    const int ca = imax(i * f - lead, 0), cb = imin(i * f - lead + f - 1, (int)g.b.w - 1);
    Sums s = {0u, 0u, 0u, 0u};
    if (ra > rb || ca > cb) return s;
    s.n = (unsigned)((rb - ra + 1) * (cb - ca + 1));
    const bool vec = d.vec != 0;
    for (int y = ra; y <= rb; ++y) {
        const char *row = (const char *)d.p0 + (size_t)y * d.pitch;
        for (int x = ca & ~3; x <= cb; x += 4) {
            unsigned v[4];
            load_group<FMT>(row, vec, x, (int)g.b.w, g.b.shift, g.b.mask, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) s.y += x + k >= ca && x + k <= cb ? v[k] : 0u;
        }
    }
    const int cya = ra >> 1, cyb = rb >> 1, cxa = ca >> 1, cxb = cb >> 1;
    for (int cy = cya; cy <= cyb; ++cy) {
        const unsigned wy = weight(ra, rb, cy);
        const char *ru = (const char *)d.p1 + (size_t)cy * d.pitch2;
        if (BI) { // Cb at the even, Cr at the odd elements
            for (int x = (2 * cxa) & ~3; x <= 2 * cxb + 1; x += 4) {
                unsigned v[4];
                load_group<FMT>(ru, vec, x, 2 * (int)g.b.cw, g.b.shift, g.b.mask, v);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int cx = (x >> 1) + k;
                    const unsigned wt = cx >= cxa && cx <= cxb ? wy * weight(ca, cb, cx) : 0u;
                    s.u += wt * v[2 * k]; s.v += wt * v[2 * k + 1];
                }
            }
        } else {
            const char *rv = (const char *)d.p2 + (size_t)cy * d.pitch2;
            for (int x = cxa & ~3; x <= cxb; x += 4) {
                unsigned u[4], v[4];
                load_group<FMT>(ru, vec, x, (int)g.b.cw, g.b.shift, g.b.mask, u);
                load_group<FMT>(rv, vec, x, (int)g.b.cw, g.b.shift, g.b.mask, v);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cx = x + k;
                    const unsigned wt = cx >= cxa && cx <= cxb ? wy * weight(ca, cb, cx) : 0u;
                    s.u += wt * u[k]; s.v += wt * v[k];
                }
            }
        }
    }
    return s;
}

// plane q (L, H, M) of a window: the affine map of the exact sums in f64, the divisor f^2, rounded once to `real`
__device__ __forceinline__ real plane_of(const TmMdsiGeom &g, int q, const Sums &s)
{
    const double t = ((g.k[q][0] * (double)s.y + g.k[q][1] * (double)s.u) + g.k[q][2] * (double)s.v) + g.k[q][3] * (double)s.n;
    return (real)(t / g.ff);
}

// the definition's one expression per position: each similarity as 1 - e, so that equal inputs give exactly 1
__device__ __forceinline__ float gcs_of(real gxr, real gyr, real gxd, real gyd, real hr, real hd, real mr, real md)
{
    const real ar = gxr * gxr + gyr * gyr, ad = gxd * gxd + gyd * gyd;
    const real sx = gxr + gxd, sy = gyr + gyd;
    const real af4 = sx * sx + sy * sy;               // four times the fused picture's squared gradient
    const real gr = root(ar), gd = root(ad), gf = root(af4) * (real)0.5;
    const real af = af4 * (real)0.25;
    const real d12 = gr - gd, d13 = gr - gf, d23 = gd - gf;
    const real e12 = (d12 * d12) / ((ar + ad) + (real)TMM_C1);
    const real e13 = (d13 * d13) / ((ar + af) + (real)TMM_C2);
    const real e23 = (d23 * d23) / ((ad + af) + (real)TMM_C2);
    const real dh = hr - hd, dm = mr - md;
    const real ec = (dh * dh + dm * dm) / ((((hr * hr + hd * hd) + mr * mr) + md * md) + (real)TMM_C3);
    const real eg = (e12 + e23) - e13;
    return (float)((real)1.0 - ((real)TMM_ALPHA * eg + ((real)1.0 - (real)TMM_ALPHA) * ec));
}

// the principal fourth root of the f32 map value
__device__ __forceinline__ Z z_of(float gcs)
{
    const double a = (double)gcs;
    Z z;
    if (a >= 0.0) {
        z.re = sqrt(sqrt(a)); z.im = 0.0;
    } else {
        const double t = sqrt(sqrt(-a)) * 0.70710678118654752440;
        z.re = t; z.im = t;
    }
    return z;
}

// the two-level tree: 256 values -> 16 sums of 16 neighbours -> their sum, each level in index order.  Lane 0 holds the result.  All
// lanes of the workgroup call it.
template <class T>
__device__ __forceinline__ void tree_sum(T &t, unsigned tid, double &a, double &b, unsigned long long &n)
{
    t.a[tid] = a; t.b[tid] = b; t.n[tid] = (unsigned)n;
    TM_LDS_BARRIER();
    if (tid < 16) {
        a = 0.0; b = 0.0; n = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { a += t.a[tid * 16 + k]; b += t.b[tid * 16 + k]; n += t.n[tid * 16 + k]; }
    }
    TM_LDS_BARRIER();
    if (tid < 16) { t.a[tid] = a; t.b[tid] = b; t.n[tid] = (unsigned)n; }
    TM_LDS_BARRIER();
    if (tid == 0) {
        a = 0.0; b = 0.0; n = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { a += t.a[k]; b += t.b[k]; n += t.n[k]; }
    }
}

struct Tree {
    double a[TMM_THREADS], b[TMM_THREADS];
    unsigned n[TMM_THREADS];
};

} // namespace tmm

// desc: [slot][side]; maps: [slot][g.hd][g.wd]; cells: [slot][g.cells].  FMT as in k_ciede: five instantiations (TMC_DISPATCH).
template <int LAYOUT, int FMT>
__global__ void __launch_bounds__(TMM_THREADS) k_mdsi(TmMdsiGeom g, const TmCiedeDesc *__restrict__ desc, float *__restrict__ maps, TmMdsiCell *__restrict__ cells)
{
    using namespace tmm;
    __shared__ Lds L;
    const unsigned tid = threadIdx.x, slot = blockIdx.y, t = blockIdx.x;
    const int x0 = (int)((t % g.tx) * TMM_TW), y0 = (int)((t / g.tx) * TMM_TH); // the tile's first decimated position

    // ---- 1. L, H, M of the tile and its halo
    for (unsigned it = tid; it < TMM_ITEMS; it += TMM_THREADS) {
        const int lj = (int)(it / TMM_LW), li = (int)(it % TMM_LW);
        const int i = x0 - 1 + li, j = y0 - 1 + lj;
        const bool inside = i >= 0 && j >= 0 && i < (int)g.wd && j < (int)g.hd;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            real v[3] = {(real)0.0, (real)0.0, (real)0.0};
            if (inside) {
                const TmCiedeDesc d = desc[2 * slot + p];
                const Sums s = box_sums<LAYOUT, FMT>(g, d, i, j);
#pragma unroll
                for (int q = 0; q < 3; ++q) v[q] = plane_of(g, q, s);
            }
#pragma unroll
            for (int q = 0; q < 3; ++q) L.v[p][q][lj][li] = v[q];
        }
    }
    TM_LDS_BARRIER();

    // ---- 2. the lane's positions: LDS column c + 1 is decimated column x0 + c, LDS row r + 1 is decimated row y0 + r
    const unsigned c = tid % TMM_TW, q = tid / TMM_TW;
    const unsigned px = (unsigned)x0 + c;
    double re = 0.0, im = 0.0;
    unsigned long long neg = 0;
#pragma unroll
    for (int k = 0; k < TMM_ROWS_PER_LANE; ++k) {
        const unsigned r = q * TMM_ROWS_PER_LANE + k, py = (unsigned)y0 + r;
        if (px < g.wd && py < g.hd) {
            real gx[2], gy[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const real(*s)[TMM_LW] = L.v[p][0];
                gx[p] = (((s[r][c + 2] - s[r][c]) + (s[r + 1][c + 2] - s[r + 1][c])) + (s[r + 2][c + 2] - s[r + 2][c])) / (real)3.0;
                gy[p] = (((s[r + 2][c] - s[r][c]) + (s[r + 2][c + 1] - s[r][c + 1])) + (s[r + 2][c + 2] - s[r][c + 2])) / (real)3.0;
            }
            const float gcs = gcs_of(gx[0], gy[0], gx[1], gy[1], L.v[0][1][r + 1][c + 1], L.v[1][1][r + 1][c + 1], L.v[0][2][r + 1][c + 1],
                                     L.v[1][2][r + 1][c + 1]);
            maps[((size_t)slot * g.hd + py) * g.wd + px] = gcs;
            const Z z = z_of(gcs);
            re += z.re; im += z.im;
            neg += gcs < 0.0f ? 1u : 0u;
        }
    }

    // ---- 3. the tile
    tree_sum(L, tid, re, im, neg);
    if (tid == 0) {
        TmMdsiCell cell;
        cell.a = re; cell.b = im; cell.n = neg;
        cells[(size_t)slot * g.cells + t] = cell;
    }
}

// grid (slots), block 256: the sums of the slot's `ncells` cells in a fixed order: lane i adds cells i, i + 256, ..., then the tree.
// stage 0 (after k_mdsi) writes re, im, neg of the slot's result; stage 1 (after k_mdsi_dev) writes dev.
__global__ void __launch_bounds__(TMM_THREADS) k_mdsi_finish(const TmMdsiCell *__restrict__ cells, unsigned ncells, int stage, TmMdsiRes *__restrict__ res)
{
    __shared__ tmm::Tree tree;
    const unsigned tid = threadIdx.x, slot = blockIdx.x;
    const TmMdsiCell *cl = cells + (size_t)slot * ncells;
    double a = 0.0, b = 0.0;
    unsigned long long n = 0;
    for (unsigned i = tid; i < ncells; i += TMM_THREADS) { a += cl[i].a; b += cl[i].b; n += cl[i].n; }
    // the tree's 32-bit words hold every count: a slot has at most 32768 x 32768 = 2^30 positions
    tmm::tree_sum(tree, tid, a, b, n);
    if (tid == 0) {
        if (stage == 0) { res[slot].re = a; res[slot].im = b; res[slot].neg = n; }
        else res[slot].dev = a;
    }
}

// maps: [slot][g.n]; res: [slot], stage 0 done; cells: [slot][g.cells2]
__global__ void __launch_bounds__(TMM_THREADS) k_mdsi_dev(TmMdsiGeom g, const float *__restrict__ maps, const TmMdsiRes *__restrict__ res, TmMdsiCell *__restrict__ cells)
{
    using namespace tmm;
    __shared__ Tree tree;
    const unsigned tid = threadIdx.x, slot = blockIdx.y, t = blockIdx.x;
    const double nn = (double)g.n;
    const double mur = res[slot].re / nn, mui = res[slot].im / nn;
    const float *m = maps + (size_t)slot * g.n;
    double dev = 0.0, zero = 0.0;
    unsigned long long none = 0;
#pragma unroll
    for (int k = 0; k < TMM_DEV_PER_LANE; ++k) {
        const unsigned long long idx = ((unsigned long long)t * TMM_DEV_PER_LANE + (unsigned)k) * TMM_THREADS + tid;
        if (idx < g.n) {
            const Z z = z_of(m[idx]);
            const double dr = z.re - mur, di = z.im - mui;
            dev += sqrt(dr * dr + di * di);
        }
    }
    tree_sum(tree, tid, dev, zero, none);
    if (tid == 0) {
        TmMdsiCell cell;
        cell.a = dev; cell.b = 0.0; cell.n = 0;
        cells[(size_t)slot * g.cells2 + t] = cell;
    }
}
