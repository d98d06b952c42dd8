// tm_cambi_kernels.h -- gfx950 kernels of CAMBI, VMAF's banding index (libturbometrics_cambi.so, include/turbo_metrics_cambi.h).
//
// The definition is DESIGN.md section 13; its literal CPU restatement is tests/cambi_ref.py.  Everything up to one IEEE f32 division
// per pixel and contrast is integer.  All kernels: block 256, slots in grid y; a
// picture's workgroups are grid x, rows of tiles (bands, rows) outermost.
//
//   k_cambi_ingest<FMT>   grid (4-sample groups / 256 x rows, slots)   a lane reads one group of four samples of rows y and y + 1 and
//                         the sample right of the group (tmx::load4: wide loads when base and pitch allow, sample by sample
//                         otherwise), shifts to 10 bits and, below 10 bits, applies the 2 x 2 anti-dither filter.  -> P0, uint16.
//   k_cambi_mask          grid (w / 64 x h / 16, slots)   a 64 x 16 tile: the zero-derivative flags of the tile and a 3-pixel apron into
//                         LDS, the 7-wide row sums into LDS, the 7-high column sums compared with mask_index.  -> M0, bytes.
//   k_cambi_mode<FIRST>   grid (pixels / 256, slots)   scale s: reads the 3 x 3 neighbours from P0 (FIRST) or from every second
//                         row and column of the filtered plane of scale s - 1, and writes Q_s = mode3x3 | mask << 15 -- the mask
//                         travels in bit 15 of the 10-bit plane, so that the hot kernel needs one load per sample.
//   k_cambi_cvalues       grid (column strips x row bands, slots)   the hot kernel.  A workgroup owns `oc` output columns and the
//                         `pad` columns on either side (at most TMC_MAX_COLS columns), and one histogram of masked samples per
//                         column in LDS: 1024 + 8 byte counters (a count is at most 2 pad + 1 <= 127), column stride 259 dwords
//                         (odd: the lanes of a half-wave, on neighbouring columns and the same value, read different banks).  Lane
//                         t owns column t's counters: walking down, a row enters with one increment and leaves with one decrement,
//                         no atomics.  The nine window counts n(v - 4) .. n(v + 4) of a pixel are nine consecutive bytes of every
//                         column of its window: three aligned dwords per column, added up as packed 16-bit pairs (even and odd
//                         bytes apart; a sum is at most 127 * 127 < 2^16).  Columns outside the picture stay zero, which IS the
//                         clipping of the window.  Unmasked pixels and pixels above tvi[4] skip the window.  The next row's three
//                         samples are loaded before the current row is computed.  A band starts from zeroed counters and warms
//                         up on the 2 pad rows around its first row.
//   k_cambi_pool          grid (scales, slots)   one workgroup per plane of c-values: radix select of the k-th largest f32 bit
//                         pattern -- 15 high bits (the sign is never set) in a 32768-bin LDS histogram, then bits 15 .. 8, then bits
//                         7 .. 0 -- with the counts strictly above the chosen bin at each level adding up to n_gt, then the f64 sum of
//                         the values above t: per lane in index order, then a fixed tree over the lanes.  Integer LDS atomics only
//                         (exact in any order); a lane folds a run of equal bins into one add.
//
// Every output cell is written by every compute with plain vector stores; nothing is zeroed by the host.
#pragma once
#include <math.h>
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::load4 / sample1: the loaders of the XPSNR, motion, VIF, ADM and scene kernels

#define TMC_THREADS 256
#define TMC_SCALES 5
#define TMC_COL_WORDS 259u                 /* dwords per column histogram: 1032 byte counters and one dword of padding */
#define TMC_COL_BYTES (TMC_COL_WORDS * 4u)
#define TMC_MAX_COLS 156u                  /* 156 * 1036 B = 161 616 B of the 163 840 B of a CU */
#define TMC_POOL_BINS 32768u
#define TMC_MASK_TW 64
#define TMC_MASK_TH 16

// layouts of include/turbo_metrics_cambi.h (motion's numbering)
enum { TMC_Y8 = 0, TMC_Y16_MSB = 1, TMC_Y16_LOW = 2, TMC_Y10_PACKED = 3 };

// one picture of a slot
struct TmCambiDesc {
    const void *p;
    unsigned long long pitch; // bytes
    int vec;                  // base and pitch 16-byte aligned: the wide loads are allowed
    int pad_;
};

// one slot's result: the layout of tm_cambi_frame
struct TmCambiRes {
    unsigned t[TMC_SCALES], n_gt[TMC_SCALES], k[TMC_SCALES], pad_;
    double sum_gt[TMC_SCALES];
};

struct TmCambiGeom {
    unsigned w[TMC_SCALES], h[TMC_SCALES];
    unsigned long long off[TMC_SCALES]; // first element of scale s in a slot's pyramid
    unsigned long long tot;             // elements of a slot's pyramid
    unsigned k[TMC_SCALES];
    int bits, fmt, shift;               // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;                      // TMX_F_U16_LOW: sample = v & mask
    int up, down;                       // P0 = (sample << up) >> down
    unsigned window, pad, oc, band_rows;
    unsigned tvi[4], mask_index;
};

// ---- host functions of the definition ------------------------------------------------------------------------------------------
static inline unsigned tmc_window(unsigned w, unsigned requested)
{
    if (requested) return requested;
    const unsigned long long d = 63ull * w / 3840ull;
    return d < 3 ? 3u : (unsigned)d;
}

static inline unsigned tmc_mask_index(unsigned w, unsigned h)
{
    const unsigned m = w < h ? w : h;
    int e = 0;
    while ((1ull << e) < m) ++e; // ceil(log2(m))
    return (unsigned)((49 + 3 * (e - 11) - 1) >> 1);
}

static inline double tmc_luminance(double x)
{
    const double Lw = 300.0, Lb = 0.01, g = 2.4;
    const double rw = pow(Lw, 1.0 / g), rb = pow(Lb, 1.0 / g);
    const double a = pow(rw - rb, g), b = rb / (rw - rb);
    double v = (x - 64.0) / 876.0;
    v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);
    const double s = v + b;
    return a * pow(s > 0.0 ? s : 0.0, g);
}

static inline void tmc_tvi(double threshold, unsigned out[4])
{
    for (int d = 1; d <= 4; ++d) {
        unsigned best = 0; // no x qualifies: no sample is at or below it but 0
        for (unsigned x = 64; x <= 939; ++x) {
            const double L = tmc_luminance((double)x);
            if (tmc_luminance((double)(x + d)) - L > threshold * L) best = x;
        }
        out[d - 1] = best;
    }
}

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED
static inline int tmc_make_geom(TmCambiGeom *g, unsigned w, unsigned h, int layout, unsigned bits, unsigned window, double topk, double tvi_threshold)
{
    memset(g, 0, sizeof *g);
    if (w < 32 || h < 32 || (unsigned long long)w * h > (1ull << 31) || bits < 8 || bits > 16) return -1;
    if (window != 0 && (window < 3 || window > 127)) return -1;
    if (!(topk > 0.0 && topk <= 1.0)) return -1;
    switch (layout) {
    case TMC_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMC_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMC_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMC_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->bits = (int)bits;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->up = bits < 10 ? 10 - (int)bits : 0;
    g->down = bits > 10 ? (int)bits - 10 : 0;
    g->window = tmc_window(w, window);
    if (g->window > 127) g->window = 127; // a derived window of a picture wider than 7741 samples
    g->pad = g->window >> 1;
    g->oc = TMC_MAX_COLS - 2 * g->pad;
    g->band_rows = 8 * g->pad + 8;
    unsigned long long off = 0;
    for (int s = 0; s < TMC_SCALES; ++s) {
        g->w[s] = s ? (g->w[s - 1] + 1) >> 1 : w;
        g->h[s] = s ? (g->h[s - 1] + 1) >> 1 : h;
        g->off[s] = off;
        const unsigned long long n = (unsigned long long)g->w[s] * g->h[s];
        off += (n + 3) / 4 * 4;
        double k = floor(topk * (double)n);
        if (k < 1.0) k = 1.0;
        if (k > (double)n) k = (double)n;
        g->k[s] = (unsigned)k;
    }
    g->tot = off;
    tmc_tvi(tvi_threshold, g->tvi);
    g->mask_index = tmc_mask_index(w, h);
    return 0;
}

// ---- ingest --------------------------------------------------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(TMC_THREADS) k_cambi_ingest(TmCambiGeom g, const TmCambiDesc *__restrict__ desc, unsigned short *__restrict__ p0)
{
    const unsigned w = g.w[0], h = g.h[0], bpr = ((w + 3) / 4 + TMC_THREADS - 1) / TMC_THREADS; // blocks per row
    const unsigned gx = (blockIdx.x % bpr) * TMC_THREADS + threadIdx.x, y = blockIdx.x / bpr, slot = blockIdx.y;
    if (gx >= (w + 3) / 4) return;
    const TmCambiDesc d = desc[slot];
    const tmx::Src src = {(const char *)d.p, d.pitch, FMT, d.vec};
    const int x = (int)(4u * gx);
    unsigned a[5], b[5] = {0u, 0u, 0u, 0u, 0u};
    {
        unsigned v[4];
        tmx::load4(src, x, (int)y, (int)w, g.shift, g.mask, v);
        for (int k = 0; k < 4; ++k) a[k] = (v[k] << g.up) >> g.down;
        a[4] = 0u;
    }
    const bool dither = g.up > 0, below = y + 1 < h, right = (unsigned)x + 4u < w;
    if (dither) {
        if (right) a[4] = tmx::sample1(src.p + (size_t)y * d.pitch, FMT, x + 4, g.shift, g.mask) << g.up;
        if (below) {
            unsigned v[4];
            tmx::load4(src, x, (int)y + 1, (int)w, g.shift, g.mask, v);
            for (int k = 0; k < 4; ++k) b[k] = v[k] << g.up;
            if (right) b[4] = tmx::sample1(src.p + (size_t)(y + 1) * d.pitch, FMT, x + 4, g.shift, g.mask) << g.up;
        }
    }
    unsigned short *o = p0 + (size_t)slot * w * h + (size_t)y * w + (unsigned)x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((unsigned)x + k >= w) break;
        unsigned r = a[k];
        if (dither) {
            const bool rt = (unsigned)x + k + 1 < w;
            if (rt && below) r = (a[k] + a[k + 1] + b[k] + b[k + 1]) >> 2;
            else if (below) r = (a[k] + b[k]) >> 1;
            else if (rt) r = (a[k] + a[k + 1]) >> 1;
        }
        o[k] = (unsigned short)r;
    }
}

// ---- spatial mask --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(TMC_THREADS) k_cambi_mask(TmCambiGeom g, const unsigned short *__restrict__ p0, unsigned char *__restrict__ mk)
{
    constexpr int ZW = TMC_MASK_TW + 6, ZH = TMC_MASK_TH + 6;
    __shared__ unsigned char z[ZH * ZW];
    __shared__ unsigned char hs[ZH * TMC_MASK_TW];
    const unsigned tid = threadIdx.x, slot = blockIdx.y;
    const long long w = g.w[0], h = g.h[0];
    const unsigned tpr = (g.w[0] + TMC_MASK_TW - 1) / TMC_MASK_TW; // tiles per row of tiles
    const long long x0 = (long long)(blockIdx.x % tpr) * TMC_MASK_TW, y0 = (long long)(blockIdx.x / tpr) * TMC_MASK_TH;
    const unsigned short *P = p0 + (size_t)slot * w * h;
    for (int i = (int)tid; i < ZH * ZW; i += TMC_THREADS) {
        const long long y = y0 - 3 + i / ZW, x = x0 - 3 + i % ZW;
        unsigned char f = 0;
        if (x >= 0 && x < w && y >= 0 && y < h) {
            const unsigned v = P[y * w + x];
            const bool er = x == w - 1 || P[y * w + x + 1] == v;
            const bool ed = y == h - 1 || P[(y + 1) * w + x] == v;
            f = er && ed;
        }
        z[i] = f;
    }
    TM_LDS_BARRIER();
    for (int i = (int)tid; i < ZH * TMC_MASK_TW; i += TMC_THREADS) {
        const int r = i / TMC_MASK_TW, c = i % TMC_MASK_TW;
        unsigned t = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) t += z[r * ZW + c + k];
        hs[i] = (unsigned char)t;
    }
    TM_LDS_BARRIER();
    for (int i = (int)tid; i < TMC_MASK_TH * TMC_MASK_TW; i += TMC_THREADS) {
        const int r = i / TMC_MASK_TW, c = i % TMC_MASK_TW;
        unsigned t = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) t += hs[(r + k) * TMC_MASK_TW + c];
        if (y0 + r < h && x0 + c < w) mk[(size_t)slot * w * h + (size_t)(y0 + r) * w + (x0 + c)] = t > g.mask_index;
    }
}

// ---- mode filter, subsampling ----------------------------------------------------------------------------------------------------
// src: P0 (FIRST) or the pyramid q; both q pointers are the same buffer, read at scale s - 1 and written at scale s
template <bool FIRST>
__global__ void __launch_bounds__(TMC_THREADS) k_cambi_mode(TmCambiGeom g, int s, const unsigned short *src, const unsigned char *__restrict__ mk, unsigned short *q)
{
    const unsigned slot = blockIdx.y;
    const unsigned long long w = g.w[s], h = g.h[s], idx = (unsigned long long)blockIdx.x * TMC_THREADS + threadIdx.x;
    if (idx >= w * h) return;
    const unsigned long long i = idx / w, j = idx % w;
    const unsigned long long sw = FIRST ? w : g.w[s - 1];
    const unsigned short *S = FIRST ? src + (size_t)slot * w * h : src + (size_t)slot * g.tot + g.off[s - 1];
    const int step = FIRST ? 1 : 2;
    const unsigned centre = S[(i * step) * sw + j * step];
    const unsigned m = FIRST ? (unsigned)(mk[(size_t)slot * w * h + idx] != 0) : centre >> 15;
    unsigned out = centre & 1023u;
    if (i > 0 && j > 0 && i + 1 < h && j + 1 < w) {
        unsigned v[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) v[a * 3 + b] = S[((i + a - 1) * step) * sw + (j + b - 1) * step] & 1023u;
        unsigned best = 0, bv = 0;
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            unsigned c = 0;
#pragma unroll
            for (int b = 0; b < 9; ++b) c += v[b] == v[a];
            if (c > best || (c == best && v[a] < bv)) { best = c; bv = v[a]; }
        }
        out = bv;
    }
    q[(size_t)slot * g.tot + g.off[s] + idx] = (unsigned short)(out | (m << 15));
}

// ---- c-values ------------------------------------------------------------------------------------------------------------------
namespace tmc {

// the c-value of a masked pixel of value v from the nine window counts n[k] = n(v - 4 + k)
__device__ __forceinline__ float cvalue(unsigned v, const unsigned (&n)[9], const unsigned (&tvi)[4])
{
    const unsigned p0 = n[4];
    float c = 0.0f;
#pragma unroll
    for (unsigned d = 1; d <= 4; ++d) {
        if (v > tvi[d - 1]) continue;
        const unsigned hi = n[4 + d], lo = n[4 - d], m = hi > lo ? hi : lo;
        const float cd = (float)(d * p0 * m) / (float)(p0 + m);
        c = cd > c ? cd : c;
    }
    return c;
}

} // namespace tmc

__global__ void __launch_bounds__(TMC_THREADS) k_cambi_cvalues(TmCambiGeom g, int s, const unsigned short *__restrict__ q, float *__restrict__ cv)
{
    __shared__ unsigned lds[TMC_MAX_COLS * TMC_COL_WORDS];
    unsigned char *hb = (unsigned char *)lds;
    const unsigned tid = threadIdx.x, slot = blockIdx.y;
    const unsigned w = g.w[s], h = g.h[s], pad = g.pad, oc = g.oc, cw = oc + 2 * pad;
    const unsigned strips = (w + oc - 1) / oc;
    const unsigned x0 = (blockIdx.x % strips) * oc, y0 = (blockIdx.x / strips) * g.band_rows;
    const unsigned y1 = y0 + g.band_rows < h ? y0 + g.band_rows : h;
    const unsigned short *Q = q + (size_t)slot * g.tot + g.off[s];
    float *Cv = cv + (size_t)slot * g.tot + g.off[s];

    for (unsigned k = tid; k < cw * TMC_COL_WORDS; k += TMC_THREADS) lds[k] = 0u;
    TM_LDS_BARRIER();

    const long long col = (long long)x0 - (long long)pad + (long long)tid; // the column whose counters this lane owns
    const bool owner = tid < cw && col >= 0 && col < (long long)w;
    const bool writer = tid < oc && x0 + tid < w;                          // ... and the output column it computes
    unsigned char *mine = hb + (size_t)(tid < cw ? tid : 0) * TMC_COL_BYTES + 4;
    // the rows below y0 + pad: what the window of row y0 holds before row y0 + pad enters
    if (owner) {
        const unsigned ra = y0 > pad ? y0 - pad : 0u, rb = y0 + pad < h ? y0 + pad : h;
        for (unsigned r = ra; r < rb; ++r) {
            const unsigned t = Q[(size_t)r * w + (size_t)col];
            if (t >> 15) mine[t & 1023u] += 1;
        }
    }
    // a value of 0 has bit 15 clear: "nothing to do"
    unsigned nadd = owner && y0 + pad < h ? Q[(size_t)(y0 + pad) * w + (size_t)col] : 0u, nrem = 0u;
    unsigned nctr = writer ? Q[(size_t)y0 * w + x0 + tid] : 0u;
    for (unsigned y = y0; y < y1; ++y) {
        const unsigned add = nadd, rem = nrem, ctr = nctr;
        const unsigned yn = y + 1;
        nadd = owner && yn < y1 && yn + pad < h ? Q[(size_t)(yn + pad) * w + (size_t)col] : 0u;
        nrem = owner && yn < y1 && yn >= pad + 1 ? Q[(size_t)(yn - pad - 1) * w + (size_t)col] : 0u;
        nctr = writer && yn < y1 ? Q[(size_t)yn * w + x0 + tid] : 0u;
        if (add >> 15) mine[add & 1023u] += 1;
        if (rem >> 15) mine[rem & 1023u] -= 1;
        TM_LDS_BARRIER();
        if (writer) {
            float c = 0.0f;
            const unsigned v = ctr & 1023u;
            if ((ctr >> 15) && v <= g.tvi[3]) {
                // indices v .. v + 8 of a column are the bins v - 4 .. v + 4: the three dwords from (v & ~3) hold them
                const unsigned *p = lds + (size_t)tid * TMC_COL_WORDS + (v >> 2);
                unsigned e0 = 0, o0 = 0, e1 = 0, o1 = 0, e2 = 0, o2 = 0;
#pragma unroll 4
                for (unsigned dc = 0; dc <= 2 * pad; ++dc, p += TMC_COL_WORDS) {
                    const unsigned a = p[0], b = p[1], d = p[2];
                    e0 += a & 0x00FF00FFu; o0 += (a >> 8) & 0x00FF00FFu;
                    e1 += b & 0x00FF00FFu; o1 += (b >> 8) & 0x00FF00FFu;
                    e2 += d & 0x00FF00FFu; o2 += (d >> 8) & 0x00FF00FFu;
                }
                const unsigned sum[12] = {e0 & 0xFFFFu, o0 & 0xFFFFu, e0 >> 16, o0 >> 16, e1 & 0xFFFFu, o1 & 0xFFFFu,
                                          e1 >> 16,     o1 >> 16,     e2 & 0xFFFFu, o2 & 0xFFFFu, e2 >> 16, o2 >> 16};
                unsigned n[9];
                const unsigned r = v & 3u;
#pragma unroll
                for (int k = 0; k < 9; ++k) n[k] = r == 0 ? sum[k] : (r == 1 ? sum[k + 1] : (r == 2 ? sum[k + 2] : sum[k + 3]));
                c = tmc::cvalue(v, n, g.tvi);
            }
            Cv[(size_t)y * w + x0 + tid] = c;
        }
        TM_LDS_BARRIER();
    }
}

// ---- pooling -------------------------------------------------------------------------------------------------------------------
namespace tmc {

// a run of equal bins of one lane is one LDS add
struct Folder {
    unsigned cur, cnt;
    __device__ __forceinline__ void put(unsigned *hist, unsigned b)
    {
        if (b == cur) { ++cnt; return; }
        if (cnt) atomicAdd(&hist[cur], cnt);
        cur = b; cnt = 1;
    }
    __device__ __forceinline__ void flush(unsigned *hist)
    {
        if (cnt) atomicAdd(&hist[cur], cnt);
        cnt = 0;
    }
};

// The bin that holds the k-th largest entry of hist[0 .. nbins) (nbins a multiple of 256, k at least 1 and at most the total), and
// the number of entries in the bins above it.  Every lane calls; every lane gets the answer.  part: 256 words, sel: 2 words of LDS.
__device__ __forceinline__ void select(const unsigned *hist, unsigned nbins, unsigned k, unsigned *part, unsigned *sel, unsigned &bin, unsigned &above)
{
    const unsigned tid = threadIdx.x, per = nbins / TMC_THREADS;
    TM_LDS_BARRIER(); // the histogram is complete
    unsigned t = 0;
    for (unsigned i = 0; i < per; ++i) t += hist[tid * per + ((i + tid) & (per - 1))]; // per is a power of two: rotated, against bank conflicts
    part[tid] = t;
    TM_LDS_BARRIER();
    if (tid == 0) {
        unsigned acc = 0;
        int c = TMC_THREADS - 1;
        while (c > 0 && acc + part[c] < k) { acc += part[c]; --c; }
        int b = (int)(c * per + per - 1);
        while (b > (int)(c * per) && acc + hist[b] < k) { acc += hist[b]; --b; }
        sel[0] = (unsigned)b;
        sel[1] = acc;
    }
    TM_LDS_BARRIER();
    bin = sel[0];
    above = sel[1];
    TM_LDS_BARRIER(); // sel and the histogram may be written again
}

} // namespace tmc

__global__ void __launch_bounds__(TMC_THREADS) k_cambi_pool(TmCambiGeom g, const float *__restrict__ cv, TmCambiRes *__restrict__ res)
{
    __shared__ unsigned hist[TMC_POOL_BINS];
    __shared__ unsigned part[TMC_THREADS];
    __shared__ unsigned sel[2];
    __shared__ double dsum[TMC_THREADS];
    const unsigned tid = threadIdx.x, s = blockIdx.x, slot = blockIdx.y;
    const unsigned long long n = (unsigned long long)g.w[s] * g.h[s];
    const unsigned *src = (const unsigned *)(cv + (size_t)slot * g.tot + g.off[s]);
    const unsigned k = g.k[s];
    unsigned prefix = 0, pmask = 0, n_gt = 0, kk = k;
    // level 0: bits 30 .. 16; level 1: bits 15 .. 8; level 2: bits 7 .. 0
    for (int level = 0; level < 3; ++level) {
        const unsigned nbins = level == 0 ? TMC_POOL_BINS : 256u, sh = level == 0 ? 16u : (level == 1 ? 8u : 0u);
        for (unsigned i = tid; i < nbins; i += TMC_THREADS) hist[i] = 0u;
        TM_LDS_BARRIER();
        tmc::Folder f = {0u, 0u};
        unsigned long long i = tid;
        for (; i + 3ull * TMC_THREADS < n; i += 4ull * TMC_THREADS) {
            const unsigned b0 = src[i], b1 = src[i + TMC_THREADS], b2 = src[i + 2 * TMC_THREADS], b3 = src[i + 3 * TMC_THREADS];
            if ((b0 & pmask) == prefix) f.put(hist, (b0 >> sh) & (nbins - 1));
            if ((b1 & pmask) == prefix) f.put(hist, (b1 >> sh) & (nbins - 1));
            if ((b2 & pmask) == prefix) f.put(hist, (b2 >> sh) & (nbins - 1));
            if ((b3 & pmask) == prefix) f.put(hist, (b3 >> sh) & (nbins - 1));
        }
        for (; i < n; i += TMC_THREADS) {
            const unsigned b0 = src[i];
            if ((b0 & pmask) == prefix) f.put(hist, (b0 >> sh) & (nbins - 1));
        }
        f.flush(hist);
        unsigned bin, above;
        tmc::select(hist, nbins, kk, part, sel, bin, above);
        n_gt += above;
        kk -= above;
        prefix |= bin << sh;
        pmask |= (nbins - 1) << sh;
    }
    const unsigned t = prefix;
    // the values above t: per lane in index order, then a fixed tree
    double acc = 0.0;
    for (unsigned long long i = tid; i < n; i += TMC_THREADS) {
        const unsigned b = src[i];
        if (b > t) acc += (double)__uint_as_float(b);
    }
    dsum[tid] = acc;
    TM_LDS_BARRIER();
    for (unsigned st = TMC_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) dsum[tid] += dsum[tid + st];
        TM_LDS_BARRIER();
    }
    if (tid == 0) {
        TmCambiRes *r = res + slot;
        r->t[s] = t;
        r->n_gt[s] = n_gt;
        r->k[s] = k;
        r->sum_gt[s] = dsum[0];
        if (s == 0) r->pad_ = 0u;
    }
}
