// tm_xpsnr_kernels.h -- gfx950 kernels of XPSNR (libturbometrics_xpsnr.so, include/turbo_metrics_xpsnr.h).
//
// The definition these kernels implement is DESIGN.md section 8 (believed to match ffmpeg's vf_xpsnr; unpinned); its literal
// CPU restatement is tests/xpsnr_ref.py, and the two cite each other tap for tap.
//
//   k_xpsnr_blocks  grid (luma blocks, slots)  block 256   one workgroup per (block, slot): integer SSE of Y / Cb / Cr, spatial
//                   activity `sa` and temporal activity `ta` of the block.  The reference luma of the block is staged band by band
//                   (32 rows plus a 2-sample halo on every side) in LDS for the high-pass taps; the distorted picture, the history
//                   pictures and the chroma blocks are read straight from memory.  Each lane reads 4 consecutive samples at a time
//                   (one dword of 8-bit, two of 16-bit, four words of the packed 10-bit kind).  Every sum is an integer: the
//                   reduction order is free and the result exact.
//   k_xpsnr_finish  grid (ceil(slots / 64))    block 64    one lane per slot walks that frame's blocks in raster order: weights in
//                   double, the in-line minimum smoothing of small pictures, the three weighted sums and their rounding.  Sequential
//                   on purpose: that is what makes it bit-exact with the restatement.
//
// History.  For slot s of a launch, m1 (the previous reference luma) is slot s-1's reference picture and m2 slot s-2's; the first
// one or two slots take them from the engine's history planes.  The workgroups of the last two slots write their reference luma
// (as uint16) into the OTHER pair of history planes, which the next launch reads: a double buffer, so that slot 0 never reads a
// history block that slot n-1 of the same launch is overwriting.
#pragma once
#include <math.h>
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_p10.h" // the packed 10-bit addressing the engine's ingest uses
#include "tm_sample_load.h" // TMX_F_*, tmx::Src / sample1 / load4: shared with the motion kernel

#define TMX_THREADS 256
#define TMX_BAND 32                             /* luma rows per LDS band (even: 2x2 cells never straddle two bands) */
#define TMX_HALO 2                              /* rows / columns around the band that the high-pass taps read */
#define TMX_MAX_B 256                           /* largest block size (pictures up to about 4 x 3840 x 2160 samples) */
#define TMX_TILE_W (TMX_MAX_B + 8)              /* LDS tile columns: x0 - 4 .. x0 + bw + 4, whole groups of 4 */
#define TMX_TILE_H (TMX_BAND + 2 * TMX_HALO)


// one picture of a slot: luma plane, then Cb / Cr (p1 = interleaved CbCr of the biplanar layouts, p2 unused there)
struct TmXpsnrDesc {
    const void *p0;
    const void *p1;
    const void *p2;
    unsigned long long pitch;  // bytes, luma rows
    unsigned long long pitch2; // bytes, chroma rows
    int vec;                   // every base and pitch 16-byte aligned: the wide loads are allowed
    int pad_;
};

struct TmXpsnrGeom {
    int w, h, cw, ch;        // luma / chroma plane sizes
    int b;                   // block size of the partition (the definition's b; 64 when b < 4, where only the SSE is used)
    int bx, by;              // chroma block size
    int wblk, hblk, nblk;    // luma block grid (== the chroma block grid, checked on the host)
    int bval;                // 1, or 2 (downsampled high-pass) above 2048 x 1152
    int second_order;        // temporal activity of second order (integer frame rate >= 32)
    int fmt_y, fmt_c;        // TMX_F_*
    int biplanar;            // NV12 / P016: p1 holds CbCr interleaved
    int shift;               // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;           // TMX_F_U16_LOW: sample = v & mask
    int small;               // b < 4: every component's result is its plain SSE
    int smooth;              // w * h <= 640 * 480: in-line minimum smoothing
    int n;                   // slots of this launch
    double avg_act;          // sqrt(16 * 2^(2D-9) / sqrt(max(1e-5, r)))
    double min_act;          // 2^(D-6)
    unsigned long long hpitch; // samples per history row
};

// ---- the definition's geometry (host code: the library's create and tests/xpsnr_emul share it) --------------------------------
// layouts of include/turbo_metrics_xpsnr.h
enum { TMX_NV12 = 0, TMX_P016 = 1, TMX_I420 = 2, TMX_I420P10 = 3 };

// b = 4 (int)(32 sqrt(r) + 0.5), r = w h / (3840 * 2160)
static inline unsigned tmx_block_size(unsigned w, unsigned h)
{
    const double r = (double)((unsigned long long)w * h) / (3840.0 * 2160.0);
    return 4u * (unsigned)(int)(32.0 * sqrt(r) + 0.5);
}

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED (w or h below 8, D outside 8 .. 16 or not the layout's, odd w or h
// with the downsampled high-pass, b above TMX_MAX_B, a chroma block grid that is not the luma grid); fps_den > 0
static inline int tmx_make_geom(TmXpsnrGeom *g, unsigned w, unsigned h, int layout, unsigned bits, unsigned fps_num, unsigned fps_den)
{
    memset(g, 0, sizeof *g);
    if (w < 8 || h < 8 || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMX_NV12: if (bits != 8) return -1; g->fmt_y = g->fmt_c = TMX_F_U8; g->biplanar = 1; break;
    case TMX_P016: if (bits < 9) return -1; g->fmt_y = g->fmt_c = TMX_F_U16_MSB; g->biplanar = 1; break;
    case TMX_I420: g->fmt_y = g->fmt_c = bits == 8 ? TMX_F_U8 : TMX_F_U16_LOW; break;
    case TMX_I420P10: if (bits != 10) return -1; g->fmt_y = g->fmt_c = TMX_F_P10; break;
    default: return -1;
    }
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    const unsigned long long px = (unsigned long long)w * h;
    g->bval = px > 2048ull * 1152ull ? 2 : 1;
    if (g->bval == 2 && ((w | h) & 1)) return -1; // the 2x2 cells would reach past the block
    const int b = (int)tmx_block_size(w, h);
    if (b > TMX_MAX_B) return -1;
    g->small = b < 4;
    g->b = g->small ? 64 : b;
    g->w = (int)w; g->h = (int)h;
    g->cw = (int)((w + 1) / 2); g->ch = (int)((h + 1) / 2);
    g->bx = g->b * g->cw / g->w; g->by = g->b * g->ch / g->h;
    g->wblk = (g->w + g->b - 1) / g->b; g->hblk = (g->h + g->b - 1) / g->b;
    g->nblk = g->wblk * g->hblk;
    // 4:2:0: the chroma block grid is the luma grid (chroma block i takes luma block i's weight)
    if (g->bx < 1 || g->by < 1 || (g->cw + g->bx - 1) / g->bx != g->wblk || (g->ch + g->by - 1) / g->by != g->hblk) return -1;
    g->second_order = fps_num / fps_den >= 32;
    g->smooth = px <= 640ull * 480ull;
    const double r = (double)px / (3840.0 * 2160.0);
    g->avg_act = sqrt(16.0 * ldexp(1.0, 2 * (int)bits - 9) / sqrt(r > 1e-5 ? r : 1e-5));
    g->min_act = ldexp(1.0, (int)bits - 6);
    g->hpitch = (unsigned long long)(g->w + 127) / 128 * 128;
    return 0;
}

// ---- wave reduction of the five block sums -------------------------------------------------------------------------------
#ifdef TM_EMULATE
// tests/xpsnr_emul: the lanes of a workgroup are host threads; the harness sums through memory, lane 0 of each wave holds the total
bool tm_xpsnr_wave_sum5(unsigned long long (&v)[5]);
#else
__device__ __forceinline__ bool tm_xpsnr_wave_sum5(unsigned long long (&v)[5])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 5; ++k) v[k] += __shfl_down(v[k], off, 64);
    }
    return (threadIdx.x & 63) == 0;
}
#endif

namespace tmx {

// chroma samples cx .. cx+3 of component c (0 = Cb, 1 = Cr) of an interleaved CbCr row (NV12 / P016)
__device__ __forceinline__ void load4_cbcr(const Src &s, int c, int cx, int cy, int lim, int shift, unsigned (&v)[4])
{
    const char *row = s.p + (size_t)cy * s.pitch;
    if (s.vec && cx + 4 <= lim) {
        if (s.fmt == TMX_F_U8) {
            const uint2 q = *(const uint2 *)(row + 2 * cx);
            v[0] = (q.x >> (8 * c)) & 255u; v[1] = (q.x >> (16 + 8 * c)) & 255u; v[2] = (q.y >> (8 * c)) & 255u; v[3] = (q.y >> (16 + 8 * c)) & 255u;
        } else {
            const uint4 q = *(const uint4 *)(row + 4 * cx);
            const unsigned h = 16u * (unsigned)c;
            v[0] = ((q.x >> h) & 0xFFFFu) >> shift; v[1] = ((q.y >> h) & 0xFFFFu) >> shift;
            v[2] = ((q.z >> h) & 0xFFFFu) >> shift; v[3] = ((q.w >> h) & 0xFFFFu) >> shift;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = cx + k < lim ? sample1(row, s.fmt, 2 * (cx + k) + c, shift, 0xFFFFu) : 0u;
}

__device__ __forceinline__ unsigned absdiff(int a) { return (unsigned)(a < 0 ? -a : a); }

} // namespace tmx

__global__ void __launch_bounds__(TMX_THREADS) k_xpsnr_blocks(TmXpsnrGeom g, const TmXpsnrDesc *__restrict__ desc,
                                                             const unsigned short *__restrict__ hin1, const unsigned short *__restrict__ hin2,
                                                             unsigned short *__restrict__ hout1, unsigned short *__restrict__ hout2,
                                                             unsigned long long *__restrict__ BLK)
{
    using namespace tmx;
    __shared__ unsigned short tile[TMX_TILE_H * TMX_TILE_W];
    __shared__ unsigned long long red[TMX_THREADS / 64][5];
    const int tid = threadIdx.x, blk = blockIdx.x, s = blockIdx.y;
    const int bxi = blk % g.wblk, byi = blk / g.wblk;
    const int x0 = bxi * g.b, y0 = byi * g.b;
    const int bw = min(g.b, g.w - x0), bh = min(g.b, g.h - y0);
    const int bval = g.bval;
    // active window of the spatial activity (relative to the block origin)
    const int xa = x0 > 0 ? 0 : bval, ya = y0 > 0 ? 0 : bval;
    const int wa = x0 + bw < g.w ? bw : bw - bval, ha = y0 + bh < g.h ? bh : bh - bval;

    const TmXpsnrDesc &dr = desc[2 * s], &dd = desc[2 * s + 1];
    const Src ref = {(const char *)dr.p0, dr.pitch, g.fmt_y, dr.vec};
    const Src dis = {(const char *)dd.p0, dd.pitch, g.fmt_y, dd.vec};
    const Src hist1 = {(const char *)hin1, g.hpitch * 2, TMX_F_HIST, 1}, hist2 = {(const char *)hin2, g.hpitch * 2, TMX_F_HIST, 1};
    Src m1 = hist1, m2 = hist2;
    if (s >= 1) { const TmXpsnrDesc &p = desc[2 * (s - 1)]; m1 = {(const char *)p.p0, p.pitch, g.fmt_y, p.vec}; }
    if (s >= 2) { const TmXpsnrDesc &p = desc[2 * (s - 2)]; m2 = {(const char *)p.p0, p.pitch, g.fmt_y, p.vec}; }
    else if (s == 1) m2 = hist1;
    // the next launch's history: m1 <- this launch's last reference, m2 <- the one before it (or this launch's first m1)
    unsigned short *const w_o1 = s == g.n - 1 ? hout1 : nullptr;
    unsigned short *const w_o2 = s == g.n - 2 ? hout2 : nullptr;
    unsigned short *const w_m1 = g.n == 1 ? hout2 : nullptr;
    const int sh = g.shift;
    const unsigned mk = g.mask;

    unsigned long long acc[5] = {0, 0, 0, 0, 0}; // sse_y, sse_cb, sse_cr, sa, ta / gamma
    for (int b0 = 0; b0 < bh; b0 += TMX_BAND) {
        const int nb = min(TMX_BAND, bh - b0);
        // ---- stage rows b0-2 .. b0+nb+1, columns x0-4 .. x0+bw+3 of the reference luma (0 outside the picture: never read)
        const int ngx = (bw + 8 + 3) / 4, nrow = nb + 2 * TMX_HALO;
        for (int it = tid; it < ngx * nrow; it += TMX_THREADS) {
            const int r = it / ngx, gx = it - r * ngx;
            const int yy = y0 + b0 - TMX_HALO + r, xx = x0 - 4 + 4 * gx;
            unsigned v[4] = {0, 0, 0, 0};
            if (yy >= 0 && yy < g.h && xx >= 0) load4(ref, xx, yy, g.w, sh, mk, v);
#pragma unroll
            for (int k = 0; k < 4; ++k) tile[r * TMX_TILE_W + 4 * gx + k] = (unsigned short)v[k];
        }
        __syncthreads();
        // T(x, y): reference luma at block-relative (x, y) of this band
#define T(xr, yr) ((int)tile[((yr) - b0 + TMX_HALO) * TMX_TILE_W + (xr) + 4])
        const int ngc = (bw + 3) / 4;
        if (bval == 1) {
            for (int it = tid; it < ngc * nb; it += TMX_THREADS) {
                const int y = b0 + it / ngc, x = 4 * (it % ngc);
                unsigned d[4], h1[4], h2[4] = {0, 0, 0, 0};
                load4(dis, x0 + x, y0 + y, g.w, sh, mk, d);
                load4(m1, x0 + x, y0 + y, g.w, sh, mk, h1);
                if (g.second_order) load4(m2, x0 + x, y0 + y, g.w, sh, mk, h2);
                const bool rowact = y >= ya && y < ha;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int xx = x + k;
                    if (xx >= bw) break;
                    const int o = T(xx, y);
                    const int e = o - (int)d[k];
                    acc[0] += (unsigned long long)(e * (long long)e);
                    acc[4] += g.second_order ? absdiff(o - 2 * (int)h1[k] + (int)h2[k]) : absdiff(o - (int)h1[k]);
                    if (rowact && xx >= xa && xx < wa) {
                        // tests/xpsnr_ref.py sa_hp1: 12 o - 2 (4 direct neighbours) - (4 diagonal neighbours)
                        const int f = 12 * o - 2 * (T(xx - 1, y) + T(xx + 1, y) + T(xx, y - 1) + T(xx, y + 1))
                                    - (T(xx - 1, y - 1) + T(xx + 1, y - 1) + T(xx - 1, y + 1) + T(xx + 1, y + 1));
                        acc[3] += absdiff(f);
                    }
                    const size_t hi = (size_t)(y0 + y) * g.hpitch + x0 + xx;
                    if (w_o1) w_o1[hi] = (unsigned short)o;
                    if (w_o2) w_o2[hi] = (unsigned short)o;
                    if (w_m1) w_m1[hi] = (unsigned short)h1[k];
                }
            }
        } else { // bval == 2: w, h even, so bw, bh, nb are even; a lane takes rows y, y+1 and the two 2x2 cells at x, x+2
            for (int it = tid; it < ngc * (nb / 2); it += TMX_THREADS) {
                const int y = b0 + 2 * (it / ngc), x = 4 * (it % ngc);
                unsigned d[2][4], h1[2][4], h2[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    load4(dis, x0 + x, y0 + y + j, g.w, sh, mk, d[j]);
                    load4(m1, x0 + x, y0 + y + j, g.w, sh, mk, h1[j]);
                    if (g.second_order) load4(m2, x0 + x, y0 + y + j, g.w, sh, mk, h2[j]);
                }
                const bool rowact = y >= ya && y < ha;
#pragma unroll
                for (int c = 0; c < 4; c += 2) {
                    const int xx = x + c;
                    if (xx >= bw) break;
                    int so = 0, s1 = 0, s2 = 0;
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int k = 0; k < 2; ++k) {
                            const int o = T(xx + k, y + j);
                            const int e = o - (int)d[j][c + k];
                            acc[0] += (unsigned long long)(e * (long long)e);
                            so += o; s1 += (int)h1[j][c + k]; s2 += (int)h2[j][c + k];
                            const size_t hi = (size_t)(y0 + y + j) * g.hpitch + x0 + xx + k;
                            if (w_o1) w_o1[hi] = (unsigned short)o;
                            if (w_o2) w_o2[hi] = (unsigned short)o;
                            if (w_m1) w_m1[hi] = (unsigned short)h1[j][c + k];
                        }
                    acc[4] += g.second_order ? absdiff(so - 2 * s1 + s2) : absdiff(so - s1);
                    if (rowact && xx >= xa && xx < wa) {
                        // ffmpeg's `highds` taps; tests/xpsnr_ref.py sa_hp2 states the same sum
                        const int f = 12 * (T(xx, y) + T(xx + 1, y) + T(xx, y + 1) + T(xx + 1, y + 1))
                                    - 3 * (T(xx - 1, y) + T(xx + 2, y) + T(xx - 1, y + 1) + T(xx + 2, y + 1))
                                    - 3 * (T(xx, y - 1) + T(xx + 1, y - 1) + T(xx, y + 2) + T(xx + 1, y + 2))
                                    - 2 * (T(xx - 1, y - 1) + T(xx + 2, y - 1) + T(xx - 1, y + 2) + T(xx + 2, y + 2))
                                    - (T(xx - 1, y - 2) + T(xx, y - 2) + T(xx + 1, y - 2) + T(xx + 2, y - 2)
                                     + T(xx - 1, y + 3) + T(xx, y + 3) + T(xx + 1, y + 3) + T(xx + 2, y + 3)
                                     + T(xx - 2, y - 1) + T(xx - 2, y) + T(xx - 2, y + 1) + T(xx - 2, y + 2)
                                     + T(xx + 3, y - 1) + T(xx + 3, y) + T(xx + 3, y + 1) + T(xx + 3, y + 2));
                        acc[3] += absdiff(f);
                    }
                }
            }
        }
#undef T
        __syncthreads(); // the next band overwrites the tile
    }

    // ---- chroma: block (bxi, byi) of the chroma grid
    {
        const int cx0 = bxi * g.bx, cy0 = byi * g.by;
        const int cbw = min(g.bx, g.cw - cx0), cbh = min(g.by, g.ch - cy0);
        // groups of 4 start at a multiple of 4 (the loaders' contract: aligned wide loads, no packed 10-bit group across two runs);
        // the columns of the group left of cx0 belong to the previous block and are skipped
        const int cxa = cx0 & ~3;
        const int ngc = (cx0 + cbw - cxa + 3) / 4;
        for (int it = tid; it < ngc * cbh; it += TMX_THREADS) {
            const int cy = cy0 + it / ngc, cx = cxa + 4 * (it % ngc);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                unsigned r[4], d[4];
                if (g.biplanar) {
                    load4_cbcr({(const char *)dr.p1, dr.pitch2, g.fmt_c, dr.vec}, c, cx, cy, cx0 + cbw, sh, r);
                    load4_cbcr({(const char *)dd.p1, dd.pitch2, g.fmt_c, dd.vec}, c, cx, cy, cx0 + cbw, sh, d);
                } else {
                    load4({(const char *)(c ? dr.p2 : dr.p1), dr.pitch2, g.fmt_c, dr.vec}, cx, cy, cx0 + cbw, sh, mk, r);
                    load4({(const char *)(c ? dd.p2 : dd.p1), dd.pitch2, g.fmt_c, dd.vec}, cx, cy, cx0 + cbw, sh, mk, d);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int e = cx + k < cx0 ? 0 : (int)r[k] - (int)d[k]; // 0 - 0 past the block's last column
                    acc[1 + c] += (unsigned long long)(e * (long long)e);
                }
            }
        }
    }

    if (tm_xpsnr_wave_sum5(acc)) {
#pragma unroll
        for (int k = 0; k < 5; ++k) red[tid >> 6][k] = acc[k];
    }
    __syncthreads();
    if (tid < 5) {
        unsigned long long t = 0;
        for (int wv = 0; wv < TMX_THREADS / 64; ++wv) t += red[wv][tid];
        BLK[((size_t)s * g.nblk + blk) * 5 + tid] = t;
    }
}

// one lane per slot: weights, smoothing, weighted sums (tests/xpsnr_ref.py frame_wsse, statement for statement)
__global__ void __launch_bounds__(64) k_xpsnr_finish(TmXpsnrGeom g, const unsigned long long *__restrict__ BLK, double *__restrict__ WGT,
                                                      unsigned long long *__restrict__ RES)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= g.n) return;
    const unsigned long long *bs = BLK + (size_t)s * g.nblk * 5;
    unsigned long long *res = RES + (size_t)s * 3;
    if (g.small) { // b < 4: plain SSE per component
        unsigned long long t[3] = {0, 0, 0};
        for (int i = 0; i < g.nblk; ++i)
            for (int c = 0; c < 3; ++c) t[c] += bs[i * 5 + c];
        for (int c = 0; c < 3; ++c) res[c] = t[c];
        return;
    }
    double *w = WGT + (size_t)s * g.nblk;
    const int b = g.b, bval = g.bval;
    for (int i = 0; i < g.nblk; ++i) {
        const int x0 = (i % g.wblk) * b, y0 = (i / g.wblk) * b;
        const int bw = min(b, g.w - x0), bh = min(b, g.h - y0);
        const int xa = x0 > 0 ? 0 : bval, ya = y0 > 0 ? 0 : bval;
        const int wa = x0 + bw < g.w ? bw : bw - bval, ha = y0 + bh < g.h ? bh : bh - bval;
        double ms = 1.0;
        if (!(wa <= xa || ha <= ya)) {
            const double sa = (double)bs[i * 5 + 3], ta = 2.0 * (double)bs[i * 5 + 4]; // gamma = 2
            ms = sa / ((double)(wa - xa) * (double)(ha - ya)) + ta / ((double)bw * (double)bh);
            ms = ms > g.min_act ? ms : g.min_act;
            ms = ms * ms;
        }
        w[i] = 1.0 / sqrt(ms);
        if (g.smooth) { // ffmpeg's in-line minimum smoothing
            double prev = x0 == 0 ? (i > 1 ? w[i - 2] : 0.0) : (x0 > b ? fmax(w[i - 2], w[i]) : w[i]);
            if (i > g.wblk) prev = fmax(prev, w[i - 1 - g.wblk]);
            if (i > 0 && w[i - 1] > prev) w[i - 1] = prev;
            if (i == g.nblk - 1 && i > g.wblk) {
                prev = fmax(w[i - 1], w[i - g.wblk]);
                if (w[i] > prev) w[i] = prev;
            }
        }
    }
    for (int c = 0; c < 3; ++c) {
        double t = 0.0;
        for (int i = 0; i < g.nblk; ++i) t += (double)bs[i * 5 + c] * w[i];
        res[c] = t <= 0.0 ? 0ull : (unsigned long long)(t * g.avg_act + 0.5);
    }
}
