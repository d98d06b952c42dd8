// tm_yuv_kernels.h -- gfx950 kernels of plane-wise YUV PSNR and SSIM (libturbometrics_yuv.so, include/turbo_metrics_yuv.h).
//
// The definition is DESIGN.md section 15; its literal CPU restatement is tests/yuv_ref.py.  Per plane of a 4:2:0 pair: the sum of
// squared differences over every sample (uint64, exact), and the x264 / ffmpeg SSIM: 4x4 block sums s1, s2, ss, s12, one f32 value
// per window of 2x2 blocks, the f64 sum of the values.  Integer arithmetic up to the one f32 expression per window.
//
//   k_yuv<LAYOUT, FMT>   grid (tiles over the three planes, slots)   block 256   one workgroup per tile of TMY_T x TMY_T windows of one
//                   plane of one slot's pair -- of BOTH chroma planes at once where they are interleaved (NV12, P016), so that the
//                   CbCr plane leaves memory once.  A tile needs (TMY_T + 1)^2 blocks: lane (bx, by) owns block (bx, by) of the
//                   tile, lanes 0 .. 2 TMY_T own the one-block halo on the right and below as well.  A block is four row loads of
//                   four samples per side (tmx::load4_raw: 4, 8 or 16 bytes), all issued before the first is unpacked.  The block
//                   sums go to LDS; lane (bx, by) then evaluates window (bx, by) from its four blocks and writes the value to the
//                   map with a plain vector store.
//                   SSE comes from the same samples: ss - 2 s12 per block.  A block counts in the tile that owns it; the halo
//                   blocks count in the last tile of their direction only (no other tile owns them), and so do the samples beyond
//                   the last full block, which that tile reads one by one.  Every sample counts in exactly one tile.
//                   The lanes' SSE (u64) and f64 window sums meet in a fixed two-level LDS tree (16 x 16) and go to the tile's OWN
//                   cell with plain stores.
//   k_yuv_finish    grid (slots)   block 256   per plane: lane i adds cells i, i + 256, ... in order, then the same tree.
//
// No atomics; every cell and every map value is written by every compute, so nothing is zeroed and nothing is kept between
// computes: two computes of the same input return the same bytes.
#pragma once
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::sample1 / load4_raw / unpack4: the loaders of the XPSNR and motion kernels

#define TMY_THREADS 256
#define TMY_T 16              /* windows per tile edge */
#define TMY_B (TMY_T + 1)     /* blocks per tile edge, halo included */
#define TMY_MAX_DIM 32768u    /* largest w, h: keeps every byte offset inside a row in an int */

// layouts of include/turbo_metrics_yuv.h (XPSNR's numbering)
enum { TMY_NV12 = 0, TMY_P016 = 1, TMY_I420 = 2, TMY_I420P10 = 3 };

// one picture of a slot
struct TmYuvDesc {
    const void *p0, *p1, *p2;          // Y, Cb (or CbCr), Cr (or null)
    unsigned long long pitch, pitch2;  // bytes per luma / chroma row
    int vec;                           // bases and pitches 16-byte aligned: the wide loads are allowed
    int pad_;
};

// what a tile leaves: its SSE and the f64 sum of its windows
struct TmYuvCell {
    unsigned long long sse;
    double ssim;
};

// one slot's result: per plane the SSE and the f64 sum of the window values
struct TmYuvRes {
    unsigned long long sse[3];
    double ssim_sum[3];
};

struct TmYuvGeom {
    unsigned w, h;
    int bits, layout;
    int fmt;             // TMX_F_* of the samples
    int shift;           // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;       // TMX_F_U16_LOW: sample = v & mask
    long long c1, c2;
    // [0]: luma, [1]: either chroma plane
    unsigned pw[2], ph[2];   // samples
    unsigned bw[2], bh[2];   // 4x4 blocks
    unsigned tx[2], ty[2];   // tiles
    unsigned tiles[2];       // tx * ty
    unsigned cells;          // per slot: tiles[0] + 2 tiles[1]; plane 0 first, then plane 1, then plane 2
    unsigned grid;           // workgroups per slot: tiles[0] + tiles[1] (interleaved chroma) or the cells
    unsigned long long map_off[3], map_floats; // floats: where a plane's map starts in a slot's maps; per slot
};

static inline long long tmy_c1(unsigned bits)
{
    const double mx = (double)((1u << bits) - 1u);
    return (long long)(.01 * .01 * mx * mx * 64 + .5);
}
static inline long long tmy_c2(unsigned bits)
{
    const double mx = (double)((1u << bits) - 1u);
    return (long long)(.03 * .03 * mx * mx * 64 * 63 + .5);
}

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 16 (a chroma plane needs one window) or above
// TMY_MAX_DIM, D outside 8 .. 16 or not one the layout carries
static inline int tmy_make_geom(TmYuvGeom *g, unsigned w, unsigned h, int layout, unsigned bits)
{
    memset(g, 0, sizeof *g);
    if (w < 16 || h < 16 || w > TMY_MAX_DIM || h > TMY_MAX_DIM || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMY_NV12: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMY_P016: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMY_I420: g->fmt = bits == 8 ? TMX_F_U8 : TMX_F_U16_LOW; break;
    case TMY_I420P10: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->w = w; g->h = h; g->bits = (int)bits; g->layout = layout;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->c1 = tmy_c1(bits); g->c2 = tmy_c2(bits);
    for (int c = 0; c < 2; ++c) {
        g->pw[c] = c ? (w + 1) / 2 : w; g->ph[c] = c ? (h + 1) / 2 : h;
        g->bw[c] = g->pw[c] >> 2; g->bh[c] = g->ph[c] >> 2;
        g->tx[c] = (g->bw[c] - 1 + TMY_T - 1) / TMY_T; g->ty[c] = (g->bh[c] - 1 + TMY_T - 1) / TMY_T;
        g->tiles[c] = g->tx[c] * g->ty[c];
    }
    g->cells = g->tiles[0] + 2 * g->tiles[1];
    g->grid = layout == TMY_NV12 || layout == TMY_P016 ? g->tiles[0] + g->tiles[1] : g->cells;
    g->map_off[0] = 0;
    g->map_off[1] = (unsigned long long)(g->bw[0] - 1) * (g->bh[0] - 1);
    g->map_off[2] = g->map_off[1] + (unsigned long long)(g->bw[1] - 1) * (g->bh[1] - 1);
    g->map_floats = g->map_off[2] + (unsigned long long)(g->bw[1] - 1) * (g->bh[1] - 1);
    return 0;
}

namespace tmy {

// the block sums of a tile in LDS: [plane of the tile][block row][block column]
struct Blocks {
    unsigned s1[2][TMY_B][TMY_B], s2[2][TMY_B][TMY_B];
    unsigned long long ss[2][TMY_B][TMY_B], s12[2][TMY_B][TMY_B];
};

// the two-level tree: 256 values -> 16 sums of 16 neighbours -> their sum, each level added in index order.  Lane 0 holds the
// total.  All lanes of the workgroup call it.
struct Tree {
    unsigned long long sse[TMY_THREADS];
    double ssim[TMY_THREADS];
};
__device__ __forceinline__ void tree_sum(Tree &t, unsigned tid, unsigned long long &sse, double &ssim)
{
    t.sse[tid] = sse; t.ssim[tid] = ssim;
    TM_LDS_BARRIER();
    if (tid < 16) {
        unsigned long long a = 0;
        double b = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { a += t.sse[tid * 16 + k]; b += t.ssim[tid * 16 + k]; }
        sse = a; ssim = b;
    }
    TM_LDS_BARRIER();
    if (tid < 16) { t.sse[tid] = sse; t.ssim[tid] = ssim; }
    TM_LDS_BARRIER();
    if (tid == 0) {
        unsigned long long a = 0;
        double b = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) { a += t.sse[k]; b += t.ssim[k]; }
        sse = a; ssim = b;
    }
}

// sums of one 4x4 block from its 16 sample pairs
struct Sums {
    unsigned s1, s2;
    unsigned long long ss, s12;
};
__device__ __forceinline__ void add_row(Sums &s, const unsigned (&a)[4], const unsigned (&b)[4], int first, int step)
{
#pragma unroll
    for (int k = first; k < 4; k += step) {
        s.s1 += a[k]; s.s2 += b[k];
        // samples are below 2^16: the 24-bit multiply gives the whole product
        s.ss += (unsigned long long)tm_mul24(a[k], a[k]) + (unsigned long long)tm_mul24(b[k], b[k]);
        s.s12 += (unsigned long long)tm_mul24(a[k], b[k]);
    }
}

// Block (gbx, gby) of a plane of both pictures -> out[0] (and out[1]: the second plane of an interleaved pair, NP == 2).
// pa, pb: the plane's (or the interleaved planes') base in the two pictures.
template <int FMT, int NP>
__device__ __forceinline__ void block_sums(const char *pa, unsigned long long pitch_a, const char *pb, unsigned long long pitch_b, bool vec,
                                           unsigned gbx, unsigned gby, int shift, unsigned mask, Sums (&out)[NP])
{
#pragma unroll
    for (int c = 0; c < NP; ++c) out[c] = Sums{0u, 0u, 0ull, 0ull};
    const int x0 = (int)(4u * NP * gbx); // the block's first element of a row
    const char *ra = pa + (size_t)(4u * gby) * pitch_a, *rb = pb + (size_t)(4u * gby) * pitch_b;
    if (vec) {
        tmx::Raw4 qa[4][NP], qb[4][NP];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                qa[r][j] = tmx::load4_raw(ra + (size_t)r * pitch_a, FMT, x0 + 4 * j);
                qb[r][j] = tmx::load4_raw(rb + (size_t)r * pitch_b, FMT, x0 + 4 * j);
            }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                unsigned a[4], b[4];
                tmx::unpack4(qa[r][j], FMT, x0 + 4 * j, shift, mask, a);
                tmx::unpack4(qb[r][j], FMT, x0 + 4 * j, shift, mask, b);
                if (NP == 1) add_row(out[0], a, b, 0, 1);
                else { add_row(out[0], a, b, 0, 2); add_row(out[NP - 1], a, b, 1, 2); } // Cb at the even, Cr at the odd elements
            }
    } else { // an unaligned picture: sample by sample
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                unsigned a[4], b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = tmx::sample1(ra + (size_t)r * pitch_a, FMT, x0 + 4 * j + k, shift, mask);
                    b[k] = tmx::sample1(rb + (size_t)r * pitch_b, FMT, x0 + 4 * j + k, shift, mask);
                }
                if (NP == 1) add_row(out[0], a, b, 0, 1);
                else { add_row(out[0], a, b, 0, 2); add_row(out[NP - 1], a, b, 1, 2); }
            }
    }
}

// one window from the sums over its four blocks
__device__ __forceinline__ float window(long long s1, long long s2, long long ss, long long s12, long long c1, long long c2)
{
    const long long vars = ss * 64 - s1 * s1 - s2 * s2;
    const long long covar = s12 * 64 - s1 * s2;
    const float n1 = (float)(2 * s1 * s2 + c1), n2 = (float)(2 * covar + c2);
    const float d1 = (float)(s1 * s1 + s2 * s2 + c1), d2 = (float)(vars + c2);
    const float num = n1 * n2, den = d1 * d2;
    return num / den;
}

// One tile of NP planes that share their sample rows (NP == 2: interleaved CbCr).  c: 0 luma geometry, 1 chroma geometry;
// plane: the first plane's number; t: the tile's number in the plane.
template <int FMT, int NP>
__device__ __forceinline__ void tile(const TmYuvGeom &g, int c, int plane, unsigned t, const char *pa, unsigned long long pitch_a, const char *pb,
                                     unsigned long long pitch_b, bool vec, float *maps, TmYuvCell *cells, Blocks &blk, Tree &tree)
{
    const unsigned tid = threadIdx.x;
    const unsigned pw = g.pw[c], ph = g.ph[c], bw = g.bw[c], bh = g.bh[c];
    const unsigned tx = t % g.tx[c], ty = t / g.tx[c];
    const bool last_x = tx + 1 == g.tx[c], last_y = ty + 1 == g.ty[c];
    const unsigned bx0 = tx * TMY_T, by0 = ty * TMY_T;
    unsigned long long sse[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) sse[j] = 0;

    // ---- block sums: pass 0 the lane's own block, pass 1 the halo (lanes 0 .. 2 TMY_T)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        unsigned lx, ly;
        bool counts;
        if (pass == 0) { lx = tid % TMY_T; ly = tid / TMY_T; counts = true; }
        else if (tid < TMY_T) { lx = TMY_T; ly = tid; counts = last_x; }
        else if (tid < 2 * TMY_T) { lx = tid - TMY_T; ly = TMY_T; counts = last_y; }
        else if (tid == 2 * TMY_T) { lx = TMY_T; ly = TMY_T; counts = last_x && last_y; }
        else break;
        const unsigned gbx = bx0 + lx, gby = by0 + ly;
        if (gbx >= bw || gby >= bh) continue;
        Sums s[NP];
        block_sums<FMT, NP>(pa, pitch_a, pb, pitch_b, vec, gbx, gby, g.shift, g.mask, s);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            blk.s1[j][ly][lx] = s[j].s1; blk.s2[j][ly][lx] = s[j].s2; blk.ss[j][ly][lx] = s[j].ss; blk.s12[j][ly][lx] = s[j].s12;
            if (counts) sse[j] += s[j].ss - 2 * s[j].s12;
        }
    }
    // ---- the samples beyond the last full block: columns [4 bw, pw) in the last tile of a row of tiles, rows [4 bh, ph) in the
    // last tile of a column (the corner belongs to the columns)
    {
        const unsigned y0 = 4 * by0, y1 = last_y ? ph : y0 + 4 * TMY_T, x0 = 4 * bx0, x1 = last_x ? 4 * bw : x0 + 4 * TMY_T;
        const unsigned rc = last_x ? pw - 4 * bw : 0u, rr = last_y ? ph - 4 * bh : 0u;
        const unsigned n_col = rc * (y1 - y0), n_row = rr * (x1 - x0);
        for (unsigned i = tid; i < n_col + n_row; i += TMY_THREADS) {
            unsigned x, y;
            if (i < n_col) { x = 4 * bw + i % rc; y = y0 + i / rc; }
            else { x = x0 + (i - n_col) % (x1 - x0); y = 4 * bh + (i - n_col) / (x1 - x0); }
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const unsigned a = tmx::sample1(pa + (size_t)y * pitch_a, FMT, (int)(NP * x + j), g.shift, g.mask);
                const unsigned b = tmx::sample1(pb + (size_t)y * pitch_b, FMT, (int)(NP * x + j), g.shift, g.mask);
                const unsigned d = a > b ? a - b : b - a;
                sse[j] += (unsigned long long)tm_mul24(d, d);
            }
        }
    }
    TM_LDS_BARRIER();

    // ---- windows
    const unsigned lx = tid % TMY_T, ly = tid / TMY_T;
    const unsigned gwx = bx0 + lx, gwy = by0 + ly;
    const bool has = gwx + 1 < bw && gwy + 1 < bh;
    const unsigned mw = bw - 1;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        double v64 = 0.0;
        if (has) {
            long long s1 = 0, s2 = 0, ss = 0, s12 = 0;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    s1 += blk.s1[j][ly + dy][lx + dx]; s2 += blk.s2[j][ly + dy][lx + dx];
                    ss += (long long)blk.ss[j][ly + dy][lx + dx]; s12 += (long long)blk.s12[j][ly + dy][lx + dx];
                }
            const float v = window(s1, s2, ss, s12, g.c1, g.c2);
            maps[g.map_off[plane + j] + (size_t)gwy * mw + gwx] = v;
            v64 = (double)v;
        }
        tree_sum(tree, tid, sse[j], v64);
        if (tid == 0) {
            TmYuvCell cell;
            cell.sse = sse[j]; cell.ssim = v64;
            cells[(plane + j == 0 ? 0u : (plane + j == 1 ? g.tiles[0] : g.tiles[0] + g.tiles[1])) + t] = cell;
        }
        // the next plane's tree starts with a barrier after its first stores, which only follow this lane-0 read in program order
        TM_LDS_BARRIER();
    }
}

} // namespace tmy

// desc: [slot][side]; maps: [slot][g.map_floats]; cells: [slot][g.cells].  FMT: the TMX_F_* the layout's samples have at this depth
// (I420: bytes at D = 8, else 16-bit words): five instantiations, the host picks one.
template <int LAYOUT, int FMT>
__global__ void __launch_bounds__(TMY_THREADS) k_yuv(TmYuvGeom g, const TmYuvDesc *__restrict__ desc, float *__restrict__ maps, TmYuvCell *__restrict__ cells)
{
    using namespace tmy;
    __shared__ Blocks blk;
    __shared__ Tree tree;
    constexpr bool BI = LAYOUT == TMY_NV12 || LAYOUT == TMY_P016;
    const unsigned slot = blockIdx.y;
    unsigned t = blockIdx.x;
    const TmYuvDesc da = desc[2 * slot], db = desc[2 * slot + 1];
    const bool vec = da.vec && db.vec;
    float *m = maps + (size_t)slot * g.map_floats;
    TmYuvCell *cl = cells + (size_t)slot * g.cells;
    if (t < g.tiles[0]) {
        tile<FMT, 1>(g, 0, 0, t, (const char *)da.p0, da.pitch, (const char *)db.p0, db.pitch, vec, m, cl, blk, tree);
    } else if (BI) { // both chroma planes from the one interleaved plane
        tile<FMT, 2>(g, 1, 1, t - g.tiles[0], (const char *)da.p1, da.pitch2, (const char *)db.p1, db.pitch2, vec, m, cl, blk, tree);
    } else {
        t -= g.tiles[0];
        const bool cr = t >= g.tiles[1];
        if (cr) t -= g.tiles[1];
        tile<FMT, 1>(g, 1, cr ? 2 : 1, t, (const char *)(cr ? da.p2 : da.p1), da.pitch2, (const char *)(cr ? db.p2 : db.p1), db.pitch2, vec, m, cl, blk, tree);
    }
}

// the launch of the instantiation for g.layout / g.fmt: the one place that maps a geometry to a kernel (library and emulation)
#define TMY_DISPATCH(g, LAUNCH)                                                   \
    do {                                                                          \
        switch ((g).layout) {                                                     \
        case TMY_NV12: LAUNCH(TMY_NV12, TMX_F_U8); break;                         \
        case TMY_P016: LAUNCH(TMY_P016, TMX_F_U16_MSB); break;                    \
        case TMY_I420:                                                            \
            if ((g).fmt == TMX_F_U8) LAUNCH(TMY_I420, TMX_F_U8);                  \
            else LAUNCH(TMY_I420, TMX_F_U16_LOW);                                 \
            break;                                                                \
        default: LAUNCH(TMY_I420P10, TMX_F_P10); break;                           \
        }                                                                         \
    } while (0)

// grid (slots), block 256: per plane the sum of the slot's cells in a fixed order
__global__ void __launch_bounds__(TMY_THREADS) k_yuv_finish(TmYuvGeom g, const TmYuvCell *__restrict__ cells, TmYuvRes *__restrict__ res)
{
    __shared__ tmy::Tree tree;
    const unsigned tid = threadIdx.x, slot = blockIdx.x;
    const TmYuvCell *cl = cells + (size_t)slot * g.cells;
    for (int p = 0; p < 3; ++p) {
        const unsigned n = g.tiles[p != 0];
        unsigned long long sse = 0;
        double ssim = 0.0;
        for (unsigned i = tid; i < n; i += TMY_THREADS) { sse += cl[i].sse; ssim += cl[i].ssim; }
        tmy::tree_sum(tree, tid, sse, ssim);
        if (tid == 0) { res[slot].sse[p] = sse; res[slot].ssim_sum[p] = ssim; }
        TM_LDS_BARRIER();
        cl += n;
    }
}
