// tm_scene_kernels.h -- gfx950 kernels of the scene-cut histogram (libturbometrics_scene.so, include/turbo_metrics_scene.h).
//
// The definition is DESIGN.md section 12; its literal CPU restatement is tests/scene_ref.py.  Per picture: hist[b] = the number of
// luma samples with sample >> (D - 8) == b, b = 0 .. 255, uint32.  Integer only; no floating point on the device.
//
//   k_scene_hist<FMT>   grid (row bands, slots)   block 256   one workgroup per band of g.band_rows rows of one slot's picture.
//                       A lane reads 4-aligned groups of 4 samples (tmx::load4_raw: every sample leaves memory once), TMS_ROWS rows
//                       of one group column at a time so that TMS_ROWS loads are in flight per lane, and counts them into LDS with
//                       integer LDS atomics.  Samples at or beyond w in a row's last group are NOT counted.
//                       The workgroup holds TMS_SUBS = 32 private sub-histograms: TMS_REPL = 8 per wave, chosen by lane & 7, stored
//                       bin-major (word bin * 32 + sub), so that the 8 sub-histograms of a wave's lanes lie in 8 different banks.  A
//                       lane first folds equal neighbours of its four samples into one add.  On a flat picture -- every lane of
//                       every wave on ONE bin -- a wave instruction is then ONE add per lane, 8 lanes per address on 8 banks,
//                       instead of four adds of 64 lanes on one address.
//                       Leaving the workgroup: lane b sums bin b over the 32 sub-histograms (rotated, so that the lanes read
//                       different banks) and writes it to the workgroup's own cell of 256 uint32 with a plain vector store.
//   k_scene_finish      grid (slots)   block 256   lane b adds bin b of the slot's cells in band order.  Every cell is written by
//                       every compute, so nothing is zeroed and nothing is kept between computes.
//
// Integer adds are exact in any order: the result does not depend on how the lanes' atomics arrive.
#pragma once
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::sample1 / load4_raw / unpack4: the loaders of the XPSNR and motion kernels

#define TMS_THREADS 256
#define TMS_BINS 256
#define TMS_REPL 8                                 /* sub-histograms per wave */
#define TMS_SUBS (TMS_REPL * (TMS_THREADS / 64))   /* per workgroup: 32 */
#define TMS_ROWS 8                                 /* rows of one group column a lane has in flight */
#define TMS_BAND_SAMPLES 65536u                    /* samples per band, about */
#define TMS_BAND_ROWS_MAX 128u

// layouts of include/turbo_metrics_scene.h (motion's numbering)
enum { TMS_Y8 = 0, TMS_Y16_MSB = 1, TMS_Y16_LOW = 2, TMS_Y10_PACKED = 3 };

// one picture of a slot
struct TmSceneDesc {
    const void *p;
    unsigned long long pitch; // bytes
    int vec;                  // base and pitch 16-byte aligned: the wide loads are allowed
    int pad_;
};

struct TmSceneGeom {
    unsigned w, h;
    int bits;       // D
    int fmt;        // TMX_F_* of the luma samples
    int shift;      // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;  // TMX_F_U16_LOW: sample = v & mask
    int hshift;     // bin = sample >> hshift: D - 8
    unsigned groups;    // 4-sample groups per row
    unsigned band_rows; // rows per workgroup
    unsigned bands;     // workgroups per picture
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h of 0, w h above 2^31, D outside 8 .. 16 or not one the layout
// carries
static inline int tms_make_geom(TmSceneGeom *g, unsigned w, unsigned h, int layout, unsigned bits)
{
    memset(g, 0, sizeof *g);
    if (w == 0 || h == 0 || (unsigned long long)w * h > (1ull << 31) || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMS_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMS_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMS_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMS_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->w = w; g->h = h; g->bits = (int)bits;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->hshift = (int)bits - 8;
    g->groups = (unsigned)(((unsigned long long)w + 3) / 4);
    unsigned br = TMS_BAND_SAMPLES / w;
    br = br < 1u ? 1u : (br > TMS_BAND_ROWS_MAX ? TMS_BAND_ROWS_MAX : br);
    g->band_rows = br;
    g->bands = (h + br - 1) / br;
    return 0;
}

namespace tms {

struct alignas(16) Word4 { unsigned a, b, c, d; };

// where the loaders find sample x of a row, as a pointer and a small column: tmx's loaders take int columns and multiply them by the
// sample size, which a row of 2^30 samples and more would overflow
template <int FMT>
__device__ __forceinline__ const char *group_base(const char *row, unsigned x, int &xl)
{
    if (FMT == TMX_F_P10) { xl = (int)(x % TM_P10_BLOCK); return row + (size_t)(x / TM_P10_BLOCK) * (TM_P10_RUN * 4u); }
    xl = 0;
    return row + (size_t)x * (FMT == TMX_F_U8 ? 1u : 2u);
}

// `n` (1 .. 4) samples of one group into the lane's sub-histogram: equal neighbours are one add.  The loaders hand out samples below
// 2^D, so a bin is below 256; the mask keeps a wrong sample inside the sub-histogram (a wrong count, never a write outside LDS)
__device__ __forceinline__ void count4(unsigned *sub, const unsigned (&v)[4], int n, int hshift)
{
    unsigned cur = (v[0] >> hshift) & (TMS_BINS - 1), c = 1;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        if (k >= n) break;
        const unsigned b = (v[k] >> hshift) & (TMS_BINS - 1);
        if (b == cur) { ++c; continue; }
        atomicAdd(&sub[cur * TMS_SUBS], c);
        cur = b; c = 1;
    }
    atomicAdd(&sub[cur * TMS_SUBS], c);
}

} // namespace tms

template <int FMT>
__global__ void __launch_bounds__(TMS_THREADS) k_scene_hist(TmSceneGeom g, const TmSceneDesc *__restrict__ desc, unsigned *__restrict__ cells)
{
    using namespace tms;
    __shared__ Word4 lds4[TMS_BINS * TMS_SUBS / 4]; // word bin * TMS_SUBS + sub
    unsigned *lds = (unsigned *)lds4;
    const unsigned tid = threadIdx.x, band = blockIdx.x, slot = blockIdx.y;
    const TmSceneDesc d = desc[slot];
#pragma unroll
    for (int k = 0; k < TMS_BINS * TMS_SUBS / 4 / TMS_THREADS; ++k) lds4[tid + k * TMS_THREADS] = Word4{0u, 0u, 0u, 0u};
    TM_LDS_BARRIER();

    unsigned *sub = lds + (tid >> 6) * TMS_REPL + (tid & (TMS_REPL - 1));
    const unsigned y0 = band * g.band_rows, y1 = y0 + g.band_rows < g.h ? y0 + g.band_rows : g.h;
    for (unsigned y = y0; y < y1; y += TMS_ROWS) {
        const unsigned rows = y1 - y < TMS_ROWS ? y1 - y : TMS_ROWS;
        for (unsigned gx = tid; gx < g.groups; gx += TMS_THREADS) {
            const unsigned x = 4u * gx;
            const int n = g.w - x < 4u ? (int)(g.w - x) : 4;
            int xl;
            const char *p = group_base<FMT>((const char *)d.p + (size_t)y * d.pitch, x, xl);
            if (d.vec && n == 4) {
                tmx::Raw4 raw[TMS_ROWS];
#pragma unroll
                for (int r = 0; r < TMS_ROWS; ++r)
                    if ((unsigned)r < rows) raw[r] = tmx::load4_raw(p + (size_t)r * d.pitch, FMT, xl);
#pragma unroll
                for (int r = 0; r < TMS_ROWS; ++r) {
                    if ((unsigned)r >= rows) break;
                    unsigned v[4];
                    tmx::unpack4(raw[r], FMT, xl, g.shift, g.mask, v);
                    count4(sub, v, 4, g.hshift);
                }
            } else { // an unaligned picture, or the row's last, partial group: sample by sample, and only the samples inside the row
                for (unsigned r = 0; r < rows; ++r) {
                    unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n) v[k] = tmx::sample1(p + (size_t)r * d.pitch, FMT, xl + k, g.shift, g.mask);
                    count4(sub, v, n, g.hshift);
                }
            }
        }
    }
    TM_LDS_BARRIER();
    // lane b: bin b over the sub-histograms, starting at sub-histogram b so that the lanes of a wave read different banks
    unsigned t = 0;
#pragma unroll
    for (int k = 0; k < TMS_SUBS; ++k) t += lds[tid * TMS_SUBS + ((tid + k) & (TMS_SUBS - 1))];
    cells[((size_t)slot * g.bands + band) * TMS_BINS + tid] = t;
}

// grid (slots), block 256: hist[slot][b] = the sum over the slot's bands, in band order
__global__ void __launch_bounds__(TMS_THREADS) k_scene_finish(unsigned bands, const unsigned *__restrict__ cells, unsigned *__restrict__ hist)
{
    const unsigned tid = threadIdx.x, slot = blockIdx.x;
    const unsigned *c = cells + (size_t)slot * bands * TMS_BINS + tid;
    unsigned t = 0;
    for (unsigned b = 0; b < bands; ++b) t += c[(size_t)b * TMS_BINS];
    hist[(size_t)slot * TMS_BINS + tid] = t;
}
