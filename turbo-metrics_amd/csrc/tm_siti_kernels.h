// tm_siti_kernels.h -- gfx950 kernel of ITU-T P.910 spatial / temporal information (libturbometrics_siti.so, include/turbo_metrics_siti.h).
//
// The definition is DESIGN.md section 19; its literal CPU restatement is tests/siti_ref.py.  Per picture, on the luma code values:
// SI: at the interior positions the 3x3 Sobel pair gx, gy, m2 = gx^2 + gy^2, M = m2 << 2 (16 - D), q = the integer nearest to sqrt(M)
// (q^2 - q < M <= q^2 + q), S1 = sum q, S2 = sum q^2.  TI: d = F_n - F_{n-1} at every position, T1 = sum d, T2 = sum d^2.  Integer only in
// what is summed; the one float instruction (an f32 square root) is an estimate that the integer inequality corrects.
//
//   k_siti<FMT>   grid (luma tiles)   block 256   one workgroup per tile of 120 x 30 samples, walking the launch's slots in sequence
//                 order.  Per slot it stages the tile plus its 1-sample halo in LDS as uint16 (every lane reads 4-aligned groups of 4
//                 samples: one wide load where the group lies inside the row of an aligned picture, sample by sample and only inside
//                 the picture otherwise; rows and columns outside the picture are never fetched and stay 0, no interior position reads
//                 them), computes Sobel, q and the frame difference from LDS, and keeps the raw tile of the previous slot in
//                 registers: a picture leaves memory once per launch for both SI and TI.  The loads of slot s + 1 are issued before
//                 the arithmetic of slot s; the LDS tile is double-buffered, so a slot costs one barrier.  A lane's four sums are
//                 reduced over the wave with shuffles and added to the slot's accumulators by four 64-bit atomics per wave, spread
//                 over TMI_BINS bins; integer addition, so the order of arrival cannot change a bit.
//
// History.  The workgroup of a tile writes the last slot's raw tile to the history plane (uint16) and the same tile's workgroup of
// the next launch reads it for its slot 0.  Tiles are disjoint: nothing else touches those samples, so one plane is enough.  The
// first launch of a sequence (g.first) does not read it: slot 0 has T1 = T2 = 0.
//
// The tile.  LDS rows hold 128 samples: columns x0 - 4 .. x0 + 123, i.e. 32 groups of 4; 32 rows y0 - 1 .. y0 + 30: exactly four
// staging items per lane.  Of those columns Sobel reads x0 - 1 .. x0 + 120.
#pragma once
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::sample1 / load4 / load4_raw / unpack4: the loaders of the XPSNR, motion and scene kernels

#define TMI_THREADS 256
#define TMI_TW 120                               /* output columns per tile */
#define TMI_TH 30                                /* output rows per tile */
#define TMI_NGX ((TMI_TW + 8) / 4)               /* 4-sample groups per staged row: 32 */
#define TMI_SH (TMI_TH + 2)                      /* staged rows: 32 */
#define TMI_STAGE ((TMI_NGX * TMI_SH + TMI_THREADS - 1) / TMI_THREADS)           /* staging items per lane: 4 */
#define TMI_OUT (((TMI_TW / 4) * TMI_TH + TMI_THREADS - 1) / TMI_THREADS)        /* output groups per lane: 4 */
#define TMI_BINS 16                              /* accumulator sets per slot (spreads the atomics) */
#define TMI_SUMS 4                               /* S1, S2, T1 (two's complement), T2 */
#define TMI_MAX_SAMPLES (1ull << 26)             /* w h above this is refused: S2 < 2^37 (w - 2)(h - 2) stays below 2^63 */

// layouts of include/turbo_metrics_siti.h (motion's numbering)
enum { TMI_Y8 = 0, TMI_Y16_MSB = 1, TMI_Y16_LOW = 2, TMI_Y10_PACKED = 3 };

// one picture of a slot
struct TmSitiDesc {
    const void *p;
    unsigned long long pitch; // bytes
    int vec;                  // base and pitch 16-byte aligned: the wide loads are allowed
    int pad_;
};

struct TmSitiGeom {
    int w, h;
    int bits;                  // D
    int fmt;                   // TMX_F_* of the luma samples
    int shift;                 // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;             // TMX_F_U16_LOW: sample = v & mask
    int tiles_x, tiles;        // tile grid
    int n;                     // slots of this launch
    int first;                 // slot 0 starts a sequence: no comparison, T1 = T2 = 0
    unsigned long long hpitch; // samples per history row
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 3 (no interior), w h above 2^26, D outside 8 .. 16 or not
// one the layout carries
static inline int tmi_make_geom(TmSitiGeom *g, unsigned w, unsigned h, int layout, unsigned bits)
{
    memset(g, 0, sizeof *g);
    if (w < 3 || h < 3 || (unsigned long long)w * h > TMI_MAX_SAMPLES || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMI_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMI_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMI_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMI_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->w = (int)w; g->h = (int)h; g->bits = (int)bits;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->tiles_x = (g->w + TMI_TW - 1) / TMI_TW;
    g->tiles = g->tiles_x * ((g->h + TMI_TH - 1) / TMI_TH);
    g->hpitch = (unsigned long long)(g->w + 63) / 64 * 64;
    return 0;
}

// ---- wave sums of the lanes' four totals: true on the lane that holds them ----------------------------------------------------
#ifdef TM_EMULATE
// tests/siti_emul: the lanes of a workgroup are host threads; the harness sums through memory
bool tm_siti_wave_sum(unsigned long long (&v)[TMI_SUMS]);
#else
__device__ __forceinline__ bool tm_siti_wave_sum(unsigned long long (&v)[TMI_SUMS])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < TMI_SUMS; ++k) v[k] += __shfl_down(v[k], off, 64);
    }
    return (threadIdx.x & 63) == 0;
}
#endif

namespace tmi {

struct alignas(8) Pack4 { unsigned lo, hi; }; // four uint16: samples 0 | 1 << 16, 2 | 3 << 16

// The magnitude on the 16-bit scale: the q >= 0 with q^2 - q < M <= q^2 + q (M = 0: q = 0), M < 2^37.  The f32 square root of the
// rounded M is within 0.03 of sqrt(M) (two roundings of 2^-24 relative on a value below 2^18.5), so the estimate is off by one at
// the most and one step either way reaches the q of the inequality.
__device__ __forceinline__ unsigned magnitude(unsigned long long M)
{
    unsigned q = (unsigned)(sqrtf((float)M) + 0.5f);
    const unsigned long long qq = (unsigned long long)q * q;
    if (qq + q < M) ++q;
    else if (q > 0 && qq - q >= M) --q;
    return q;
}

// Samples xx .. xx+3 of picture row `yy` (inside the picture) for the staged tile, as loaded: a group inside the row of an aligned
// picture is its raw dwords (unpacked when it is written to LDS, one slot later, so that nothing waits for the load here); otherwise
// (`packed`) q[0], q[1] are the four samples already: columns outside the picture, or outside x_lo .. x_hi (what Sobel reads of this
// tile), are not fetched and are 0.
struct Staged {
    tmx::Raw4 raw;
    bool packed;
};

template <int FMT>
__device__ __forceinline__ Staged stage4(const TmSitiDesc &d, int xx, int yy, int x_lo, int x_hi, int w, int shift, unsigned mask)
{
    const char *row = (const char *)d.p + (size_t)yy * d.pitch;
    if (d.vec && xx >= 0 && xx + 4 <= w) return {tmx::load4_raw(row, FMT, xx), false};
    unsigned v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = xx + k;
        v[k] = x >= x_lo && x <= x_hi ? tmx::sample1(row, FMT, x, shift, mask) : 0u;
    }
    return {{{v[0] | v[1] << 16, v[2] | v[3] << 16, 0, 0}}, true};
}

template <int FMT>
__device__ __forceinline__ Pack4 staged_pack(const Staged &t, int xx, int shift, unsigned mask)
{
    if (t.packed) return {t.raw.q[0], t.raw.q[1]};
    unsigned v[4];
    tmx::unpack4(t.raw, FMT, xx, shift, mask, v);
    return {v[0] | v[1] << 16, v[2] | v[3] << 16};
}

} // namespace tmi

template <int FMT>
__global__ void __launch_bounds__(TMI_THREADS) k_siti(TmSitiGeom g, const TmSitiDesc *__restrict__ desc, unsigned short *__restrict__ hist,
                                                     unsigned long long *__restrict__ ACC)
{
    using namespace tmi;
    __shared__ Pack4 src[2][TMI_SH * TMI_NGX]; // the staged samples of slot s in src[s & 1]: rows y0 - 1 .. y0 + 30
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int x0 = (tile % g.tiles_x) * TMI_TW, y0 = (tile / g.tiles_x) * TMI_TH;
    const int sh = g.shift;
    const unsigned mk = g.mask;
    const int mshift = 2 * (16 - g.bits);
    // the columns of the picture Sobel reads in this tile
    const int x_lo = x0 > 0 ? x0 - 1 : 0, x_hi = x0 + TMI_TW < g.w ? x0 + TMI_TW : g.w - 1;

    // ---- this lane's staging items (row r, group gx of the staged tile): fixed over the slots
    int s_x[TMI_STAGE], s_y[TMI_STAGE]; // s_y < 0: nothing to fetch (a row or a group outside the picture, or one Sobel never reads)
#pragma unroll
    for (int k = 0; k < TMI_STAGE; ++k) {
        const int it = tid + k * TMI_THREADS, r = it / TMI_NGX, gx = it % TMI_NGX;
        const int yy = y0 - 1 + r;
        s_x[k] = x0 - 4 + 4 * gx;
        s_y[k] = it < TMI_NGX * TMI_SH && yy >= 0 && yy < g.h && s_x[k] + 3 >= x_lo && s_x[k] <= x_hi ? yy : -1;
    }
    // ---- this lane's output groups (4 samples at block-relative (4 og, orow)) and the previous slot's raw samples
    int o_g[TMI_OUT], o_r[TMI_OUT];
    bool o_on[TMI_OUT];
    Pack4 prev[TMI_OUT];
#pragma unroll
    for (int k = 0; k < TMI_OUT; ++k) {
        const int it = tid + k * TMI_THREADS;
        o_g[k] = it % (TMI_TW / 4);
        o_r[k] = it / (TMI_TW / 4);
        o_on[k] = o_r[k] < TMI_TH && y0 + o_r[k] < g.h && x0 + 4 * o_g[k] < g.w;
        prev[k] = {0u, 0u};
        if (o_on[k] && !g.first) {
            const tmx::Src hs = {(const char *)hist, g.hpitch * 2, TMX_F_HIST, 1};
            unsigned v[4];
            tmx::load4(hs, x0 + 4 * o_g[k], y0 + o_r[k], g.w, 0, 0xFFFFu, v);
            prev[k] = {v[0] | v[1] << 16, v[2] | v[3] << 16};
        }
    }

    const Staged nothing = {{{0, 0, 0, 0}}, true};
    Staged nxt[TMI_STAGE];
#pragma unroll
    for (int k = 0; k < TMI_STAGE; ++k) nxt[k] = s_y[k] >= 0 ? stage4<FMT>(desc[0], s_x[k], s_y[k], x_lo, x_hi, g.w, sh, mk) : nothing;

    for (int s = 0; s < g.n; ++s) {
        Pack4 *buf = src[s & 1];
#pragma unroll
        for (int k = 0; k < TMI_STAGE; ++k) {
            const int it = tid + k * TMI_THREADS;
            if (it < TMI_NGX * TMI_SH) buf[it] = staged_pack<FMT>(nxt[k], s_x[k], sh, mk);
        }
        // orders LDS only: a __syncthreads() would also wait for the loads issued below, one slot early.  One barrier per slot is
        // enough: slot s + 1 writes the other buffer, and nobody writes this one again before the barrier of slot s + 1.
        TM_LDS_BARRIER();
        // the next slot's samples: in flight during this slot's arithmetic
        if (s + 1 < g.n) {
            const TmSitiDesc d = desc[s + 1];
#pragma unroll
            for (int k = 0; k < TMI_STAGE; ++k)
                if (s_y[k] >= 0) nxt[k] = stage4<FMT>(d, s_x[k], s_y[k], x_lo, x_hi, g.w, sh, mk);
        }
        const bool compare = s > 0 || !g.first; // the first picture of a sequence is not compared with anything
        unsigned s1 = 0;
        int t1 = 0;
        unsigned long long s2 = 0, t2 = 0; // a lane adds 16 values: s1 < 2^23, |t1| < 2^20
#pragma unroll
        for (int k = 0; k < TMI_OUT; ++k) {
            if (!o_on[k]) continue;
            const int x = x0 + 4 * o_g[k], y = y0 + o_r[k];
            // output column 4 og is staged column 4 og + 4: Sobel reads staged columns 4 og + 3 .. 4 og + 8 of groups og, og + 1, og + 2
            // in staged rows orow .. orow + 2
            int t[3][6];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const Pack4 *row = buf + (o_r[k] + r) * TMI_NGX + o_g[k];
                const Pack4 a = row[0], b = row[1], c = row[2];
                t[r][0] = (int)(a.hi >> 16);
                t[r][1] = (int)(b.lo & 0xFFFFu); t[r][2] = (int)(b.lo >> 16); t[r][3] = (int)(b.hi & 0xFFFFu); t[r][4] = (int)(b.hi >> 16);
                t[r][5] = (int)(c.lo & 0xFFFFu);
            }
            const bool rows_in = y >= 1 && y <= g.h - 2;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (rows_in && x + j >= 1 && x + j <= g.w - 2) {
                    const int gx = (t[0][j + 2] - t[0][j]) + 2 * (t[1][j + 2] - t[1][j]) + (t[2][j + 2] - t[2][j]);
                    const int gy = (t[2][j] - t[0][j]) + 2 * (t[2][j + 1] - t[0][j + 1]) + (t[2][j + 2] - t[0][j + 2]);
                    // |gx|, |gy| <= 4 (2^D - 1) < 2^18: each square below 2^36
                    const unsigned ax = (unsigned)(gx < 0 ? -gx : gx), ay = (unsigned)(gy < 0 ? -gy : gy);
                    const unsigned long long m2 = (unsigned long long)ax * ax + (unsigned long long)ay * ay;
                    const unsigned q = magnitude(m2 << mshift);
                    s1 += q;
                    s2 += (unsigned long long)q * q;
                }
                if (compare && x + j < g.w) {
                    const int cur = t[1][j + 1], old = (int)((j < 2 ? prev[k].lo >> (16 * j) : prev[k].hi >> (16 * (j - 2))) & 0xFFFFu);
                    const int dd = cur - old;
                    const unsigned ad = (unsigned)(dd < 0 ? -dd : dd);
                    t1 += dd;
                    t2 += ad * ad; // |dd| < 2^16: the square is below 2^32
                }
            }
            prev[k] = {(unsigned)t[1][1] | (unsigned)t[1][2] << 16, (unsigned)t[1][3] | (unsigned)t[1][4] << 16};
        }
        unsigned long long v[TMI_SUMS] = {s1, s2, (unsigned long long)(long long)t1, t2};
        if (tm_siti_wave_sum(v)) {
            unsigned long long *a = ACC + ((size_t)s * TMI_BINS + (tile & (TMI_BINS - 1))) * TMI_SUMS;
#pragma unroll
            for (int k = 0; k < TMI_SUMS; ++k)
                if (v[k]) atomicAdd(&a[k], v[k]);
        }
    }
    // ---- the next launch's history: the last slot's raw tile
#pragma unroll
    for (int k = 0; k < TMI_OUT; ++k) {
        if (!o_on[k]) continue;
        const int x = x0 + 4 * o_g[k];
        unsigned short *row = hist + (size_t)(y0 + o_r[k]) * g.hpitch + x;
        if (x + 4 <= g.w) *(Pack4 *)row = prev[k];
        else
            for (int j = 0; j < 4 && x + j < g.w; ++j) row[j] = (unsigned short)((j < 2 ? prev[k].lo >> (16 * j) : prev[k].hi >> (16 * (j - 2))) & 0xFFFFu);
    }
}
