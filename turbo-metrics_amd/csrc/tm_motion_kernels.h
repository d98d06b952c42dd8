// tm_motion_kernels.h -- gfx950 kernel of VMAF's integer motion (libturbometrics_motion.so, include/turbo_metrics_motion.h).
//
// The definition is DESIGN.md section 9; its literal CPU restatement is tests/motion_ref.py.  Per picture: a separable 5-tap
// integer low-pass of the luma plane (vertical pass first, rounded to 16 bits, then the horizontal pass on the rounded values;
// asymmetric mirror at the borders), and the sum of absolute differences between that blurred plane and the previous picture's.
//
//   k_motion<FMT>   grid (luma tiles)   block 256   one workgroup per tile of 120 x 16 samples, walking the launch's slots in
//                   sequence order.  Per slot it stages the tile plus its 2-sample halo in LDS (every lane reads 4-aligned
//                   groups of 4 samples; the mirror is applied while staging, so both passes are plain stencils), runs the
//                   vertical pass LDS -> LDS and the horizontal pass LDS -> registers, and keeps the blurred tile of the previous
//                   slot in registers: a blurred plane never goes through memory inside a launch.  The loads of slot s + 1 are
//                   issued before the passes of slot s.  A lane's |B - B_prev| sum is a uint32, reduced over the wave with
//                   shuffles and added to the slot's uint64 by one atomic per wave; integer addition, so the order of arrival
//                   cannot change a bit.
//
// History.  The workgroup of a tile writes the last slot's blurred tile to the history plane (uint16) and the same tile's
// workgroup of the next launch reads it for its slot 0.  Tiles are disjoint: nothing else touches those samples, so one plane is
// enough.  The first launch of a sequence (g.first) does not read it: slot 0 has sad 0.
//
// The tile.  LDS rows hold 128 samples: columns x0 - 4 .. x0 + 123, i.e. 32 groups of 4, so that the vertical pass is exactly one
// item per lane (32 groups x 8 row pairs) with conflict-free 8-byte accesses.  Of those columns the horizontal pass reads
// x0 - 2 .. x0 + 121.
#pragma once
#include <string.h>

#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_sample_load.h" // TMX_F_*, tmx::Src / sample1 / load4: the loaders of the XPSNR kernels

#define TMM_THREADS 256
#define TMM_TW 120                               /* output columns per tile */
#define TMM_TH 16                                /* output rows per tile */
#define TMM_NGX ((TMM_TW + 8) / 4)               /* 4-sample groups per staged row: 32 */
#define TMM_LW (4 * TMM_NGX)                     /* LDS row, samples */
#define TMM_SH (TMM_TH + 4)                      /* staged rows */
#define TMM_STAGE ((TMM_NGX * TMM_SH + TMM_THREADS - 1) / TMM_THREADS)           /* staging items per lane: 3 */
#define TMM_OUT (((TMM_TW / 4) * TMM_TH + TMM_THREADS - 1) / TMM_THREADS)        /* output groups per lane: 2 */
#define TMM_BINS 16                              /* uint64 accumulators per slot (spreads the atomics) */

// layouts of include/turbo_metrics_motion.h (the luma planes of the XPSNR layouts)
enum { TMM_Y8 = 0, TMM_Y16_MSB = 1, TMM_Y16_LOW = 2, TMM_Y10_PACKED = 3 };

// one picture of a slot
struct TmMotionDesc {
    const void *p;
    unsigned long long pitch; // bytes
    int vec;                  // base and pitch 16-byte aligned: the wide loads are allowed
    int pad_;
};

struct TmMotionGeom {
    int w, h;
    int bits;                  // D
    int fmt;                   // TMX_F_* of the luma samples
    int shift;                 // TMX_F_U16_MSB: sample = v >> shift
    unsigned mask;             // TMX_F_U16_LOW: sample = v & mask
    int tiles_x, tiles;        // tile grid
    int n;                     // slots of this launch
    int first;                 // slot 0 starts a sequence: no comparison, sad = 0
    unsigned long long hpitch; // samples per history row
};

// 0, or -1 for what the library refuses as TM_ERR_UNSUPPORTED: w or h below 3 (the mirror would leave the plane), D outside
// 8 .. 16 or not one the layout carries
static inline int tmm_make_geom(TmMotionGeom *g, unsigned w, unsigned h, int layout, unsigned bits)
{
    memset(g, 0, sizeof *g);
    if (w < 3 || h < 3 || bits < 8 || bits > 16) return -1;
    switch (layout) {
    case TMM_Y8: if (bits != 8) return -1; g->fmt = TMX_F_U8; break;
    case TMM_Y16_MSB: if (bits < 9) return -1; g->fmt = TMX_F_U16_MSB; break;
    case TMM_Y16_LOW: if (bits < 9) return -1; g->fmt = TMX_F_U16_LOW; break;
    case TMM_Y10_PACKED: if (bits != 10) return -1; g->fmt = TMX_F_P10; break;
    default: return -1;
    }
    g->w = (int)w; g->h = (int)h; g->bits = (int)bits;
    g->shift = 16 - (int)bits;
    g->mask = (1u << bits) - 1u;
    g->tiles_x = (g->w + TMM_TW - 1) / TMM_TW;
    g->tiles = g->tiles_x * ((g->h + TMM_TH - 1) / TMM_TH);
    g->hpitch = (unsigned long long)(g->w + 63) / 64 * 64;
    return 0;
}

// ---- wave sum of the lanes' absolute differences: true on the lane that holds the total ---------------------------------------
#ifdef TM_EMULATE
// tests/motion_emul: the lanes of a workgroup are host threads; the harness sums through memory
bool tm_motion_wave_sum(unsigned &v);
#else
__device__ __forceinline__ bool tm_motion_wave_sum(unsigned &v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return (threadIdx.x & 63) == 0;
}
#endif

namespace tmm {

// the definition's border rule: the top / left edge reflects without repeating the edge sample, the bottom / right edge repeats it
__device__ __forceinline__ int mirror(int i, int n)
{
    const int a = i < 0 ? -i : i;
    return a < n ? a : 2 * n - a - 1;
}

// F = {3571, 16004, 26386, 16004, 3571} on five values below 2^16: below 2^32 (65536 * 65535), every product of 24-bit factors
__device__ __forceinline__ unsigned taps(unsigned a, unsigned b, unsigned c, unsigned d, unsigned e)
{
    return tm_mul24(3571u, a + e) + tm_mul24(16004u, b + d) + tm_mul24(26386u, c);
}

struct alignas(8) Pack4 { unsigned lo, hi; }; // four uint16: samples 0 | 1 << 16, 2 | 3 << 16

// Samples xx .. xx+3 of picture row `yy` (already mirrored) for the staged tile, as loaded: a group inside the plane of an aligned
// picture is its raw dwords (unpacked when it is written to LDS, one slot later, so that nothing waits for the load here);
// otherwise (`packed`) q[0], q[1] are the four samples already: columns outside the plane mirrored, columns the passes never read
// (beyond w + 1) 0.
struct Staged {
    tmx::Raw4 raw;
    bool packed;
};

template <int FMT>
__device__ __forceinline__ Staged stage4(const TmMotionDesc &d, int xx, int yy, int w, int shift, unsigned mask)
{
    const char *row = (const char *)d.p + (size_t)yy * d.pitch;
    if (d.vec && xx >= 0 && xx + 4 <= w) return {tmx::load4_raw(row, FMT, xx), false};
    unsigned v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = xx + k;
        v[k] = x >= -2 && x <= w + 1 ? tmx::sample1(row, FMT, mirror(x, w), shift, mask) : 0u;
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

} // namespace tmm

template <int FMT>
__global__ void __launch_bounds__(TMM_THREADS) k_motion(TmMotionGeom g, const TmMotionDesc *__restrict__ desc, unsigned short *__restrict__ hist,
                                                       unsigned long long *__restrict__ SAD)
{
    using namespace tmm;
    __shared__ Pack4 src[TMM_SH * TMM_NGX]; // the staged samples, rows y0 - 2 .. y0 + 17
    __shared__ Pack4 ver[TMM_TH * TMM_NGX]; // the vertical pass, rows y0 .. y0 + 15
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int x0 = (tile % g.tiles_x) * TMM_TW, y0 = (tile / g.tiles_x) * TMM_TH;
    const int sh = g.shift;
    const unsigned mk = g.mask;
    const unsigned vround = 1u << (g.bits - 1);

    // ---- this lane's staging items (row r, group gx of the staged tile): fixed over the slots
    int s_x[TMM_STAGE], s_y[TMM_STAGE]; // s_y < 0: nothing to stage (beyond the tile, or a row the passes never read)
#pragma unroll
    for (int k = 0; k < TMM_STAGE; ++k) {
        const int it = tid + k * TMM_THREADS, r = it / TMM_NGX, gx = it % TMM_NGX;
        const int yy = y0 - 2 + r;
        s_x[k] = x0 - 4 + 4 * gx;
        s_y[k] = it < TMM_NGX * TMM_SH && yy <= g.h + 1 && s_x[k] <= g.w + 1 ? mirror(yy, g.h) : -1;
    }
    // ---- this lane's output groups (4 samples at block-relative (4 og, orow)) and the previous slot's blurred values
    int o_g[TMM_OUT], o_r[TMM_OUT];
    bool o_on[TMM_OUT];
    unsigned prev[TMM_OUT][4];
#pragma unroll
    for (int k = 0; k < TMM_OUT; ++k) {
        const int it = tid + k * TMM_THREADS;
        o_g[k] = it % (TMM_TW / 4);
        o_r[k] = it / (TMM_TW / 4);
        o_on[k] = o_r[k] < TMM_TH && y0 + o_r[k] < g.h && x0 + 4 * o_g[k] < g.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) prev[k][j] = 0;
        if (o_on[k] && !g.first) {
            const int x = x0 + 4 * o_g[k];
            const tmx::Src hs = {(const char *)hist, g.hpitch * 2, TMX_F_HIST, 1};
            tmx::load4(hs, x, y0 + o_r[k], g.w, 0, 0xFFFFu, prev[k]);
        }
    }

    Staged nxt[TMM_STAGE];
#pragma unroll
    for (int k = 0; k < TMM_STAGE; ++k) nxt[k] = s_y[k] >= 0 ? stage4<FMT>(desc[0], s_x[k], s_y[k], g.w, sh, mk) : Staged{{{0, 0, 0, 0}}, true};

    for (int s = 0; s < g.n; ++s) {
#pragma unroll
        for (int k = 0; k < TMM_STAGE; ++k) {
            const int it = tid + k * TMM_THREADS;
            if (it < TMM_NGX * TMM_SH) src[it] = staged_pack<FMT>(nxt[k], s_x[k], sh, mk);
        }
        TM_LDS_BARRIER(); // orders LDS only: a __syncthreads() would also wait for the loads issued below, one slot early
        // the next slot's samples: in flight during this slot's passes
        if (s + 1 < g.n) {
            const TmMotionDesc d = desc[s + 1];
#pragma unroll
            for (int k = 0; k < TMM_STAGE; ++k)
                if (s_y[k] >= 0) nxt[k] = stage4<FMT>(d, s_x[k], s_y[k], g.w, sh, mk);
        }
        // ---- vertical pass: group gx, rows 2 rp and 2 rp + 1 of the tile from staged rows 2 rp .. 2 rp + 5
        {
            const int gx = tid % TMM_NGX, rp = tid / TMM_NGX;
            Pack4 q[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) q[j] = src[(2 * rp + j) * TMM_NGX + gx];
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                unsigned v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#define TMM_S(j) (c < 2 ? (q[o + (j)].lo >> (16 * c)) & 0xFFFFu : (q[o + (j)].hi >> (16 * (c - 2))) & 0xFFFFu)
                    v[c] = (taps(TMM_S(0), TMM_S(1), TMM_S(2), TMM_S(3), TMM_S(4)) + vround) >> g.bits;
#undef TMM_S
                }
                ver[(2 * rp + o) * TMM_NGX + gx] = {v[0] | v[1] << 16, v[2] | v[3] << 16};
            }
        }
        TM_LDS_BARRIER();
        // ---- horizontal pass and the absolute differences
        unsigned acc = 0;
#pragma unroll
        for (int k = 0; k < TMM_OUT; ++k) {
            if (!o_on[k]) continue;
            // output column 4 og is staged column 4 og + 4: its taps are columns 4 og + 2 .. 4 og + 9 of groups og, og + 1, og + 2
            const Pack4 a = ver[o_r[k] * TMM_NGX + o_g[k]], b = ver[o_r[k] * TMM_NGX + o_g[k] + 1], c = ver[o_r[k] * TMM_NGX + o_g[k] + 2];
            const unsigned t[8] = {a.hi & 0xFFFFu, a.hi >> 16, b.lo & 0xFFFFu, b.lo >> 16, b.hi & 0xFFFFu, b.hi >> 16, c.lo & 0xFFFFu, c.lo >> 16};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned bl = (taps(t[j], t[j + 1], t[j + 2], t[j + 3], t[j + 4]) + 32768u) >> 16;
                if (x0 + 4 * o_g[k] + j < g.w) acc += bl > prev[k][j] ? bl - prev[k][j] : prev[k][j] - bl;
                prev[k][j] = bl;
            }
        }
        if (s == 0 && g.first) acc = 0; // the first picture of a sequence is not compared with anything
        if (tm_motion_wave_sum(acc)) atomicAdd(&SAD[(size_t)s * TMM_BINS + (tile & (TMM_BINS - 1))], (unsigned long long)acc);
    }
    // ---- the next launch's history: the last slot's blurred tile
#pragma unroll
    for (int k = 0; k < TMM_OUT; ++k) {
        if (!o_on[k]) continue;
        const int x = x0 + 4 * o_g[k];
        unsigned short *row = hist + (size_t)(y0 + o_r[k]) * g.hpitch + x;
        if (x + 4 <= g.w) *(Pack4 *)row = {prev[k][0] | prev[k][1] << 16, prev[k][2] | prev[k][3] << 16};
        else
            for (int j = 0; j < 4 && x + j < g.w; ++j) row[j] = (unsigned short)prev[k][j];
    }
}
