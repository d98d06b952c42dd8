// tm_sample_load.h -- reading integer samples of one plane in the four luma layouts (bytes, 16-bit words with the value in the
// high or the low bits, the packed 10-bit upload layout of tm_geom.h) and of the uint16 history planes: 4-aligned groups of
// samples per lane.  Shared by the XPSNR kernels (tm_xpsnr_kernels.h) and the motion kernel (tm_motion_kernels.h).  Every
// function is force-inlined: a caller that passes a compile-time format gets the switch folded away.
#pragma once
#include "tm_platform.h"
#include "tm_geom.h"
#include "tm_p10.h"

// sample formats of one plane as the loader reads it
enum { TMX_F_U8 = 0, TMX_F_U16_MSB = 1, TMX_F_U16_LOW = 2, TMX_F_P10 = 3, TMX_F_HIST = 4 };

namespace tmx {

// samples x .. x+3 of row y of a plane (x a multiple of 4); samples at or beyond `lim` read as 0
struct Src {
    const char *p;
    unsigned long long pitch;
    int fmt;
    int vec;
};

__device__ __forceinline__ unsigned sample1(const char *row, int fmt, int x, int shift, unsigned mask)
{
    switch (fmt) {
    case TMX_F_U8: return (unsigned)((const unsigned char *)row)[x];
    case TMX_F_U16_MSB: return (unsigned)((const unsigned short *)row)[x] >> shift;
    case TMX_F_U16_LOW: return (unsigned)((const unsigned short *)row)[x] & mask;
    case TMX_F_P10: return tmk::p10_sample(row, (unsigned)x);
    default: return (unsigned)((const unsigned short *)row)[x];
    }
}

__device__ __forceinline__ void load4(const Src &s, int x, int y, int lim, int shift, unsigned mask, unsigned (&v)[4])
{
    const char *row = s.p + (size_t)y * s.pitch;
    if (s.vec && x + 4 <= lim) {
        switch (s.fmt) {
        case TMX_F_U8: {
            const unsigned q = *(const unsigned *)(row + x);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (q >> (8 * k)) & 255u;
            return;
        }
        case TMX_F_P10: {
            const uint4 q = *(const uint4 *)(row + tmk::p10_word_offset((unsigned)x));
            const unsigned sh = tmk::p10_shift((unsigned)x);
            v[0] = (q.x >> sh) & 1023u; v[1] = (q.y >> sh) & 1023u; v[2] = (q.z >> sh) & 1023u; v[3] = (q.w >> sh) & 1023u;
            return;
        }
        default: { // 16-bit samples: two dwords
            const uint2 q = *(const uint2 *)(row + 2 * x);
            const unsigned r[4] = {q.x & 0xFFFFu, q.x >> 16, q.y & 0xFFFFu, q.y >> 16};
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = s.fmt == TMX_F_U16_MSB ? r[k] >> shift : (s.fmt == TMX_F_U16_LOW ? r[k] & mask : r[k]);
            return;
        }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = x + k < lim ? sample1(row, s.fmt, x + k, shift, mask) : 0u;
}

// load4's wide load of samples x .. x+3 (x a multiple of 4; base and pitch 16-byte aligned) and its unpacking, separately: a caller
// that issues the load early and unpacks late keeps only the raw dwords in registers (bytes: q[0]; 16-bit samples: q[0], q[1];
// packed 10-bit: q[0] .. q[3]).  The plane is device memory: the loads are global loads, which a wait for LDS does not wait for
// (a load through a generic pointer counts as an LDS access too).
struct Raw4 { unsigned q[4]; };

__device__ __forceinline__ Raw4 load4_raw(const char *row, int fmt, int x)
{
    Raw4 r = {{0, 0, 0, 0}};
    switch (fmt) {
    case TMX_F_U8: r.q[0] = *(const TM_GLOBAL_AS unsigned *)(row + x); break;
    case TMX_F_P10: {
        const TM_GLOBAL_AS tm_u2 *p = (const TM_GLOBAL_AS tm_u2 *)(row + tmk::p10_word_offset((unsigned)x));
        const tm_u2 a = p[0], b = p[1];
        r.q[0] = a.x; r.q[1] = a.y; r.q[2] = b.x; r.q[3] = b.y;
        break;
    }
    default: { // 16-bit samples: two dwords
        const tm_u2 q = *(const TM_GLOBAL_AS tm_u2 *)(row + 2 * x); // (a plain vector type: HIP's uint2 would be read through a generic reference)
        r.q[0] = q.x; r.q[1] = q.y;
        break;
    }
    }
    return r;
}

__device__ __forceinline__ void unpack4(const Raw4 &r, int fmt, int x, int shift, unsigned mask, unsigned (&v)[4])
{
    switch (fmt) {
    case TMX_F_U8:
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (r.q[0] >> (8 * k)) & 255u;
        return;
    case TMX_F_P10: {
        const unsigned sh = tmk::p10_shift((unsigned)x);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (r.q[k] >> sh) & 1023u;
        return;
    }
    default: {
        const unsigned t[4] = {r.q[0] & 0xFFFFu, r.q[0] >> 16, r.q[1] & 0xFFFFu, r.q[1] >> 16};
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = fmt == TMX_F_U16_MSB ? t[k] >> shift : (fmt == TMX_F_U16_LOW ? t[k] & mask : t[k]);
        return;
    }
    }
}

} // namespace tmx
