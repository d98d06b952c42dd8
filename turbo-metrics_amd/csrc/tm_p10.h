// tm_p10.h -- device addressing of the packed 10-bit rows of TM_KIND_I420_P10 (layout: tm_geom.h), shared by the engine's ingest
// (tm_kernels.h) and the XPSNR kernels (tm_xpsnr_kernels.h).
#pragma once
#include "tm_platform.h"
#include "tm_geom.h"

namespace tmk {

// sample x of a TM_KIND_I420_P10 row (tm_geom.h): block x / 384, run (x % 384) / 128, word x % 128
__device__ __forceinline__ unsigned p10_word_offset(unsigned x) { return ((x / TM_P10_BLOCK) * TM_P10_RUN + (x % TM_P10_RUN)) * 4u; }
__device__ __forceinline__ unsigned p10_shift(unsigned x) { return 10u * ((x % TM_P10_BLOCK) / TM_P10_RUN); }
__device__ __forceinline__ unsigned p10_sample(const char *row, unsigned x)
{
    return (*(const unsigned *)(row + p10_word_offset(x)) >> p10_shift(x)) & 1023u;
}

} // namespace tmk
