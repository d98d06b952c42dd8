/*
 * turbo_metrics_hvs.h -- C ABI of PSNR-HVS (Egiazarian et al., 2006) and PSNR-HVS-M (Ponomarenko et al., 2007) on the MI355X (gfx950):
 * libturbometrics_hvs.so, a library of its own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the other feature
 * libraries.
 *
 * Both compare the luma planes of a reference and a distorted picture over non-overlapping 8x8 blocks: the DCT coefficients of the
 * difference, weighted by a contrast sensitivity table; PSNR-HVS-M first lowers every AC coefficient by a contrast masking threshold
 * taken from the two pictures' blocks.  The definition this library computes is stated in DESIGN.md section 16: exact integers up to
 * the transforms, one f32 expression per block, f64 sums over the blocks in a fixed order; recalled from the authors' MATLAB
 * psnrhvsm.m, believed to match, unpinned.  It is NOT the psnr_hvs of libvmaf / Daala (overlapping blocks, an integer transform, other
 * tables).  Only luma is read.  There is no state between pairs.
 *
 * Use:  tm_hvs_create -> per batch: tm_hvs_set_pair (slots 0 .. n-1) -> tm_hvs_compute_async(n) -> tm_hvs_sync -> tm_hvs_get.
 *       One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_HVS_H
#define TURBO_METRICS_HVS_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the sample values and bit depth D the metric sees), numbered as in turbo_metrics_vif.h:
 *   TM_HVS_Y8             bytes; D = 8
 *   TM_HVS_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (the luma of P010 / P016)
 *   TM_HVS_Y16_LOW        16-bit little-endian words, the value in the LOW D bits, higher bits ignored; D = 9 .. 16
 *   TM_HVS_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_HVS_Y8 = 0, TM_HVS_Y16_MSB = 1, TM_HVS_Y16_LOW = 2, TM_HVS_Y10_PACKED = 3 };

typedef struct tm_hvs tm_hvs;

/* one pair's result: S2 and S1 of DESIGN.md section 16 -- the sums over all blocks of the squared CSF-weighted coefficients of the
 * difference, unmasked (PSNR-HVS) and masked (PSNR-HVS-M) -- and the number of 8x8 blocks, (w / 8) (h / 8) rounded down each */
typedef struct tm_hvs_frame {
    double s_hvs, s_hvsm;
    uint64_t blocks;
} tm_hvs_frame;

/* On the current HIP device.  w, h: luma size; bits: D; batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch, more than
 * 65535 slots; TM_ERR_UNSUPPORTED (before any device call): w or h below 8 or above 32768, D outside 8 .. 16 or not one the layout
 * carries. */
int tm_hvs_create(tm_hvs **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity);
void tm_hvs_destroy(tm_hvs *v);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_hvs_mem_usage(const tm_hvs *v);
/* The pair of slot `slot`.  ref_y, dis_y: the luma planes, pitch_*: bytes per row.  mem (both planes): TM_MEM_HOST is copied before
 * the call returns; TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_hvs_sync returns; TM_MEM_DEVICE is
 * read in place by the kernel (zero copy), with the same rule.  The kernels run on the library's own non-blocking stream, with no
 * ordering against the stream that produced a device surface: it must be complete before tm_hvs_compute_async.  Every compute
 * consumes its slots' pairs: slots [0, n) are set again before each tm_hvs_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_hvs_set_pair(tm_hvs *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem);
int tm_hvs_compute_async(tm_hvs *v, uint32_t n_slots);
int tm_hvs_sync(tm_hvs *v);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_hvs_get(tm_hvs *v, uint32_t first_slot, uint32_t n, tm_hvs_frame *out);

/* host functions of the definition.
 * tm_hvs_psnr: 10 log10(peak^2 * 64 * blocks / s) with peak = 2^bits - 1; +inf for s = 0; NaN for bits outside 8 .. 16 or no block.
 * A sequence's value is tm_hvs_psnr of the summed s and the summed blocks.
 * tm_hvs_csf / tm_hvs_mask: the two 8x8 tables, 64 floats each, [vertical frequency][horizontal frequency]. */
double tm_hvs_psnr(double s, uint64_t blocks, uint32_t bits);
const float *tm_hvs_csf(void);
const float *tm_hvs_mask(void);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_HVS_H */
