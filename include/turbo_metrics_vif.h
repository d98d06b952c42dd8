/*
 * turbo_metrics_vif.h -- C ABI of VMAF's VIF feature (visual information fidelity, four scales) on the MI355X (gfx950):
 * libturbometrics_vif.so, a library of its own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine),
 * libturbometrics_xpsnr.so and libturbometrics_motion.so.
 *
 * VIF compares the luma planes of a reference and a distorted picture.  The definition this library computes is stated in
 * integer Gaussian moments at four scales (exact), a per-pixel statistic in double, and per scale the sums
 * `num` and `den` of its two terms; recalled from libvmaf, believed to match, unpinned.  Only luma is read.  There is no state
 * between pairs.
 *
 * Use:  tm_vif_create -> per batch: tm_vif_set_pair (slots 0 .. n-1) -> tm_vif_compute_async(n) -> tm_vif_sync -> tm_vif_get.
 *       One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_VIF_H
#define TURBO_METRICS_VIF_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the sample values and bit depth D the metric sees):
 *   TM_VIF_Y8             bytes; D = 8
 *   TM_VIF_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (the luma of P010 / P016)
 *   TM_VIF_Y16_LOW        16-bit little-endian words, the value in the LOW D bits, higher bits ignored; D = 9 .. 16
 *   TM_VIF_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_VIF_Y8 = 0, TM_VIF_Y16_MSB = 1, TM_VIF_Y16_LOW = 2, TM_VIF_Y10_PACKED = 3 };

typedef struct tm_vif tm_vif;

/* one pair's result: per scale s = 0 .. 3 the sums of the statistic's two terms over the w_s x h_s pixels of that scale
 * (den[s] >= w_s h_s) */
typedef struct tm_vif_frame {
    double num[4];
    double den[4];
} tm_vif_frame;

/* On the current HIP device.  w, h: luma size; bits: D; batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch;
 * TM_ERR_UNSUPPORTED (before any device call): w or h below 32, D outside 8 .. 16 or not one the layout carries. */
int tm_vif_create(tm_vif **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity);
void tm_vif_destroy(tm_vif *v);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_vif_mem_usage(const tm_vif *v);
/* The pair of slot `slot`.  ref_y, dis_y: the luma planes, pitch_*: bytes per row.  mem (both planes): TM_MEM_HOST is copied before
 * the call returns; TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_vif_sync returns; TM_MEM_DEVICE is
 * read in place by the kernel (zero copy), with the same rule.  The kernels run on the library's own non-blocking stream, with no
 * ordering against the stream that produced a device surface: it must be complete before tm_vif_compute_async.  Every compute
 * consumes its slots' pairs: slots [0, n) are set again before each tm_vif_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_vif_set_pair(tm_vif *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem);
int tm_vif_compute_async(tm_vif *v, uint32_t n_slots);
int tm_vif_sync(tm_vif *v);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_vif_get(tm_vif *v, uint32_t first_slot, uint32_t n, tm_vif_frame *out);

/* host function of the definition: out[s] = num[s] / den[s] (vif_scale0 .. vif_scale3), out[4] = sum num / sum den (vif), the
 * sums taken in scale order */
void tm_vif_scores(const tm_vif_frame *f, double out[5]);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_VIF_H */
