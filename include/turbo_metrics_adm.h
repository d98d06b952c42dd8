/*
 * turbo_metrics_adm.h -- C ABI of VMAF's ADM feature (the detail-loss metric: adm2 and adm_scale0 .. adm_scale3) on the MI355X
 * (gfx950): libturbometrics_adm.so, a library of its own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine),
 * libturbometrics_xpsnr.so, libturbometrics_motion.so and libturbometrics_vif.so.
 *
 * ADM compares the luma planes of a reference and a distorted picture.  The definition this library computes is stated in
 * a four-level db2 wavelet pyramid in f32, the decoupling of the distorted picture's detail bands, a 3 x 3
 * masking threshold, and per scale and band the sums of cubes over the centre of the plane; recalled from libvmaf's float adm,
 * believed to match, unpinned.  Only luma is read.  There is no state between pairs.
 *
 * Use:  tm_adm_create -> per batch: tm_adm_set_pair (slots 0 .. n-1) -> tm_adm_compute_async(n) -> tm_adm_sync -> tm_adm_get.
 *       One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_ADM_H
#define TURBO_METRICS_ADM_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the sample values and bit depth D the metric sees):
 *   TM_ADM_Y8             bytes; D = 8
 *   TM_ADM_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (the luma of P010 / P016)
 *   TM_ADM_Y16_LOW        16-bit little-endian words, the value in the LOW D bits, higher bits ignored; D = 9 .. 16
 *   TM_ADM_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_ADM_Y8 = 0, TM_ADM_Y16_MSB = 1, TM_ADM_Y16_LOW = 2, TM_ADM_Y10_PACKED = 3 };

typedef struct tm_adm tm_adm;

/* one pair's result: per scale s = 0 .. 3 and band b = h, v, d the sums over the centre region of the band plane of the cubes of
 * the masked restored coefficient (num_cube) and of the weighted reference coefficient (den_cube) */
typedef struct tm_adm_frame {
    double num_cube[4][3];
    double den_cube[4][3];
} tm_adm_frame;

/* On the current HIP device.  w, h: luma size; bits: D; batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch;
 * TM_ERR_UNSUPPORTED (before any device call): w or h below 32, D outside 8 .. 16 or not one the layout carries. */
int tm_adm_create(tm_adm **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity);
void tm_adm_destroy(tm_adm *v);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_adm_mem_usage(const tm_adm *v);
/* The pair of slot `slot`.  ref_y, dis_y: the luma planes, pitch_*: bytes per row.  mem (both planes): TM_MEM_HOST is copied before
 * the call returns; TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_adm_sync returns; TM_MEM_DEVICE is
 * read in place by the kernel (zero copy), with the same rule.  The kernels run on the library's own non-blocking stream, with no
 * ordering against the stream that produced a device surface: it must be complete before tm_adm_compute_async.  Every compute
 * consumes its slots' pairs: slots [0, n) are set again before each tm_adm_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_adm_set_pair(tm_adm *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem);
int tm_adm_compute_async(tm_adm *v, uint32_t n_slots);
int tm_adm_sync(tm_adm *v);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_adm_get(tm_adm *v, uint32_t first_slot, uint32_t n, tm_adm_frame *out);

/* host function of the definition, for a frame of a w x h pair: with area_s the pixels of the region the sums ran over,
 * num_s = sum_b (cbrt(num_cube[s][b]) + cbrt(area_s / 32)), den_s likewise; out[s] = score(num_s, den_s) (adm_scale0 ..
 * adm_scale3), out[4] = score(sum num_s, sum den_s) (adm2), the sums taken in scale order; score(n, d): each below 1e-10 counts
 * as 0, d == 0 gives 1, otherwise n / d */
void tm_adm_scores(const tm_adm_frame *f, uint32_t w, uint32_t h, double out[5]);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_ADM_H */
