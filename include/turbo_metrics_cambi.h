/*
 * turbo_metrics_cambi.h -- C ABI of CAMBI, VMAF's banding index, on the MI355X (gfx950): libturbometrics_cambi.so, a library of its
 * own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the XPSNR, motion, VIF, ADM and scene libraries.
 *
 * The definition is DESIGN.md section 13: one luma plane -> 10 bits (and an anti-dither filter below 10 bits) -> a spatial mask of
 * flat neighbourhoods -> five scales, each mode-filtered -> per masked pixel the c-value, the largest contrast-weighted share of a
 * neighbouring code value in a window -> per scale the mean of the top-k c-values -> one weighted score.  CAMBI is a no-reference
 * metric: one stream per object, nothing kept between pictures or computes.  The device delivers per scale the k-th largest c-value,
 * the number of values above it and their sum; the scores are the host function tm_cambi_scores.  Parity with libvmaf is recalled,
 * not pinned; no encode-resolution resize, no full_ref mode, no EOTF other than BT.1886.
 *
 * Use:  tm_cambi_create -> per batch: tm_cambi_set_frame (slots 0 .. n-1) -> tm_cambi_compute_async(n) -> tm_cambi_sync ->
 *       tm_cambi_get -> tm_cambi_scores; tm_cambi_get_map for the c-value plane (the heat map) of a computed slot.
 *       One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_CAMBI_H
#define TURBO_METRICS_CAMBI_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the numbering and the meaning of turbo_metrics_motion.h):
 *   TM_CAMBI_Y8             bytes; D = 8
 *   TM_CAMBI_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (the luma of P010 / P016)
 *   TM_CAMBI_Y16_LOW        16-bit little-endian words, the value in the LOW D bits, higher bits ignored; D = 9 .. 16
 *   TM_CAMBI_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_CAMBI_Y8 = 0, TM_CAMBI_Y16_MSB = 1, TM_CAMBI_Y16_LOW = 2, TM_CAMBI_Y10_PACKED = 3 };

#define TM_CAMBI_SCALES 5
#define TM_CAMBI_DEFAULT_TOPK 0.6
#define TM_CAMBI_DEFAULT_TVI_THRESHOLD 0.019

typedef struct tm_cambi tm_cambi;

/* one picture's result, per scale s (w_s x h_s c-values, w_s = (w_{s-1} + 1) >> 1):
 *   k       clamp(floor(topk w_s h_s), 1, w_s h_s)
 *   t       the k-th largest c-value, as f32 bits (non-negative f32 values order like their bit patterns)
 *   n_gt    the number of c-values strictly above t
 *   sum_gt  their sum in f64, accumulated in a fixed order: two computes of one picture give identical bits */
typedef struct tm_cambi_frame {
    uint32_t t[TM_CAMBI_SCALES];
    uint32_t n_gt[TM_CAMBI_SCALES];
    uint32_t k[TM_CAMBI_SCALES];
    uint32_t reserved;
    double sum_gt[TM_CAMBI_SCALES];
} tm_cambi_frame;

/* On the current HIP device.  w, h: luma size; bits: D; window: 0 (derive: 63 w / 3840, at least 3) or 3 .. 127; topk in (0, 1];
 * batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch; TM_ERR_UNSUPPORTED (before any device call): w or h below 32,
 * w h above 2^31, D outside 8 .. 16 or not one the layout carries, a window outside {0, 3 .. 127}, a topk outside (0, 1]. */
int tm_cambi_create(tm_cambi **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t window, double topk, double tvi_threshold,
                    uint32_t batch_capacity);
void tm_cambi_destroy(tm_cambi *s);
/* bytes of device and page-locked host memory the library holds */
size_t tm_cambi_mem_usage(const tm_cambi *s);
/* The picture of slot `slot`.  y: the luma plane, pitch_y: bytes per row.  mem: TM_MEM_HOST is copied before the call returns;
 * TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_cambi_sync returns; TM_MEM_DEVICE is read in place
 * by the kernel (zero copy), with the same rule.  The kernels run on the library's own non-blocking stream, with no ordering
 * against the stream that produced a device surface: it must be complete before tm_cambi_compute_async.  A base or pitch that is
 * not 16-byte aligned is read sample by sample instead of with wide loads; the result is the same.  Every compute consumes its
 * slots' pictures: slots [0, n) are set again before each tm_cambi_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_cambi_set_frame(tm_cambi *s, uint32_t slot, const void *y, size_t pitch_y, int mem);
int tm_cambi_compute_async(tm_cambi *s, uint32_t n_slots);
int tm_cambi_sync(tm_cambi *s);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_cambi_get(tm_cambi *s, uint32_t first_slot, uint32_t n, tm_cambi_frame *out);
/* the c-values of scale `scale` of slot `slot` of the last compute, w_scale x h_scale floats, rows `pitch` bytes apart in host
 * memory (synchronises).  TM_ERR_STATE for a slot the last compute did not cover; TM_ERR_INVALID_ARG for a scale above 4, a pitch
 * below a row or not a multiple of 4 */
int tm_cambi_get_map(tm_cambi *s, uint32_t slot, uint32_t scale, float *out, size_t pitch);

/* host functions of the definition: plain C, no device call */
/* out[0 .. 4]: score_s = (sum_gt + (k - n_gt) t) / k; out[5]: cambi = min(sum_s weight_s score_s / area, 1000), weights 16, 8, 4, 2,
 * 1, area = (2 (window >> 1) + 1)^2.  window: the window in use (tm_cambi_window) */
int tm_cambi_scores(const tm_cambi_frame *frame, uint32_t window, double out[6]);
/* the largest 10-bit code x in 64 .. 939 at which a step of d = 1 .. 4 codes is still visible at this threshold (BT.1886, 300 and
 * 0.01 cd/m2); 0.019 gives 178, 305, 432, 559 */
int tm_cambi_tvi(double tvi_threshold, uint32_t out[4]);
/* (49 + 3 (ceil(log2(min(w, h))) - 11) - 1) >> 1 */
uint32_t tm_cambi_mask_index(uint32_t w, uint32_t h);
/* requested, or for 0: max(63 w / 3840, 3), at most 127 */
uint32_t tm_cambi_window(uint32_t w, uint32_t requested);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_CAMBI_H */
