/*
 * turbo_metrics_motion.h -- C ABI of VMAF's integer motion feature on the MI355X (gfx950): libturbometrics_motion.so, a library
 * of its own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and libturbometrics_xpsnr.so.
 *
 * `motion` / `motion2` is VMAF's temporal feature (ffmpeg's `vmafmotion`): the mean absolute difference between consecutive
 * low-pass-filtered luma pictures of ONE sequence.  The definition this library computes is stated in DESIGN.md section 9: the
 * blur and the sum of absolute differences are all integer and exact; the normalisation and motion2 are recalled from libvmaf
 * (unpinned).  Only luma is read.  It is stateful: a picture is compared with the previous picture of the sequence, which the
 * engine keeps across batches.  The first picture of a sequence has sad = 0 and motion = 0.
 *
 * Use:  tm_motion_create -> per batch: tm_motion_set_frame (slots 0 .. n-1) -> tm_motion_compute_async(n) -> tm_motion_sync ->
 *       tm_motion_get.  Slots 0 .. n-1 of a batch are the next n pictures of the sequence, in order.  tm_motion_reset starts a
 *       new sequence.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_MOTION_H
#define TURBO_METRICS_MOTION_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the sample values and bit depth D the metric sees):
 *   TM_MOTION_Y8             bytes; D = 8
 *   TM_MOTION_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (the luma of P010 / P016)
 *   TM_MOTION_Y16_LOW        16-bit little-endian words, the value in the LOW D bits, higher bits ignored; D = 9 .. 16
 *   TM_MOTION_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_MOTION_Y8 = 0, TM_MOTION_Y16_MSB = 1, TM_MOTION_Y16_LOW = 2, TM_MOTION_Y10_PACKED = 3 };

typedef struct tm_motion tm_motion;

/* one picture's result: the sum of absolute differences of the blurred planes (16-bit scale) and libvmaf's normalisation of it */
typedef struct tm_motion_frame {
    uint64_t sad;
    double motion;
} tm_motion_frame;

/* On the current HIP device.  w, h: luma size; bits: D; batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch;
 * TM_ERR_UNSUPPORTED (before any device call): w or h below 3, D outside 8 .. 16 or not one the layout carries. */
int tm_motion_create(tm_motion **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity);
void tm_motion_destroy(tm_motion *m);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_motion_mem_usage(const tm_motion *m);
/* The picture of slot `slot`.  y: the luma plane, pitch_y: bytes per row.  mem: TM_MEM_HOST is copied before the call returns;
 * TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_motion_sync returns; TM_MEM_DEVICE is read in place
 * by the kernel (zero copy), with the same rule.  The kernel runs on the library's own non-blocking stream, with no ordering
 * against the stream that produced a device surface: it must be complete before tm_motion_compute_async.  Every compute consumes
 * its slots' pictures: slots [0, n) are set again before each tm_motion_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_motion_set_frame(tm_motion *m, uint32_t slot, const void *y, size_t pitch_y, int mem);
/* slots [0, n_slots) continue the sequence */
int tm_motion_compute_async(tm_motion *m, uint32_t n_slots);
int tm_motion_sync(tm_motion *m);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_motion_get(tm_motion *m, uint32_t first_slot, uint32_t n, tm_motion_frame *out);
/* the next compute starts a new sequence */
int tm_motion_reset(tm_motion *m);

/* host functions of the definition */
/* (double)((float)(sad / 256.0) / (float)(w h)): libvmaf's normalize_and_scale_sad, float casts included */
double tm_motion_from_sad(uint64_t sad, uint32_t w, uint32_t h);
/* motion2 of picture i: min(motion[i], motion[i + 1]); the last picture's motion2 is its motion */
double tm_motion2(double motion_i, double motion_next);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_MOTION_H */
