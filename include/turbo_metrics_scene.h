/*
 * turbo_metrics_scene.h -- C ABI of scene-cut detection on the MI355X (gfx950): libturbometrics_scene.so, a library of its own
 * beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the XPSNR, motion, VIF and ADM libraries.
 *
 * The device computes ONE thing: the 256-bin histogram of a luma plane, hist[b] = the number of samples with
 * sample >> (D - 8) == b.  All integer, exact.  Only luma is read.  The library is stateless: one histogram
 * per picture, nothing kept between pictures or computes.  The verdict -- bin merging, distance, score, threshold -- is the four
 * host functions at the end, plain C on 256 integers: policy changes without touching a kernel.
 *
 * Use:  tm_scene_create -> per batch: tm_scene_set_frame (slots 0 .. n-1) -> tm_scene_compute_async(n) -> tm_scene_sync ->
 *       tm_scene_get; then per picture tm_scene_distance against the previous picture's histogram, tm_scene_score, tm_scene_is_cut.
 *       One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_SCENE_H
#define TURBO_METRICS_SCENE_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the numbering and the meaning of turbo_metrics_motion.h):
 *   TM_SCENE_Y8             bytes; D = 8
 *   TM_SCENE_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (the luma of P010 / P016)
 *   TM_SCENE_Y16_LOW        16-bit little-endian words, the value in the LOW D bits, higher bits ignored; D = 9 .. 16
 *   TM_SCENE_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_SCENE_Y8 = 0, TM_SCENE_Y16_MSB = 1, TM_SCENE_Y16_LOW = 2, TM_SCENE_Y10_PACKED = 3 };

typedef struct tm_scene tm_scene;

/* one picture's result: hist[b] = samples with sample >> (D - 8) == b; the 256 counts add up to w h */
typedef struct tm_scene_frame {
    uint32_t hist[256];
} tm_scene_frame;

/* On the current HIP device.  w, h: luma size (1 x 1 is a picture); bits: D; batch_capacity: slots.  TM_ERR_INVALID_ARG: null out,
 * zero batch; TM_ERR_UNSUPPORTED (before any device call): w or h of 0, w h above 2^31, D outside 8 .. 16 or not one the layout
 * carries. */
int tm_scene_create(tm_scene **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity);
void tm_scene_destroy(tm_scene *s);
/* bytes of device and page-locked host memory the library holds */
size_t tm_scene_mem_usage(const tm_scene *s);
/* The picture of slot `slot`.  y: the luma plane, pitch_y: bytes per row.  mem: TM_MEM_HOST is copied before the call returns;
 * TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_scene_sync returns; TM_MEM_DEVICE is read in place
 * by the kernel (zero copy), with the same rule.  The kernel runs on the library's own non-blocking stream, with no ordering
 * against the stream that produced a device surface: it must be complete before tm_scene_compute_async.  A base or pitch that is
 * not 16-byte aligned is read sample by sample instead of with wide loads; the result is the same.  Every compute consumes its
 * slots' pictures: slots [0, n) are set again before each tm_scene_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_scene_set_frame(tm_scene *s, uint32_t slot, const void *y, size_t pitch_y, int mem);
int tm_scene_compute_async(tm_scene *s, uint32_t n_slots);
int tm_scene_sync(tm_scene *s);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_scene_get(tm_scene *s, uint32_t first_slot, uint32_t n, tm_scene_frame *out);

/* host functions of the definition: plain C, no device call */
#define TM_SCENE_DEFAULT_BINS 64
#define TM_SCENE_DEFAULT_THRESHOLD 0.5
/* bins: 8, 16, 32, 64, 128 or 256 (anything else, or a null pointer: TM_ERR_INVALID_ARG).  Every run of 256 / bins adjacent bins is
 * added up in 64 bits; *out = sum over the merged bins k of |A_k - B_k| */
int tm_scene_distance(const uint32_t a[256], const uint32_t b[256], int bins, uint64_t *out);
/* (double)distance / (2.0 (double)w (double)h): 0 for equal histograms, 1 when no merged bin is shared */
double tm_scene_score(uint64_t distance, uint32_t w, uint32_t h);
/* score >= threshold.  The first picture of a sequence has score 0 and is never a cut */
int tm_scene_is_cut(double score, double threshold);
/* the lowest and the highest bin that is not empty, and sum(b hist[b]) (64-bit integer) divided once by sum(hist[b]).  An empty
 * histogram or a null pointer: TM_ERR_INVALID_ARG */
int tm_scene_stats(const uint32_t hist[256], uint32_t *min_bin, uint32_t *max_bin, double *mean_bin);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_SCENE_H */
