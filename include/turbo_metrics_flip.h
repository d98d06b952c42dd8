/*
 * turbo_metrics_flip.h -- C ABI of LDR-FLIP, the perceptual image-difference map, on the MI355X (gfx950): libturbometrics_flip.so, a
 * library of its own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the XPSNR, motion, VIF, ADM, scene and CAMBI
 * libraries.
 *
 * The definition is DESIGN.md section 14 (Andersson et al., "FLIP: A Difference Evaluator for Alternating Images", HPG 2020, for
 * low-dynamic-range pictures): two sRGB pictures -> YCxCz -> contrast-sensitivity filters at `ppd` pixels per degree -> Hunt-adjusted
 * Lab -> HyAB colour difference, redistributed (dEc); edge and point detectors on the achromatic channel (dEf); FLIP = dEc^(1 - dEf), a
 * per-pixel map in [0, 1] whose mean is the score.  Parity with NVIDIA's tool is believed and unpinned.
 *
 * Use:  tm_flip_create -> per batch: tm_flip_set_pair (slots 0 .. n-1) -> tm_flip_compute_async(n) -> tm_flip_sync -> tm_flip_get;
 *       tm_flip_get_map for the maps of a computed slot.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_FLIP_H
#define TURBO_METRICS_FLIP_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* layouts:  TM_FLIP_RGB8   packed R, G, B bytes, sRGB, rows `pitch` >= 3 w bytes apart, any alignment */
enum { TM_FLIP_RGB8 = 0 };
/* maps of tm_flip_get_map: FLIP itself, the colour difference dEc, the feature difference dEf */
enum { TM_FLIP_MAP = 0, TM_FLIP_MAP_COLOR = 1, TM_FLIP_MAP_FEATURE = 2 };

/* 0.7 * 3840 / 0.7 * pi / 180: a 0.7 m wide 3840-pixel monitor seen from 0.7 m */
#define TM_FLIP_DEFAULT_PPD 67.02064327658226
/* the largest filter radius a tile's halo holds: a ppd whose spatial radius (tm_flip_radius) is above it -- every ppd above
 * 10 / (3 sqrt(0.04 / (2 pi^2))) = 74.048 -- is TM_ERR_UNSUPPORTED */
#define TM_FLIP_MAX_RADIUS 10

typedef struct tm_flip tm_flip;

/* one pair's result: the mean of the FLIP map (an f64 sum in a fixed order over w h: two computes give identical bits), its smallest
 * and largest value */
typedef struct tm_flip_frame {
    double mean, min, max;
} tm_flip_frame;

/* On the current HIP device.  w, h: picture size, 1 x 1 and up; ppd: pixels per degree, 8 .. 256, or 0 for TM_FLIP_DEFAULT_PPD;
 * batch_capacity: slots.  TM_ERR_INVALID_ARG (checked first): null out, a batch of 0 or above 65535; TM_ERR_UNSUPPORTED (before any device call): w or
 * h of 0, w h above 2^31, a layout other than TM_FLIP_RGB8, a ppd outside 8 .. 256 or one whose spatial radius is above
 * TM_FLIP_MAX_RADIUS. */
int tm_flip_create(tm_flip **out, uint32_t w, uint32_t h, int layout, double ppd, uint32_t batch_capacity);
void tm_flip_destroy(tm_flip *f);
/* bytes of device and page-locked host memory the library holds */
size_t tm_flip_mem_usage(const tm_flip *f);
/* The pair of slot `slot`.  mem: TM_MEM_HOST is copied before the call returns; TM_MEM_DEVICE is read in place by the kernel, on the
 * library's own non-blocking stream with no ordering against the stream that produced the surface: it must be complete before
 * tm_flip_compute_async and stay valid until tm_flip_sync returns.  Every compute consumes its slots' pairs: slots [0, n) are set
 * again before each tm_flip_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_flip_set_pair(tm_flip *f, uint32_t slot, const void *ref, size_t ref_pitch, const void *dis, size_t dis_pitch, int mem);
int tm_flip_compute_async(tm_flip *f, uint32_t n_slots);
int tm_flip_sync(tm_flip *f);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_flip_get(tm_flip *f, uint32_t first_slot, uint32_t n, tm_flip_frame *out);
/* one map of slot `slot` of the last compute, w x h floats, rows `pitch` bytes apart in host memory (synchronises).  TM_ERR_STATE for a
 * slot the last compute did not cover; TM_ERR_INVALID_ARG for another kind, a pitch below a row or not a multiple of 4 */
int tm_flip_get_map(tm_flip *f, uint32_t slot, int kind, float *out, size_t pitch);

/* host function of the definition: the radii of the spatial filter, ceil(3 sqrt(0.04 / (2 pi^2)) ppd), and of the feature filters,
 * ceil(3 * 0.5 * 0.082 ppd); (10, 9) at the default.  ppd 0: the default.  TM_ERR_INVALID_ARG: a null pointer, a ppd not above 0 or above 1e6 */
int tm_flip_radius(double ppd, uint32_t *r_spatial, uint32_t *r_feature);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_FLIP_H */
