/*
 * turbo_metrics_haarpsi.h -- C ABI of HaarPSI, the Haar wavelet-based perceptual similarity index (Reisenhofer, Bosse, Kutyniok, Wiegand,
 * Signal Processing: Image Communication 2018) on the MI355X (gfx950): libturbometrics_haarpsi.so, a library of its own beside
 * libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the other feature libraries.
 *
 * The grayscale form, on luma.  Both luma planes of a pair are averaged over 2x2 samples and decimated by two; the Haar coefficients of
 * the two decimated planes at the scales 1 and 2 (windows of 2 and 4 positions), vertical and horizontal, give a local similarity per
 * position and orientation, (2 a d + C) / (a^2 + d^2 + C) averaged over the two scales with C = 30; a logistic with alpha = 4.2 maps it,
 * the larger magnitude of the two scale-3 coefficients (windows of 8) weights it, and the logit of the weighted mean, squared, is the
 * index: 1 for identical pictures, smaller for worse ones.  The definition this library computes is stated in DESIGN.md section 21:
 * exact integers up to one f32 expression per position and orientation, then the sums Q = sum q W (f64, fixed order) and WS = sum W
 * (exact); recalled from the paper and the authors' HaarPSI.m, believed to match, unpinned against MATLAB.  C is the paper's 30 on the
 * 0 .. 255 scale at every depth.  Only luma is read; the colour (YIQ) form is not computed.  There is no state between pairs.
 *
 * Use:  tm_haarpsi_create -> per batch: tm_haarpsi_set_pair (slots 0 .. n-1) -> tm_haarpsi_compute_async(n) -> tm_haarpsi_sync ->
 *       tm_haarpsi_get / tm_haarpsi_map.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_HAARPSI_H
#define TURBO_METRICS_HAARPSI_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the sample values and bit depth b the metric sees), numbered as in turbo_metrics_gmsd.h:
 *   TM_HAARPSI_Y8             bytes; b = 8
 *   TM_HAARPSI_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - b); b = 9 .. 16 (the luma of P010 / P016)
 *   TM_HAARPSI_Y16_LOW        16-bit little-endian words, the value in the LOW b bits, higher bits ignored; b = 9 .. 16
 *   TM_HAARPSI_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; b = 10 */
enum { TM_HAARPSI_Y8 = 0, TM_HAARPSI_Y16_MSB = 1, TM_HAARPSI_Y16_LOW = 2, TM_HAARPSI_Y10_PACKED = 3 };

/* tm_haarpsi_create flags */
enum { TM_HAARPSI_MAPS = 1 }; /* keep every slot's local similarity map for tm_haarpsi_map */

typedef struct tm_haarpsi tm_haarpsi;

/* one pair's result: Q = sum q_o W_o and WS = sum W_o over the ceil(w / 2) ceil(h / 2) decimated positions and the two orientations
 * (q_o = 1 - sigmoid(4.2 s_o), W_o the larger scale-3 magnitude in integer units) */
typedef struct tm_haarpsi_frame {
    double q;
    uint64_t ws;
} tm_haarpsi_frame;

/* On the current HIP device.  w, h: luma size; bits: b; batch_capacity: slots; flags: 0 or TM_HAARPSI_MAPS.  TM_ERR_INVALID_ARG: null
 * out, zero batch, more than 65535 slots, an unknown flag; TM_ERR_UNSUPPORTED (before any device call): w or h below 4 or above 32768, b
 * outside 8 .. 16 or not one the layout carries. */
int tm_haarpsi_create(tm_haarpsi **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity, uint32_t flags);
void tm_haarpsi_destroy(tm_haarpsi *p);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_haarpsi_mem_usage(const tm_haarpsi *p);
/* The pair of slot `slot`.  ref_y, dis_y: the luma planes, pitch_*: bytes per row.  mem (both planes): TM_MEM_HOST is copied before
 * the call returns; TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_haarpsi_sync returns; TM_MEM_DEVICE is
 * read in place by the kernel (zero copy), with the same rule.  The kernels run on the library's own non-blocking stream, with no
 * ordering against the stream that produced a device surface: it must be complete before tm_haarpsi_compute_async.  A pending compute is
 * waited for first.  Every compute consumes its slots' pairs: slots [0, n) are set again before each tm_haarpsi_compute_async(n)
 * (otherwise TM_ERR_STATE). */
int tm_haarpsi_set_pair(tm_haarpsi *p, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem);
int tm_haarpsi_compute_async(tm_haarpsi *p, uint32_t n_slots);
int tm_haarpsi_sync(tm_haarpsi *p);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_haarpsi_get(tm_haarpsi *p, uint32_t first_slot, uint32_t n, tm_haarpsi_frame *out);
/* The local similarity map of slot `slot` of the last compute into host memory: (s_v + s_h) / 2, the unweighted similarity in (0, 1],
 * ceil(h / 2) rows of ceil(w / 2) floats, pitch: bytes per row of dst (at least 4 ceil(w / 2), a multiple of 4).  Synchronises.
 * TM_ERR_STATE: created without TM_HAARPSI_MAPS, or a slot the last compute did not cover. */
int tm_haarpsi_map(tm_haarpsi *p, uint32_t slot, float *dst, size_t pitch);

/* host function of the definition (double): x = q / ws, HaarPSI = (log((1 - x) / x) / (double)4.2f)^2.  NaN for ws = 0 (both pictures
 * flat: MATLAB's 0 / 0).  A sequence's value is the same function of the summed q and ws of its pairs. */
double tm_haarpsi_score(double q, uint64_t ws);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_HAARPSI_H */
