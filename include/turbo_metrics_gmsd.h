/*
 * turbo_metrics_gmsd.h -- C ABI of GMSD, the gradient magnitude similarity deviation (Xue, Zhang, Mou, Bovik, IEEE TIP 2014) on the
 * MI355X (gfx950): libturbometrics_gmsd.so, a library of its own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the
 * other feature libraries.
 *
 * Both luma planes of a pair are averaged over 2x2 samples and decimated by two; the Prewitt gradient magnitudes m_r, m_d of the two
 * decimated planes give, per decimated position, the gradient magnitude similarity GMS = (2 m_r m_d + c) / (m_r^2 + m_d^2 + c).  GMSD is
 * the standard deviation of GMS over the picture (0: identical), its mean is reported as gmsm.  The definition this library computes is
 * stated in DESIGN.md section 20: exact integers up to one f32 expression per position, which is e = 1 - GMS =
 * (m_r - m_d)^2 / (m_r^2 + m_d^2 + c), then f64 sums of e and e^2 in a fixed order; recalled from the paper and the authors' GMSD.m,
 * believed to match, unpinned against MATLAB.  c is the paper's 170 on the 0 .. 255 scale at every depth.  Only luma is read.  There is
 * no state between pairs.
 *
 * Use:  tm_gmsd_create -> per batch: tm_gmsd_set_pair (slots 0 .. n-1) -> tm_gmsd_compute_async(n) -> tm_gmsd_sync -> tm_gmsd_get /
 *       tm_gmsd_map.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_GMSD_H
#define TURBO_METRICS_GMSD_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the sample values and bit depth b the metric sees), numbered as in turbo_metrics_hvs.h:
 *   TM_GMSD_Y8             bytes; b = 8
 *   TM_GMSD_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - b); b = 9 .. 16 (the luma of P010 / P016)
 *   TM_GMSD_Y16_LOW        16-bit little-endian words, the value in the LOW b bits, higher bits ignored; b = 9 .. 16
 *   TM_GMSD_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; b = 10 */
enum { TM_GMSD_Y8 = 0, TM_GMSD_Y16_MSB = 1, TM_GMSD_Y16_LOW = 2, TM_GMSD_Y10_PACKED = 3 };

/* tm_gmsd_create flags */
enum { TM_GMSD_MAPS = 1 }; /* keep every slot's GMS map for tm_gmsd_map */

typedef struct tm_gmsd tm_gmsd;

/* one pair's result: E1 = sum e and E2 = sum e^2 over the n = ceil(w / 2) ceil(h / 2) decimated positions (e = 1 - GMS, DESIGN.md
 * section 20) and the largest e */
typedef struct tm_gmsd_frame {
    double e1, e2;
    float e_max;
    uint64_t n;
} tm_gmsd_frame;

/* On the current HIP device.  w, h: luma size; bits: b; batch_capacity: slots; flags: 0 or TM_GMSD_MAPS.  TM_ERR_INVALID_ARG: null out,
 * zero batch, more than 65535 slots, an unknown flag; TM_ERR_UNSUPPORTED (before any device call): w or h below 4 or above 32768, b
 * outside 8 .. 16 or not one the layout carries. */
int tm_gmsd_create(tm_gmsd **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity, uint32_t flags);
void tm_gmsd_destroy(tm_gmsd *g);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_gmsd_mem_usage(const tm_gmsd *g);
/* The pair of slot `slot`.  ref_y, dis_y: the luma planes, pitch_*: bytes per row.  mem (both planes): TM_MEM_HOST is copied before
 * the call returns; TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_gmsd_sync returns; TM_MEM_DEVICE is
 * read in place by the kernel (zero copy), with the same rule.  The kernels run on the library's own non-blocking stream, with no
 * ordering against the stream that produced a device surface: it must be complete before tm_gmsd_compute_async.  A pending compute is
 * waited for first.  Every compute consumes its slots' pairs: slots [0, n) are set again before each tm_gmsd_compute_async(n)
 * (otherwise TM_ERR_STATE). */
int tm_gmsd_set_pair(tm_gmsd *g, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem);
int tm_gmsd_compute_async(tm_gmsd *g, uint32_t n_slots);
int tm_gmsd_sync(tm_gmsd *g);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_gmsd_get(tm_gmsd *g, uint32_t first_slot, uint32_t n, tm_gmsd_frame *out);
/* The GMS map (GMS = 1 - e) of slot `slot` of the last compute into host memory: ceil(h / 2) rows of ceil(w / 2) floats, pitch: bytes
 * per row of dst (at least 4 ceil(w / 2), a multiple of 4).  Synchronises.  TM_ERR_STATE: created without TM_GMSD_MAPS, or a slot the
 * last compute did not cover. */
int tm_gmsd_map(tm_gmsd *g, uint32_t slot, float *dst, size_t pitch);

/* host functions of the definition (double).
 * tm_gmsd_score: GMSD = sqrt(max(0, (e2 - e1^2 / n) / (n - 1))), the sample standard deviation of GMS (MATLAB's std2); population != 0
 * divides by n instead.  tm_gmsd_mean: 1 - e1 / n, the mean GMS (gmsm).  NaN for n < 2.  A sequence's value is the same functions of the
 * summed e1, e2 and n of its pairs: pooled over all positions of all pairs. */
double tm_gmsd_score(double e1, double e2, uint64_t n, int population);
double tm_gmsd_mean(double e1, uint64_t n);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_GMSD_H */
