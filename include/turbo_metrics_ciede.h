/*
 * turbo_metrics_ciede.h -- C ABI of CIEDE2000 of 4:2:0 video on the MI355X (gfx950): libturbometrics_ciede.so, a library of its own
 * beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the other feature libraries.
 *
 * The colour difference dE00 of Sharma, Wu and Dalal (2005) at every luma position of a reference and a distorted picture: limited
 * range Y'CbCr -> R'G'B' (no clamping) -> linear (the sRGB curve) -> XYZ -> CIE Lab (D65) on both sides, then dE00 with the
 * parametric factors kL, kC, kH.  The chroma of luma position (x, y) is the chroma sample (x >> 1, y >> 1): no interpolation.  The
 * definition this library computes is stated in full in DESIGN.md section 17; the dE00 formula is pinned by the 34 pairs the authors
 * published.  There is no state between pairs.
 *
 * Use:  tm_ciede_create -> per batch: tm_ciede_set_frame (both sides of slots 0 .. n-1) -> tm_ciede_compute_async(n) ->
 *       tm_ciede_sync -> tm_ciede_get / tm_ciede_get_map.  One compute at a time: compute_async while one is in flight is
 *       TM_ERR_STATE.
 *
 * Plain C99; return codes, sides and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_CIEDE_H
#define TURBO_METRICS_CIEDE_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* picture layouts (the sample values and bit depth D the metric sees): those of turbo_metrics_yuv.h
 *   TM_CIEDE_NV12              8-bit luma plane + interleaved CbCr plane (u = CbCr, v = NULL); D = 8
 *   TM_CIEDE_P016              16-bit luma + interleaved CbCr, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (10: P010)
 *   TM_CIEDE_I420              three planes; D = 8: bytes, D = 9 .. 16: 16-bit little-endian words, the value in the LOW D bits
 *   TM_CIEDE_I420P10_PACKED    three planes of the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_CIEDE_NV12 = 0, TM_CIEDE_P016 = 1, TM_CIEDE_I420 = 2, TM_CIEDE_I420P10_PACKED = 3 };

/* the Y'CbCr -> R'G'B' matrix: R = y + c0 v, G = y - c1 u - c2 v, B = y + c3 u
 *   TM_CIEDE_BT709      c = (1.5748, 0.187324, 0.468124, 1.8556)
 *   TM_CIEDE_BT601      c = (1.402, 0.344136, 0.714136, 1.772)
 *   TM_CIEDE_LIBVMAF    c = (1.28033, 0.21482, 0.38059, 2.12798): the constants libvmaf's `ciede` feature is recalled to use; recalled,
 *                       unpinned.  libvmaf is also recalled to use kL, kC, kH = 0.65, 1, 4 (likewise unpinned). */
enum { TM_CIEDE_BT709 = 0, TM_CIEDE_BT601 = 1, TM_CIEDE_LIBVMAF = 2 };

typedef struct tm_ciede tm_ciede;

/* one pair's result: the f64 sum of dE00 over all w h luma positions, de_sum / pixels, the largest dE00, and
 * tm_ciede_score(de_sum, pixels) */
typedef struct tm_ciede_frame {
    double de_sum, de_mean, de_max, score;
    uint64_t pixels;
} tm_ciede_frame;

/* On the current HIP device.  w, h: luma size; bits: D; matrix: TM_CIEDE_BT709 ...; kl, kc, kh: the parametric factors (1, 1, 1 is
 * the standard); full_range: must be 0; want_map: nonzero keeps a w x h f32 dE00 map per slot (tm_ciede_get_map);
 * batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch, more than 65535 slots, an unknown matrix, a factor that is not a
 * finite number above 0; TM_ERR_UNSUPPORTED (before any device call): full range, w or h below 2 or above 32768, D outside 8 .. 16 or
 * not one the layout carries. */
int tm_ciede_create(tm_ciede **out, uint32_t w, uint32_t h, int layout, uint32_t bits, int matrix, double kl, double kc, double kh,
                    int full_range, int want_map, uint32_t batch_capacity);
void tm_ciede_destroy(tm_ciede *x);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_ciede_mem_usage(const tm_ciede *x);
/* One picture of slot `slot`.  y, u, v: the planes (NV12 / P016: u = CbCr, v ignored); pitch_y / pitch_uv: bytes per luma / chroma
 * row.  The chroma planes are (w + 1) / 2 x (h + 1) / 2.  mem: TM_MEM_HOST is copied before the call returns; TM_MEM_HOST_PINNED is
 * an asynchronous DMA, the bytes must stay valid until tm_ciede_sync returns; TM_MEM_DEVICE is read in place by the kernel (zero
 * copy), with the same rule.  While a compute is in flight, a host or pinned picture waits for it first (its staging surface may
 * still be read); a device picture does not.  The kernels run on the library's own non-blocking stream, with no ordering against the
 * stream that produced a device surface: it must be complete before tm_ciede_compute_async.  Every compute consumes its slots'
 * pictures: both sides of slots [0, n) are set again before each tm_ciede_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_ciede_set_frame(tm_ciede *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y,
                       size_t pitch_uv, int mem);
int tm_ciede_compute_async(tm_ciede *x, uint32_t n_slots);
int tm_ciede_sync(tm_ciede *x);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_ciede_get(tm_ciede *x, uint32_t first_slot, uint32_t n, tm_ciede_frame *out);
/* the dE00 of every luma position of slot `slot` of the last compute: h rows of w floats into host memory, `pitch` bytes per row
 * (at least 4 w, a multiple of 4).  TM_ERR_STATE: created without want_map, or a slot the last compute did not cover.
 * Synchronises. */
int tm_ciede_get_map(tm_ciede *x, uint32_t slot, float *dst, size_t pitch);

/* host functions of the definition, in double */
/* dE00 of two Lab triples (L, a, b); NaN for a factor that is not above 0 */
double tm_ciede_de00(const double lab1[3], const double lab2[3], double kl, double kc, double kh);
/* one limited-range Y'CbCr triple of depth `bits` -> Lab.  TM_ERR_INVALID_ARG: null lab, an unknown matrix;
 * TM_ERR_UNSUPPORTED: bits outside 8 .. 16 */
int tm_ciede_lab(uint32_t y, uint32_t u, uint32_t v, int matrix, uint32_t bits, double lab[3]);
/* min(45 - 20 log10(de_sum / n), 100); 100 at de_sum = 0; NaN for n = 0.  A sequence's value is tm_ciede_score of the summed
 * de_sum and the summed pixel counts. */
double tm_ciede_score(double de_sum, uint64_t n);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_CIEDE_H */
