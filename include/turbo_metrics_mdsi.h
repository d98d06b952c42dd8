/*
 * turbo_metrics_mdsi.h -- C ABI of MDSI, the mean deviation similarity index (Nafchi, Shahkolaei, Hedjam, Cheriet, IEEE Access 2016)
 * of 4:2:0 video on the MI355X (gfx950): libturbometrics_mdsi.so, a library of its own beside libturbometrics_hip.so (the
 * SSIMULACRA2 / PSNR engine) and the other feature libraries.
 *
 * Per pair of limited-range Y'CbCr pictures: the f x f box mean of R'G'B' (0 .. 255, not clipped; the chroma of luma position (x, y)
 * is the chroma sample (x >> 1, y >> 1)) at every f-th position, the planes L, H, M, the Prewitt gradient similarity GS of L between
 * the two pictures and their mean, the chromaticity similarity CS of H and M, GCS = 0.6 GS + 0.4 CS, z = GCS^(1/4) (the principal
 * complex root where GCS < 0), MAD = mean |z - mean z| and mdsi = MAD^(1/4): 0 for identical pictures, larger is worse.  The
 * definition this library computes is stated in full in DESIGN.md section 23 (recalled from the paper and the authors' MDSI.m,
 * believed to match, unpinned against MATLAB).  There is no state between pairs, and MDSI does not pool across pictures: a
 * sequence's value is the mean of its pairs' values.
 *
 * Use:  tm_mdsi_create -> per batch: tm_mdsi_set_frame (both sides of slots 0 .. n-1) -> tm_mdsi_compute_async(n) -> tm_mdsi_sync ->
 *       tm_mdsi_get / tm_mdsi_map.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes, sides and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_MDSI_H
#define TURBO_METRICS_MDSI_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* picture layouts (the sample values and bit depth D the metric sees): those of turbo_metrics_ciede.h
 *   TM_MDSI_NV12              8-bit luma plane + interleaved CbCr plane (u = CbCr, v = NULL); D = 8
 *   TM_MDSI_P016              16-bit luma + interleaved CbCr, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (10: P010)
 *   TM_MDSI_I420              three planes; D = 8: bytes, D = 9 .. 16: 16-bit little-endian words, the value in the LOW D bits
 *   TM_MDSI_I420P10_PACKED    three planes of the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_MDSI_NV12 = 0, TM_MDSI_P016 = 1, TM_MDSI_I420 = 2, TM_MDSI_I420P10_PACKED = 3 };

/* the Y'CbCr -> R'G'B' matrix, with the constants of turbo_metrics_ciede.h: R = y + c0 v, G = y - c1 u - c2 v, B = y + c3 u
 *   TM_MDSI_BT709        c = (1.5748, 0.187324, 0.468124, 1.8556)
 *   TM_MDSI_BT601        c = (1.402, 0.344136, 0.714136, 1.772)
 *   TM_MDSI_BY_HEIGHT    BT.709 for h >= 720, BT.601 below */
enum { TM_MDSI_BT709 = 0, TM_MDSI_BT601 = 1, TM_MDSI_BY_HEIGHT = 2 };

/* flags of tm_mdsi_create: TM_MDSI_MAPS lets tm_mdsi_map read the GCS map of a slot back (the map itself is always formed: the
 * second pooling pass reads it) */
enum { TM_MDSI_MAPS = 1 };

typedef struct tm_mdsi tm_mdsi;

/* one pair's result: the f64 sums of Re z and Im z over the n = ceil(w / f) ceil(h / f) positions, dev = the f64 sum of |z - mu| with
 * mu = (sum_re + i sum_im) / n, the number of positions with GCS < 0, and the factor f that was used.
 * MAD = dev / n, mdsi = tm_mdsi_score(dev, n). */
typedef struct tm_mdsi_frame {
    double sum_re, sum_im, dev;
    uint64_t n, negatives;
    uint32_t factor, pad_;
} tm_mdsi_frame;

/* On the current HIP device.  w, h: luma size; bits: D; matrix: TM_MDSI_BT709 ...; factor: f in 1 .. 128, or 0 for
 * max(1, round(min(w, h) / 256)) (halves away from zero); flags: TM_MDSI_MAPS or 0; batch_capacity: slots.  TM_ERR_INVALID_ARG: null
 * out, zero batch, more than 65535 slots, an unknown flag, an unknown matrix, a factor above 128; TM_ERR_UNSUPPORTED (before any
 * device call): w or h below 2 or above 32768, D outside 8 .. 16 or not one the layout carries, fewer than 4 decimated positions. */
int tm_mdsi_create(tm_mdsi **out, uint32_t w, uint32_t h, int layout, uint32_t bits, int matrix, uint32_t factor, uint32_t flags,
                   uint32_t batch_capacity);
void tm_mdsi_destroy(tm_mdsi *x);
/* bytes of device and page-locked host memory the object holds */
size_t tm_mdsi_mem_usage(const tm_mdsi *x);
/* the factor f the object uses: the forced one, or the automatic one of its picture size; 0 for NULL */
uint32_t tm_mdsi_get_factor(const tm_mdsi *x);
/* One picture of slot `slot`.  y, u, v: the planes (NV12 / P016: u = CbCr, v ignored); pitch_y / pitch_uv: bytes per luma / chroma
 * row.  The chroma planes are (w + 1) / 2 x (h + 1) / 2.  mem: TM_MEM_HOST is copied before the call returns; TM_MEM_HOST_PINNED is
 * an asynchronous DMA, the bytes must stay valid until tm_mdsi_sync returns; TM_MEM_DEVICE is read in place by the kernel (zero
 * copy), with the same rule.  While a compute is in flight, a host or pinned picture waits for it first (its staging surface may
 * still be read); a device picture does not.  The kernels run on the library's own non-blocking stream, with no ordering against the
 * stream that produced a device surface: it must be complete before tm_mdsi_compute_async.  Every compute consumes its slots'
 * pictures: both sides of slots [0, n) are set again before each tm_mdsi_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_mdsi_set_frame(tm_mdsi *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y, size_t pitch_uv,
                      int mem);
int tm_mdsi_compute_async(tm_mdsi *x, uint32_t n_slots);
int tm_mdsi_sync(tm_mdsi *x);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_mdsi_get(tm_mdsi *x, uint32_t first_slot, uint32_t n, tm_mdsi_frame *out);
/* the GCS of every decimated position of slot `slot` of the last compute: ceil(h / f) rows of ceil(w / f) floats into host memory,
 * `pitch` bytes per row (at least 4 ceil(w / f), a multiple of 4).  TM_ERR_STATE: created without TM_MDSI_MAPS, or a slot the last
 * compute did not cover.  Synchronises. */
int tm_mdsi_map(tm_mdsi *x, uint32_t slot, float *dst, size_t pitch);

/* host functions of the definition, in double */
/* mdsi = (dev / n)^(1/4); NaN for n = 0 */
double tm_mdsi_score(double dev, uint64_t n);
/* the automatic factor of a w x h picture */
uint32_t tm_mdsi_factor(uint32_t w, uint32_t h);
/* one limited-range Y'CbCr triple of depth `bits` -> (L, H, M) on the 0 .. 255 scale.  TM_ERR_INVALID_ARG: null out, an unknown matrix
 * (TM_MDSI_BY_HEIGHT has no height here and is refused); TM_ERR_UNSUPPORTED: bits outside 8 .. 16 */
int tm_mdsi_lhm(uint32_t y, uint32_t u, uint32_t v, int matrix, uint32_t bits, double out[3]);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_MDSI_H */
