/*
 * turbo_metrics_itp.h -- C ABI of the HDR colour difference dE ITP (ITU-R BT.2124) of 4:2:0 video on the MI355X (gfx950):
 * libturbometrics_itp.so, a library of its own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the other feature
 * libraries.
 *
 * At every luma position of a reference and a distorted picture: limited-range Y'CbCr -> BT.2020 non-constant-luminance R'G'B',
 * clamped to [0, 1] -> display light in cd/m2 (the PQ EOTF, or HLG on a 1000 cd/m2 display) -> LMS -> the PQ inverse EOTF -> ICtCp
 * (BT.2100) on both sides, then dE ITP = 720 sqrt(dI^2 + (dCt / 2)^2 + dCp^2): 1 is about one just-noticeable difference.  The chroma
 * of luma position (x, y) is the chroma sample (x >> 1, y >> 1): no interpolation.  The definition this library computes is stated in
 * full in DESIGN.md section 22.  There is no state between pairs and no derived score: BT.2124 defines none.
 *
 * Use:  tm_itp_create -> per batch: tm_itp_set_frame (both sides of slots 0 .. n-1) -> tm_itp_compute_async(n) -> tm_itp_sync ->
 *       tm_itp_get / tm_itp_get_map.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes, sides and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_ITP_H
#define TURBO_METRICS_ITP_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* picture layouts (the sample values and bit depth D the metric sees): those of turbo_metrics_yuv.h
 *   TM_ITP_NV12              8-bit luma plane + interleaved CbCr plane (u = CbCr, v = NULL); D = 8
 *   TM_ITP_P016              16-bit luma + interleaved CbCr, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (10: P010)
 *   TM_ITP_I420              three planes; D = 8: bytes, D = 9 .. 16: 16-bit little-endian words, the value in the LOW D bits
 *   TM_ITP_I420P10_PACKED    three planes of the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_ITP_NV12 = 0, TM_ITP_P016 = 1, TM_ITP_I420 = 2, TM_ITP_I420P10_PACKED = 3 };

/* the transfer function of the samples
 *   TM_ITP_PQ     BT.2100 PQ: the signal is absolute, 0 .. 10000 cd/m2
 *   TM_ITP_HLG    BT.2100 HLG shown on a display of nominal peak 1000 cd/m2 (system gamma 1.2) */
enum { TM_ITP_PQ = 0, TM_ITP_HLG = 1 };

typedef struct tm_itp tm_itp;

/* one pair's result: the f64 sum of dE ITP over all w h luma positions, de_sum / pixels, the largest dE ITP.  A sequence's mean is
 * the summed de_sum over the summed pixels. */
typedef struct tm_itp_frame {
    double de_sum, de_mean, de_max;
    uint64_t pixels;
} tm_itp_frame;

/* On the current HIP device.  w, h: luma size; bits: D; transfer: TM_ITP_PQ / TM_ITP_HLG; full_range: must be 0; want_map: nonzero
 * keeps a w x h f32 dE ITP map per slot (tm_itp_get_map); batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch, more than
 * 65535 slots, an unknown transfer; TM_ERR_UNSUPPORTED (before any device call): full range, w or h below 2 or above 32768, D outside
 * 8 .. 16 or not one the layout carries. */
int tm_itp_create(tm_itp **out, uint32_t w, uint32_t h, int layout, uint32_t bits, int transfer, int full_range, int want_map,
                  uint32_t batch_capacity);
void tm_itp_destroy(tm_itp *x);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_itp_mem_usage(const tm_itp *x);
/* One picture of slot `slot`.  y, u, v: the planes (NV12 / P016: u = CbCr, v ignored); pitch_y / pitch_uv: bytes per luma / chroma
 * row.  The chroma planes are (w + 1) / 2 x (h + 1) / 2.  mem: TM_MEM_HOST is copied before the call returns; TM_MEM_HOST_PINNED is
 * an asynchronous DMA, the bytes must stay valid until tm_itp_sync returns; TM_MEM_DEVICE is read in place by the kernel (zero
 * copy), with the same rule.  While a compute is in flight, a host or pinned picture waits for it first (its staging surface may
 * still be read); a device picture does not.  The kernels run on the library's own non-blocking stream, with no ordering against the
 * stream that produced a device surface: it must be complete before tm_itp_compute_async.  Every compute consumes its slots'
 * pictures: both sides of slots [0, n) are set again before each tm_itp_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_itp_set_frame(tm_itp *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y, size_t pitch_uv,
                     int mem);
int tm_itp_compute_async(tm_itp *x, uint32_t n_slots);
int tm_itp_sync(tm_itp *x);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_itp_get(tm_itp *x, uint32_t first_slot, uint32_t n, tm_itp_frame *out);
/* the dE ITP of every luma position of slot `slot` of the last compute: h rows of w floats into host memory, `pitch` bytes per row
 * (at least 4 w, a multiple of 4).  TM_ERR_STATE: created without want_map, or a slot the last compute did not cover.
 * Synchronises. */
int tm_itp_get_map(tm_itp *x, uint32_t slot, float *dst, size_t pitch);

/* host functions of the definition, in double */
/* one limited-range Y'CbCr triple of depth `bits` -> (I, Ct, Cp).  TM_ERR_INVALID_ARG: null out, an unknown transfer;
 * TM_ERR_UNSUPPORTED: bits outside 8 .. 16 */
int tm_itp_ictcp(uint32_t y, uint32_t u, uint32_t v, uint32_t bits, int transfer, double out[3]);
/* dE ITP of two (I, Ct, Cp) triples; NaN for a null argument */
double tm_itp_de(const double ictcp1[3], const double ictcp2[3]);
/* the PQ EOTF: signal (clamped to [0, 1]) -> cd/m2, and its inverse: cd/m2 (clamped to [0, 10000]) -> signal */
double tm_itp_pq_eotf(double signal);
double tm_itp_pq_inv_eotf(double light);
/* HLG R'G'B' signals (clamped to [0, 1]) -> the R, G, B display light in cd/m2 of a 1000 cd/m2 display.  TM_ERR_INVALID_ARG: null */
int tm_itp_hlg_display(const double signal[3], double out[3]);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_ITP_H */
