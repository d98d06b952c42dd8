/*
 * turbo_metrics_xpsnr.h -- C ABI of XPSNR on the MI355X (gfx950): libturbometrics_xpsnr.so, a library of its own beside
 * libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine), as the reference keeps XPSNR in crates of its own.
 *
 * XPSNR is the perceptually weighted PSNR of Helmrich et al., "XPSNR: A Low-Complexity Extension of the Perceptually Weighted
 * PSNR for Versatile Video Coding" (ICASSP 2020), the `xpsnr` filter of ffmpeg >= 7.0.  The definition this library computes is
 * stated in DESIGN.md section 8 (believed to match ffmpeg vf_xpsnr; unpinned).  It works on the integer samples of 4:2:0
 * pictures; no colour conversion.  It is stateful: the temporal activity of a picture needs the previous one (first order) or
 * two (second order) REFERENCE pictures of the sequence, which the engine keeps.  At the start of a sequence they are all zero.
 *
 * Use:  tm_xpsnr_create -> per batch: tm_xpsnr_set_frame (both sides of slots 0 .. n-1) -> tm_xpsnr_compute_async(n) ->
 *       tm_xpsnr_sync -> tm_xpsnr_get.  Slots 0 .. n-1 of a batch are the next n pictures of the sequence, in order.
 *       tm_xpsnr_reset starts a new sequence.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes, sides and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_XPSNR_H
#define TURBO_METRICS_XPSNR_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* picture layouts (the sample values and bit depth D the metric sees):
 *   TM_XPSNR_NV12              8-bit luma plane + interleaved CbCr plane (u = CbCr, v = NULL); D = 8
 *   TM_XPSNR_P016              16-bit luma + interleaved CbCr, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (10: P010)
 *   TM_XPSNR_I420              three planes; D = 8: bytes, D = 9 .. 16: 16-bit little-endian words, the value in the LOW D bits
 *   TM_XPSNR_I420P10_PACKED    three planes of the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_XPSNR_NV12 = 0, TM_XPSNR_P016 = 1, TM_XPSNR_I420 = 2, TM_XPSNR_I420P10_PACKED = 3 };

typedef struct tm_xpsnr tm_xpsnr;

/* one frame's result: the rounded weighted SSE and the XPSNR in dB of Y, Cb, Cr (+inf when the weighted SSE is 0) */
typedef struct tm_xpsnr_frame {
    uint64_t wsse[3];
    double xpsnr[3];
} tm_xpsnr_frame;

/* On the current HIP device.  w, h: luma size; bits: D; fps_num / fps_den: the frame rate (integer rate < 32: first-order temporal
 * activity, else second order); batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero w / h / fps / batch; TM_ERR_UNSUPPORTED
 * (before any device call): w or h below 8, D outside 8 .. 16 or not one the layout carries, odd w or h above 2048 x 1152 samples
 * (the downsampled high-pass works on 2x2 cells), pictures whose block size exceeds 256 (above about 4 x 3840 x 2160 samples). */
int tm_xpsnr_create(tm_xpsnr **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t fps_num, uint32_t fps_den,
                    uint32_t batch_capacity);
void tm_xpsnr_destroy(tm_xpsnr *x);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_xpsnr_mem_usage(const tm_xpsnr *x);
/* One picture of slot `slot`.  y, u, v: the planes (NV12 / P016: u = CbCr, v ignored); pitch_y / pitch_uv: bytes per luma / chroma row.  mem: TM_MEM_HOST is
 * copied before the call returns; TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_xpsnr_sync returns;
 * TM_MEM_DEVICE is read in place by the kernels (zero copy), with the same rule.  The kernels run on the library's own non-blocking
 * stream, with no ordering against the stream that produced a device surface: it must be complete before tm_xpsnr_compute_async.
 * Every compute consumes its slots' pictures: both sides of slots [0, n) are set again before each tm_xpsnr_compute_async(n)
 * (otherwise TM_ERR_STATE). */
int tm_xpsnr_set_frame(tm_xpsnr *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y,
                       size_t pitch_uv, int mem);
/* slots [0, n_slots) continue the sequence */
int tm_xpsnr_compute_async(tm_xpsnr *x, uint32_t n_slots);
int tm_xpsnr_sync(tm_xpsnr *x);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_xpsnr_get(tm_xpsnr *x, uint32_t first_slot, uint32_t n, tm_xpsnr_frame *out);
/* the next compute starts a new sequence (history all zero) */
int tm_xpsnr_reset(tm_xpsnr *x);

/* host functions of the definition */
uint32_t tm_xpsnr_block_size(uint32_t w, uint32_t h);   /* b = 4 (int)(32 sqrt(w h / (3840 * 2160)) + 0.5) */
/* 10 log10(plane_w plane_h (2^bits - 1)^2 / s^2), s = sqrt(wsse); +inf for wsse = 0 */
double tm_xpsnr_from_wsse(uint64_t wsse, uint32_t plane_w, uint32_t plane_h, uint32_t bits);
/* the sequence score: S = sum over frames of sqrt(wsse); S >= n: 10 log10(plane_w plane_h (2^bits - 1)^2 / (S / n)^2), else the
 * mean of the per-frame scores (sum_xpsnr / n) */
double tm_xpsnr_sequence(double sum_sqrt_wsse, double sum_xpsnr, uint64_t n_frames, uint32_t plane_w, uint32_t plane_h,
                         uint32_t bits);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_XPSNR_H */
