/*
 * turbo_metrics_yuv.h -- C ABI of plane-wise YUV PSNR and SSIM on the MI355X (gfx950): libturbometrics_yuv.so, a library of its own
 * beside libturbometrics_hip.so, like libturbometrics_xpsnr.so.
 *
 * The two numbers every video tool prints: PSNR per plane on the coded samples (psnr_y / psnr_u / psnr_v / average, as ffmpeg's
 * `psnr` filter and libvmaf's `psnr`) and the SSIM of x264 / ffmpeg's `ssim` filter per plane (Y / U / V / All).  The definition
 * this library computes is stated in DESIGN.md section 15 (believed to match ffmpeg vf_psnr / vf_ssim, x264 and libvmaf; unpinned).
 * It works on the integer samples of 4:2:0 pictures; no colour conversion.  The chroma planes are (w + 1) / 2 x (h + 1) / 2.  It is
 * stateless: a pair's result depends on the pair alone.
 *
 * Use:  tm_yuv_create -> per batch: tm_yuv_set_frame (both sides of slots 0 .. n-1) -> tm_yuv_compute_async(n) -> tm_yuv_sync ->
 *       tm_yuv_get / tm_yuv_get_ssim_map.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes, sides and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_YUV_H
#define TURBO_METRICS_YUV_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* picture layouts (the sample values and bit depth D the metric sees): those of turbo_metrics_xpsnr.h
 *   TM_YUV_NV12              8-bit luma plane + interleaved CbCr plane (u = CbCr, v = NULL); D = 8
 *   TM_YUV_P016              16-bit luma + interleaved CbCr, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (10: P010)
 *   TM_YUV_I420              three planes; D = 8: bytes, D = 9 .. 16: 16-bit little-endian words, the value in the LOW D bits
 *   TM_YUV_I420P10_PACKED    three planes of the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_YUV_NV12 = 0, TM_YUV_P016 = 1, TM_YUV_I420 = 2, TM_YUV_I420P10_PACKED = 3 };

typedef struct tm_yuv tm_yuv;

/* one pair's result per plane Y, Cb, Cr: the sum of squared differences over every sample; the SSIM (ssim_sum / windows); the f64 sum
 * of the plane's window values */
typedef struct tm_yuv_frame {
    uint64_t sse[3];
    double ssim[3];
    double ssim_sum[3];
} tm_yuv_frame;

/* On the current HIP device.  w, h: luma size; bits: D; batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch;
 * TM_ERR_UNSUPPORTED (before any device call): w or h below 16 (a chroma plane needs one SSIM window) or above 32768, D outside
 * 8 .. 16 or not one the layout carries. */
int tm_yuv_create(tm_yuv **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity);
void tm_yuv_destroy(tm_yuv *x);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_yuv_mem_usage(const tm_yuv *x);
/* One picture of slot `slot`.  y, u, v: the planes (NV12 / P016: u = CbCr, v ignored); pitch_y / pitch_uv: bytes per luma / chroma row.  mem: TM_MEM_HOST is
 * copied before the call returns; TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_yuv_sync returns;
 * TM_MEM_DEVICE is read in place by the kernels (zero copy), with the same rule.  While a compute is in flight, a host or pinned picture
 * waits for it first (its staging surface may still be read); a device picture does not.  The kernels run on the library's own non-blocking
 * stream, with no ordering against the stream that produced a device surface: it must be complete before tm_yuv_compute_async.
 * Every compute consumes its slots' pictures: both sides of slots [0, n) are set again before each tm_yuv_compute_async(n)
 * (otherwise TM_ERR_STATE). */
int tm_yuv_set_frame(tm_yuv *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y,
                     size_t pitch_uv, int mem);
int tm_yuv_compute_async(tm_yuv *x, uint32_t n_slots);
int tm_yuv_sync(tm_yuv *x);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_yuv_get(tm_yuv *x, uint32_t first_slot, uint32_t n, tm_yuv_frame *out);
/* the window values of plane `plane` (0 Y, 1 Cb, 2 Cr) of slot `slot` of the last compute, the x264 SSIM error map: mh rows of mw
 * floats (tm_yuv_map_size) into host memory, `pitch` bytes per row (at least 4 mw, a multiple of 4).  Synchronises. */
int tm_yuv_get_ssim_map(tm_yuv *x, uint32_t slot, int plane, float *dst, size_t pitch);

/* host functions of the definition */
/* bits outside 8 .. 16: NaN.  sse = 0: +inf (cap > 0: cap).  Otherwise, in double: max = 2^bits - 1; 10 * log10(((max * max) * (double)n_samples) / (double)sse); cap > 0:
 * the smaller of that and cap (libvmaf: cap = 6 bits + 12).  The "average" of a frame and the PSNR of a sequence are the PSNR of
 * the summed sse over the summed sample counts. */
double tm_yuv_psnr(uint64_t sse, uint64_t n_samples, uint32_t bits, double cap);
/* -10 log10(1 - s); +inf at s = 1 */
double tm_yuv_ssim_db(double s);
/* (n_y ssim_y + n_u ssim_u + n_v ssim_v) / (n_y + n_u + n_v) with the planes' sample counts of a w x h picture */
double tm_yuv_ssim_all(const double ssim[3], uint32_t w, uint32_t h);
/* size of a plane's SSIM map: mw = (pw >> 2) - 1, mh = (ph >> 2) - 1.  TM_ERR_INVALID_ARG: a plane outside 0 .. 2, null pointers;
 * TM_ERR_UNSUPPORTED: w or h below 16 */
int tm_yuv_map_size(uint32_t w, uint32_t h, int plane, uint32_t *mw, uint32_t *mh);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_YUV_H */
