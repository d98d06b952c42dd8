/*
 * turbo_metrics_siti.h -- C ABI of ITU-T P.910 spatial and temporal information (SI / TI) on the MI355X (gfx950):
 * libturbometrics_siti.so, a library of its own beside libturbometrics_hip.so (the SSIMULACRA2 / PSNR engine) and the other
 * feature libraries.
 *
 * SI and TI say how hard ONE stream is to code: SI is the standard deviation of the Sobel magnitude of a luma picture, TI the
 * standard deviation of the difference between a luma picture and the previous one.  The definition this library computes is
 * stated in DESIGN.md section 19.  Everything the device produces is an exact integer: per picture S1 = sum q and S2 = sum q^2 over
 * the (w - 2)(h - 2) interior positions, q the Sobel magnitude quantised to the nearest integer on the 16-bit scale, and T1 = sum d,
 * T2 = sum d^2 of the frame difference d over all w h positions.  The two host functions below turn the sums into SI and TI on the
 * 8-bit scale.  Range handling (gain) is believed to match P.910 (2023) / siti-tools for SDR and is unpinned; PQ / HLG modes are
 * not offered.  Only luma is read.  It is stateful: a picture is compared with the previous picture of the sequence, which the
 * engine keeps across batches.  The first picture of a sequence has ti_valid = 0, T1 = T2 = 0 and ti = 0.
 *
 * Use:  tm_siti_create -> per batch: tm_siti_set_frame (slots 0 .. n-1) -> tm_siti_compute_async(n) -> tm_siti_sync ->
 *       tm_siti_get.  Slots 0 .. n-1 of a batch are the next n pictures of the sequence, in order.  tm_siti_reset starts a
 *       new sequence.  One compute at a time: compute_async while one is in flight is TM_ERR_STATE.
 *
 * Plain C99; return codes and memory kinds are those of turbo_metrics_hip.h.
 */
#ifndef TURBO_METRICS_SITI_H
#define TURBO_METRICS_SITI_H

#include <stddef.h>
#include <stdint.h>

#include "turbo_metrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* luma layouts (the sample values and bit depth D the metric sees):
 *   TM_SITI_Y8             bytes; D = 8
 *   TM_SITI_Y16_MSB        16-bit words, the value in the HIGH bits: sample = v >> (16 - D); D = 9 .. 16 (the luma of P010 / P016)
 *   TM_SITI_Y16_LOW        16-bit little-endian words, the value in the LOW D bits, higher bits ignored; D = 9 .. 16
 *   TM_SITI_Y10_PACKED     the packed 10-bit upload layout of tm_engine_set_frame_i420p10; D = 10 */
enum { TM_SITI_Y8 = 0, TM_SITI_Y16_MSB = 1, TM_SITI_Y16_LOW = 2, TM_SITI_Y10_PACKED = 3 };

typedef struct tm_siti tm_siti;

/* one picture's result: the exact sums, and SI / TI of them at gain 1 */
typedef struct tm_siti_frame {
    uint64_t s1, s2; /* sum q, sum q^2 over the (w - 2)(h - 2) interior positions; q on the 16-bit scale */
    int64_t t1;      /* sum d over the w h positions, d = this picture - the previous one, in code values */
    uint64_t t2;     /* sum d^2 */
    int ti_valid;    /* 0 for the first picture of a sequence: t1 = t2 = 0, ti = 0 */
    double si, ti;   /* tm_siti_si / tm_siti_ti of the sums at gain 1 */
} tm_siti_frame;

/* On the current HIP device.  w, h: luma size; bits: D; batch_capacity: slots.  TM_ERR_INVALID_ARG: null out, zero batch;
 * TM_ERR_UNSUPPORTED (before any device call): w or h below 3, w h above 2^26, D outside 8 .. 16 or not one the layout carries. */
int tm_siti_create(tm_siti **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity);
void tm_siti_destroy(tm_siti *m);
/* bytes of device and page-locked host memory the engine holds */
size_t tm_siti_mem_usage(const tm_siti *m);
/* The picture of slot `slot`.  y: the luma plane, pitch_y: bytes per row.  mem: TM_MEM_HOST is copied before the call returns;
 * TM_MEM_HOST_PINNED is an asynchronous DMA, the bytes must stay valid until tm_siti_sync returns; TM_MEM_DEVICE is read in place
 * by the kernel (zero copy), with the same rule.  The kernel runs on the library's own non-blocking stream, with no ordering
 * against the stream that produced a device surface: it must be complete before tm_siti_compute_async.  Every compute consumes
 * its slots' pictures: slots [0, n) are set again before each tm_siti_compute_async(n) (otherwise TM_ERR_STATE). */
int tm_siti_set_frame(tm_siti *m, uint32_t slot, const void *y, size_t pitch_y, int mem);
/* slots [0, n_slots) continue the sequence */
int tm_siti_compute_async(tm_siti *m, uint32_t n_slots);
int tm_siti_sync(tm_siti *m);
/* results of slots [first_slot, first_slot + n) of the last compute (synchronises if it is still in flight) */
int tm_siti_get(tm_siti *m, uint32_t first_slot, uint32_t n, tm_siti_frame *out);
/* the next compute starts a new sequence */
int tm_siti_reset(tm_siti *m);

/* host functions of the definition: population standard deviations on the 8-bit scale.  The radicand n S2 - S1^2 is formed exactly
 * in 128-bit integers and converted to double once.  gain 1 takes the code values as they are (classic P.910); gain 255 / 219 is the
 * linear limited-to-full-range stretch, without clipping.  n of 0 gives 0. */
/* gain sqrt(n_si s2 - s1^2) / n_si / 256, n_si = (w - 2)(h - 2) */
double tm_siti_si(uint64_t s1, uint64_t s2, uint64_t n_si, double gain);
/* gain sqrt(n t2 - t1^2) / n / 2^(bits - 8), n = w h */
double tm_siti_ti(int64_t t1, uint64_t t2, uint64_t n, uint32_t bits, double gain);

#ifdef __cplusplus
}
#endif

#endif /* TURBO_METRICS_SITI_H */
