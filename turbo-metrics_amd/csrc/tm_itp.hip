// tm_itp.hip -- host side of libturbometrics_itp.so (include/turbo_metrics_itp.h): frame upload, the two launches per batch and the
// host functions of the definition, in double.  Kernels: tm_itp_kernels.h (the load paths, the sums and the
// finish kernel are tm_ciede_kernels.h's); the host core it shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_itp.h"
#include "tm_itp_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMC_NV12 == TM_ITP_NV12 && TMC_P016 == TM_ITP_P016 && TMC_I420 == TM_ITP_I420 && TMC_I420P10 == TM_ITP_I420P10_PACKED, "layouts");
static_assert(TMI_PQ == TM_ITP_PQ && TMI_HLG == TM_ITP_HLG && TMI_TRANSFERS == 2, "transfers");

const double kMatrix[4] = TMI_MATRIX_VALUES;
const double kM1 = 2610.0 / 16384.0, kM2 = 2523.0 / 32.0, kC1 = 3424.0 / 4096.0, kC2 = 2413.0 / 128.0, kC3 = 2392.0 / 128.0;

double clamp01(double v) { return std::min(std::max(v, 0.0), 1.0); }

double hlg_scene(double e)
{
    const double a = 0.17883277, b = 1.0 - 4.0 * a, c = 0.5 - a * log(4.0 * a);
    return e <= 0.5 ? e * e / 3.0 : (exp((e - c) / a) + b) / 12.0;
}

} // namespace

#ifdef TM_EMULATE
// tests/host/itp_host_test.cpp compiles this file with a host compiler against a fake runtime, where nothing can be launched: the two
// launches are the test's own function
void tm_itp_host_test_launch(const TmItpGeom &g, unsigned n_slots, const TmCiedeDesc *desc, float *maps, TmCiedeCell *cells, TmCiedeCell *res);
#endif

struct tm_itp {
    TmItpGeom g;
    TmFeatureHost c;                                  // have, staging: [slot][side]
    TmCiedeDesc *d_desc = nullptr, *h_desc = nullptr; // [slot][side]; h_desc is page-locked, copied at each compute
    std::vector<TmCiedeDesc> desc;                    // what set_frame wrote
    float *d_maps = nullptr;                          // want_map: [slot][h][w]: every value is written by every compute
    TmCiedeCell *d_cells = nullptr;                   // [slot][g.b.cells]: likewise
    TmCiedeCell *d_res = nullptr, *h_res = nullptr;   // [slot]
};

namespace {

// bytes of one luma / chroma row of this layout, and the number of chroma planes
void plane_rows(const tm_itp *x, size_t *row_y, size_t *row_c, int *nc)
{
    const TmCiedeGeom &g = x->g.b;
    const size_t bps = g.bits == 8 ? 1 : 2;
    switch (g.layout) {
    case TM_ITP_NV12: case TM_ITP_P016: *row_y = g.w * bps; *row_c = 2 * (size_t)g.cw * bps; *nc = 1; break;
    case TM_ITP_I420: *row_y = g.w * bps; *row_c = g.cw * bps; *nc = 2; break;
    default: *row_y = (size_t)tm_p10_row_words(g.w) * 4; *row_c = (size_t)tm_p10_row_words(g.cw) * 4; *nc = 2; break;
    }
}

} // namespace

extern "C" {

double tm_itp_pq_eotf(double signal)
{
    const double p = pow(clamp01(signal), 1.0 / kM2);
    return 10000.0 * pow(std::max(p - kC1, 0.0) / (kC2 - kC3 * p), 1.0 / kM1);
}

double tm_itp_pq_inv_eotf(double light)
{
    const double y = pow(std::min(std::max(light, 0.0), 10000.0) / 10000.0, kM1);
    return pow((kC1 + kC2 * y) / (1.0 + kC3 * y), kM2);
}

int tm_itp_hlg_display(const double signal[3], double out[3])
{
    if (!signal || !out) return TM_ERR_INVALID_ARG;
    const double R = hlg_scene(clamp01(signal[0])), G = hlg_scene(clamp01(signal[1])), B = hlg_scene(clamp01(signal[2]));
    const double ys = 0.2627 * R + 0.6780 * G + 0.0593 * B;
    const double k = ys > 0.0 ? 1000.0 * pow(ys, 0.2) : 0.0;
    out[0] = k * R; out[1] = k * G; out[2] = k * B;
    return TM_OK;
}

int tm_itp_ictcp(uint32_t y, uint32_t u, uint32_t v, uint32_t bits, int transfer, double out[3])
{
    if (!out || transfer < 0 || transfer >= TMI_TRANSFERS) return TM_ERR_INVALID_ARG;
    if (bits < 8 || bits > 16) return TM_ERR_UNSUPPORTED;
    const double s = (double)(1u << (bits - 8));
    const double *c = kMatrix;
    const double yn = ((double)y - 16.0 * s) / (219.0 * s), un = ((double)u - 128.0 * s) / (224.0 * s), vn = ((double)v - 128.0 * s) / (224.0 * s);
    const double e[3] = {clamp01(yn + c[0] * vn), clamp01(yn - c[1] * un - c[2] * vn), clamp01(yn + c[3] * un)};
    double f[3];
    if (transfer == TM_ITP_HLG) tm_itp_hlg_display(e, f);
    else for (int k = 0; k < 3; ++k) f[k] = tm_itp_pq_eotf(e[k]);
    const double L = tm_itp_pq_inv_eotf((1688.0 * f[0] + 2146.0 * f[1] + 262.0 * f[2]) / 4096.0);
    const double M = tm_itp_pq_inv_eotf((683.0 * f[0] + 2951.0 * f[1] + 462.0 * f[2]) / 4096.0);
    const double S = tm_itp_pq_inv_eotf((99.0 * f[0] + 309.0 * f[1] + 3688.0 * f[2]) / 4096.0);
    out[0] = (L + M) / 2.0;
    out[1] = (6610.0 * L - 13613.0 * M + 7003.0 * S) / 4096.0;
    out[2] = (17933.0 * L - 17390.0 * M - 543.0 * S) / 4096.0;
    return TM_OK;
}

double tm_itp_de(const double a[3], const double b[3])
{
    if (!a || !b) return NAN;
    const double di = b[0] - a[0], dt = (b[1] - a[1]) / 2.0, dp = b[2] - a[2];
    return 720.0 * sqrt(di * di + dt * dt + dp * dp);
}

int tm_itp_create(tm_itp **out, uint32_t w, uint32_t h, int layout, uint32_t bits, int transfer, int full_range, int want_map,
                  uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    if (full_range) return TM_ERR_UNSUPPORTED;
    TmItpGeom gi;
    if (tmi_make_geom(&gi, w, h, layout, bits, transfer)) return TM_ERR_UNSUPPORTED;
    if (transfer < 0 || transfer >= TMI_TRANSFERS) return TM_ERR_INVALID_ARG;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launch's grid y
    tm_itp *x = new tm_itp();
    x->g = gi;
    const TmCiedeGeom &g = x->g.b;
    const size_t B = batch_capacity;
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&x->c, batch_capacity, B * 2, B * 2))) { delete x; return rc; }
    if ((rc = tmfh_dev_alloc(&x->c, &x->d_desc, B * 2 * sizeof(TmCiedeDesc))) ||
        (want_map && (rc = tmfh_dev_alloc(&x->c, &x->d_maps, B * (size_t)g.w * g.h * sizeof(float)))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_cells, B * g.cells * sizeof(TmCiedeCell))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_res, B * sizeof(TmCiedeCell))) ||
        (rc = tmfh_pinned_alloc(&x->c, &x->h_desc, B * 2 * sizeof(TmCiedeDesc))) ||
        (rc = tmfh_pinned_alloc(&x->c, &x->h_res, B * sizeof(TmCiedeCell)))) {
        tm_itp_destroy(x);
        return rc;
    }
    x->desc.assign(B * 2, TmCiedeDesc{});
    *out = x;
    return TM_OK;
}

void tm_itp_destroy(tm_itp *x)
{
    if (!x) return;
    tmfh_close(&x->c, {x->d_desc, x->d_maps, x->d_cells, x->d_res}, {x->h_desc, x->h_res});
    delete x;
}

size_t tm_itp_mem_usage(const tm_itp *x) { return x ? x->c.bytes : 0; }

int tm_itp_set_frame(tm_itp *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y, size_t pitch_uv,
                     int mem)
{
    if (!x || slot >= x->c.cap || (side != TM_SIDE_REF && side != TM_SIDE_DIS) || !y || !u) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const TmCiedeGeom &g = x->g.b;
    const bool biplanar = g.layout == TM_ITP_NV12 || g.layout == TM_ITP_P016;
    if (biplanar) v = nullptr;
    else if (!v) return TM_ERR_INVALID_ARG;
    size_t row_y, row_c;
    int nc;
    plane_rows(x, &row_y, &row_c, &nc);
    if (pitch_y < row_y || pitch_uv < row_c) return TM_ERR_INVALID_ARG;
    const size_t align = g.layout == TM_ITP_I420P10_PACKED ? 4 : (g.bits == 8 ? 1 : 2);
    if (((uintptr_t)y | (uintptr_t)u | (uintptr_t)v | pitch_y | pitch_uv) & (align - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    // not for TM_MEM_DEVICE: the staging surface may still be read; a device surface is only noted in a host-side descriptor
    if (mem != TM_MEM_DEVICE && (rc = tmfh_sync(&x->c))) return rc;
    TMFH_CHK(hipSetDevice(x->c.device));
    const size_t idx = (size_t)slot * 2 + side;
    const void *p[3] = {y, u, v};
    unsigned long long pitch[2] = {pitch_y, pitch_uv};
    if (mem != TM_MEM_DEVICE) {
        if ((rc = tmfh_upload_420(&x->c, idx, y, u, v, pitch_y, pitch_uv, row_y, row_c, g.h, g.ch, nc, p, pitch))) return rc;
        if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(x->c.stream));
    }
    TmCiedeDesc d{};
    d.p0 = p[0]; d.p1 = p[1]; d.p2 = p[2]; d.pitch = pitch[0]; d.pitch2 = pitch[1];
    d.vec = tmfh_vec((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2);
    x->desc[idx] = d;
    x->c.have[idx] = 1;
    return TM_OK;
}

int tm_itp_compute_async(tm_itp *x, uint32_t n_slots)
{
    if (!x) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&x->c, n_slots, 2);
    if (rc) return rc;
    hipStream_t stream = x->c.stream;
    memcpy(x->h_desc, x->desc.data(), 2 * n_slots * sizeof(TmCiedeDesc));
    TMFH_CHK(hipMemcpyAsync(x->d_desc, x->h_desc, 2 * n_slots * sizeof(TmCiedeDesc), hipMemcpyHostToDevice, stream));
    const TmItpGeom gi = x->g;
#ifdef TM_EMULATE
    tm_itp_host_test_launch(gi, n_slots, x->d_desc, x->d_maps, x->d_cells, x->d_res);
#else
    const TmCiedeGeom g = gi.b;
    const dim3 grid(g.cells, n_slots), block(TMC_THREADS);
#define TMI_LAUNCH(L, F) k_itp<L, F><<<grid, block, 0, stream>>>(gi, x->d_desc, x->d_maps, x->d_cells)
    TMC_DISPATCH(g, TMI_LAUNCH);
#undef TMI_LAUNCH
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    k_ciede_finish<<<dim3(n_slots), block, 0, stream>>>(g, x->d_cells, x->d_res);
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
#endif
    TMFH_CHK_QUEUED(&x->c, hipMemcpyAsync(x->h_res, x->d_res, n_slots * sizeof(TmCiedeCell), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&x->c, n_slots, 2);
    return TM_OK;
}

int tm_itp_sync(tm_itp *x) { return x ? tmfh_sync(&x->c) : TM_ERR_INVALID_ARG; }

int tm_itp_get(tm_itp *x, uint32_t first_slot, uint32_t n, tm_itp_frame *out)
{
    if (!x || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&x->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    const uint64_t px = (uint64_t)x->g.b.w * x->g.b.h;
    for (uint32_t i = 0; i < n; ++i) {
        const TmCiedeCell &r = x->h_res[first_slot + i];
        out[i].de_sum = r.sum;
        out[i].de_mean = r.sum / (double)px;
        out[i].de_max = (double)r.max;
        out[i].pixels = px;
    }
    return TM_OK;
}

int tm_itp_get_map(tm_itp *x, uint32_t slot, float *dst, size_t pitch)
{
    if (!x || !dst) return TM_ERR_INVALID_ARG;
    const TmCiedeGeom &g = x->g.b;
    if (pitch < (size_t)g.w * sizeof(float) || (pitch & 3)) return TM_ERR_INVALID_ARG;
    if (!x->d_maps || slot >= x->c.n_last) return TM_ERR_STATE;
    const int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    TMFH_CHK(hipSetDevice(x->c.device));
    const float *src = x->d_maps + (size_t)slot * g.w * g.h;
    TMFH_CHK(hipMemcpy2D(dst, pitch, src, (size_t)g.w * sizeof(float), (size_t)g.w * sizeof(float), g.h, hipMemcpyDeviceToHost));
    return TM_OK;
}

} // extern "C"
