// tm_ciede.hip -- host side of libturbometrics_ciede.so (include/turbo_metrics_ciede.h): frame upload, the two launches per batch and
// the host functions of the definition, in double.  Kernels: tm_ciede_kernels.h; the host core it shares:
// tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_ciede.h"
#include "tm_ciede_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMC_NV12 == TM_CIEDE_NV12 && TMC_P016 == TM_CIEDE_P016 && TMC_I420 == TM_CIEDE_I420 && TMC_I420P10 == TM_CIEDE_I420P10_PACKED, "layouts");
static_assert(TM_CIEDE_BT709 == 0 && TM_CIEDE_BT601 == 1 && TM_CIEDE_LIBVMAF == 2 && TMC_MATRICES == 3, "matrices");

const double kMatrix[TMC_MATRICES][4] = TMC_MATRIX_VALUES;

} // namespace

struct tm_ciede {
    TmCiedeGeom g;
    TmFeatureHost c;                                  // have, staging: [slot][side]
    TmCiedeDesc *d_desc = nullptr, *h_desc = nullptr; // [slot][side]; h_desc is page-locked, copied at each compute
    std::vector<TmCiedeDesc> desc;                    // what set_frame wrote
    float *d_maps = nullptr;                          // want_map: [slot][h][w]: every value is written by every compute
    TmCiedeCell *d_cells = nullptr;                   // [slot][g.cells]: likewise
    TmCiedeCell *d_res = nullptr, *h_res = nullptr;   // [slot]
};

namespace {

// bytes of one luma / chroma row of this layout, and the number of chroma planes
void plane_rows(const tm_ciede *x, size_t *row_y, size_t *row_c, int *nc)
{
    const TmCiedeGeom &g = x->g;
    const size_t bps = g.bits == 8 ? 1 : 2;
    switch (g.layout) {
    case TM_CIEDE_NV12: case TM_CIEDE_P016: *row_y = g.w * bps; *row_c = 2 * (size_t)g.cw * bps; *nc = 1; break;
    case TM_CIEDE_I420: *row_y = g.w * bps; *row_c = g.cw * bps; *nc = 2; break;
    default: *row_y = (size_t)tm_p10_row_words(g.w) * 4; *row_c = (size_t)tm_p10_row_words(g.cw) * 4; *nc = 2; break;
    }
}

double srgb_linear(double c) { return c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4); }
double lab_f(double t) { return t > 216.0 / 24389.0 ? cbrt(t) : ((24389.0 / 27.0) * t + 16.0) / 116.0; }
double hue_deg(double b, double a)
{
    if (a == 0.0 && b == 0.0) return 0.0;
    const double h = atan2(b, a) * (180.0 / M_PI);
    return h < 0.0 ? h + 360.0 : h;
}
double rad(double deg) { return deg * (M_PI / 180.0); }

} // namespace

extern "C" {

double tm_ciede_de00(const double lab1[3], const double lab2[3], double kl, double kc, double kh)
{
    if (!lab1 || !lab2 || !(kl > 0 && kc > 0 && kh > 0)) return NAN;
    const double p25_7 = 6103515625.0;
    const double c1 = hypot(lab1[1], lab1[2]), c2 = hypot(lab2[1], lab2[2]);
    const double cb7 = pow((c1 + c2) / 2, 7.0);
    const double G = 0.5 * (1.0 - sqrt(cb7 / (cb7 + p25_7)));
    const double a1 = (1.0 + G) * lab1[1], a2 = (1.0 + G) * lab2[1];
    const double C1 = hypot(a1, lab1[2]), C2 = hypot(a2, lab2[2]);
    const double h1 = hue_deg(lab1[2], a1), h2 = hue_deg(lab2[2], a2);
    const double dL = lab2[0] - lab1[0], dC = C2 - C1;
    const double prod = C1 * C2;
    double dh = 0.0;
    if (prod != 0.0) {
        dh = h2 - h1;
        if (dh > 180.0) dh -= 360.0;
        else if (dh < -180.0) dh += 360.0;
    }
    const double dH = 2.0 * sqrt(prod) * sin(rad(dh / 2));
    const double Lb = (lab1[0] + lab2[0]) / 2, Cb = (C1 + C2) / 2;
    double hb = h1 + h2;
    if (prod != 0.0) {
        if (fabs(h1 - h2) <= 180.0) hb = (h1 + h2) / 2;
        else if (h1 + h2 < 360.0) hb = (h1 + h2) / 2 + 180.0;
        else hb = (h1 + h2) / 2 - 180.0;
    }
    const double T = 1.0 - 0.17 * cos(rad(hb - 30.0)) + 0.24 * cos(rad(2.0 * hb)) + 0.32 * cos(rad(3.0 * hb + 6.0)) - 0.20 * cos(rad(4.0 * hb - 63.0));
    const double e = (hb - 275.0) / 25.0;
    const double dth = 30.0 * exp(-(e * e));
    const double Cb7 = pow(Cb, 7.0);
    const double RC = 2.0 * sqrt(Cb7 / (Cb7 + p25_7));
    const double l2 = (Lb - 50.0) * (Lb - 50.0);
    const double SL = 1.0 + 0.015 * l2 / sqrt(20.0 + l2);
    const double SC = 1.0 + 0.045 * Cb, SH = 1.0 + 0.015 * Cb * T;
    const double RT = -sin(rad(2.0 * dth)) * RC;
    const double x = dL / (kl * SL), y = dC / (kc * SC), z = dH / (kh * SH);
    const double r = x * x + y * y + z * z + RT * y * z;
    return sqrt(r > 0.0 ? r : 0.0);
}

int tm_ciede_lab(uint32_t y, uint32_t u, uint32_t v, int matrix, uint32_t bits, double lab[3])
{
    if (!lab || matrix < 0 || matrix >= TMC_MATRICES) return TM_ERR_INVALID_ARG;
    if (bits < 8 || bits > 16) return TM_ERR_UNSUPPORTED;
    const double s = (double)(1u << (bits - 8));
    const double *c = kMatrix[matrix];
    const double yn = ((double)y - 16.0 * s) / (219.0 * s), un = ((double)u - 128.0 * s) / (224.0 * s), vn = ((double)v - 128.0 * s) / (224.0 * s);
    const double R = srgb_linear(yn + c[0] * vn), G = srgb_linear(yn - c[1] * un - c[2] * vn), B = srgb_linear(yn + c[3] * un);
    const double X = 0.4124564 * R + 0.3575761 * G + 0.1804375 * B;
    const double Y = 0.2126729 * R + 0.7151522 * G + 0.0721750 * B;
    const double Z = 0.0193339 * R + 0.1191920 * G + 0.9503041 * B;
    const double fx = lab_f(X / 0.95047), fy = lab_f(Y), fz = lab_f(Z / 1.08883);
    lab[0] = 116.0 * fy - 16.0;
    lab[1] = 500.0 * (fx - fy);
    lab[2] = 200.0 * (fy - fz);
    return TM_OK;
}

double tm_ciede_score(double de_sum, uint64_t n)
{
    if (n == 0) return NAN;
    if (de_sum == 0.0) return 100.0;
    return std::min(45.0 - 20.0 * log10(de_sum / (double)n), 100.0);
}

int tm_ciede_create(tm_ciede **out, uint32_t w, uint32_t h, int layout, uint32_t bits, int matrix, double kl, double kc, double kh,
                    int full_range, int want_map, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    if (full_range) return TM_ERR_UNSUPPORTED;
    TmCiedeGeom g;
    if (tmc_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    if (tmc_set_params(&g, matrix, kl, kc, kh)) return TM_ERR_INVALID_ARG;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launch's grid y
    tm_ciede *x = new tm_ciede();
    x->g = g;
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
        tm_ciede_destroy(x);
        return rc;
    }
    x->desc.assign(B * 2, TmCiedeDesc{});
    *out = x;
    return TM_OK;
}

void tm_ciede_destroy(tm_ciede *x)
{
    if (!x) return;
    tmfh_close(&x->c, {x->d_desc, x->d_maps, x->d_cells, x->d_res}, {x->h_desc, x->h_res});
    delete x;
}

size_t tm_ciede_mem_usage(const tm_ciede *x) { return x ? x->c.bytes : 0; }

int tm_ciede_set_frame(tm_ciede *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y,
                       size_t pitch_uv, int mem)
{
    if (!x || slot >= x->c.cap || (side != TM_SIDE_REF && side != TM_SIDE_DIS) || !y || !u) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const TmCiedeGeom &g = x->g;
    const bool biplanar = g.layout == TM_CIEDE_NV12 || g.layout == TM_CIEDE_P016;
    if (biplanar) v = nullptr;
    else if (!v) return TM_ERR_INVALID_ARG;
    size_t row_y, row_c;
    int nc;
    plane_rows(x, &row_y, &row_c, &nc);
    if (pitch_y < row_y || pitch_uv < row_c) return TM_ERR_INVALID_ARG;
    const size_t align = g.layout == TM_CIEDE_I420P10_PACKED ? 4 : (g.bits == 8 ? 1 : 2);
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

int tm_ciede_compute_async(tm_ciede *x, uint32_t n_slots)
{
    if (!x) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&x->c, n_slots, 2);
    if (rc) return rc;
    hipStream_t stream = x->c.stream;
    memcpy(x->h_desc, x->desc.data(), 2 * n_slots * sizeof(TmCiedeDesc));
    TMFH_CHK(hipMemcpyAsync(x->d_desc, x->h_desc, 2 * n_slots * sizeof(TmCiedeDesc), hipMemcpyHostToDevice, stream));
    const TmCiedeGeom g = x->g;
    const dim3 grid(g.cells, n_slots), block(TMC_THREADS);
#define TMC_LAUNCH(L, F) k_ciede<L, F><<<grid, block, 0, stream>>>(g, x->d_desc, x->d_maps, x->d_cells)
    TMC_DISPATCH(g, TMC_LAUNCH);
#undef TMC_LAUNCH
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    k_ciede_finish<<<dim3(n_slots), block, 0, stream>>>(g, x->d_cells, x->d_res);
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    TMFH_CHK_QUEUED(&x->c, hipMemcpyAsync(x->h_res, x->d_res, n_slots * sizeof(TmCiedeCell), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&x->c, n_slots, 2);
    return TM_OK;
}

int tm_ciede_sync(tm_ciede *x) { return x ? tmfh_sync(&x->c) : TM_ERR_INVALID_ARG; }

int tm_ciede_get(tm_ciede *x, uint32_t first_slot, uint32_t n, tm_ciede_frame *out)
{
    if (!x || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&x->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    const uint64_t px = (uint64_t)x->g.w * x->g.h;
    for (uint32_t i = 0; i < n; ++i) {
        const TmCiedeCell &r = x->h_res[first_slot + i];
        out[i].de_sum = r.sum;
        out[i].de_mean = r.sum / (double)px;
        out[i].de_max = (double)r.max;
        out[i].score = tm_ciede_score(r.sum, px);
        out[i].pixels = px;
    }
    return TM_OK;
}

int tm_ciede_get_map(tm_ciede *x, uint32_t slot, float *dst, size_t pitch)
{
    if (!x || !dst) return TM_ERR_INVALID_ARG;
    const TmCiedeGeom &g = x->g;
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

