// tm_cambi.hip -- host side of libturbometrics_cambi.so (include/turbo_metrics_cambi.h): frame upload, the launches of a batch, the
// heat-map read-back and the host functions of the definition.  Kernels: tm_cambi_kernels.h; definition: DESIGN.md section 13; the host
// core it shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_cambi.h"
#include "tm_cambi_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMC_Y8 == TM_CAMBI_Y8 && TMC_Y16_MSB == TM_CAMBI_Y16_MSB && TMC_Y16_LOW == TM_CAMBI_Y16_LOW && TMC_Y10_PACKED == TM_CAMBI_Y10_PACKED, "layouts");
static_assert(TMC_SCALES == TM_CAMBI_SCALES && sizeof(tm_cambi_frame) == sizeof(TmCambiRes), "one result is the device's cell");
TMFH_FORMATS_AGREE;

} // namespace

struct tm_cambi {
    TmCambiGeom g;
    TmFeatureHost c;                                  // have, staging: [slot]
    TmCambiDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmCambiDesc> desc;                    // what set_frame wrote
    unsigned short *d_p0 = nullptr;                   // [slot][h][w]: the 10-bit plane before the mode filter
    unsigned char *d_mk = nullptr;                    // [slot][h][w]: the scale-0 mask
    unsigned short *d_q = nullptr;                    // [slot][pyramid]: mode-filtered planes, the mask in bit 15
    float *d_cv = nullptr;                            // [slot][pyramid]: c-values
    TmCambiRes *d_res = nullptr, *h_res = nullptr;    // [slot]
};

namespace {

unsigned blocks(unsigned long long n) { return (unsigned)((n + TMC_THREADS - 1) / TMC_THREADS); }

} // namespace

extern "C" {

int tm_cambi_scores(const tm_cambi_frame *f, uint32_t window, double out[6])
{
    if (!f || !out || window < 3 || window > 127) return TM_ERR_INVALID_ARG;
    static const double weight[TM_CAMBI_SCALES] = {16.0, 8.0, 4.0, 2.0, 1.0};
    const double side = (double)(2 * (window >> 1) + 1), area = side * side;
    double total = 0.0;
    for (int s = 0; s < TM_CAMBI_SCALES; ++s) {
        if (f->k[s] == 0 || f->n_gt[s] >= f->k[s]) return TM_ERR_INVALID_ARG;
        float t;
        memcpy(&t, &f->t[s], 4);
        out[s] = (f->sum_gt[s] + (double)(f->k[s] - f->n_gt[s]) * (double)t) / (double)f->k[s];
        total += weight[s] * out[s];
    }
    const double c = total / area;
    out[5] = c < 1000.0 ? c : 1000.0;
    return TM_OK;
}

int tm_cambi_tvi(double tvi_threshold, uint32_t out[4])
{
    if (!out) return TM_ERR_INVALID_ARG;
    unsigned t[4];
    tmc_tvi(tvi_threshold, t);
    for (int d = 0; d < 4; ++d) out[d] = t[d];
    return TM_OK;
}

uint32_t tm_cambi_mask_index(uint32_t w, uint32_t h) { return tmc_mask_index(w, h); }

uint32_t tm_cambi_window(uint32_t w, uint32_t requested)
{
    const unsigned r = tmc_window(w, requested);
    return r > 127 ? 127 : r;
}

int tm_cambi_create(tm_cambi **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t window, double topk, double tvi_threshold,
                    uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmCambiGeom g;
    if (tmc_make_geom(&g, w, h, layout, bits, window, topk, tvi_threshold)) return TM_ERR_UNSUPPORTED;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launches' grid y
    tm_cambi *s = new tm_cambi();
    s->g = g;
    const size_t B = batch_capacity, px = (size_t)w * h, res = B * sizeof(TmCambiRes);
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&s->c, batch_capacity, B, B))) { delete s; return rc; }
    if ((rc = tmfh_dev_alloc(&s->c, &s->d_desc, B * sizeof(TmCambiDesc))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_p0, B * px * sizeof(unsigned short))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_mk, B * px)) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_q, B * g.tot * sizeof(unsigned short))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_cv, B * g.tot * sizeof(float))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_res, res)) ||
        (rc = tmfh_pinned_alloc(&s->c, &s->h_desc, B * sizeof(TmCambiDesc))) ||
        (rc = tmfh_pinned_alloc(&s->c, &s->h_res, res))) {
        tm_cambi_destroy(s);
        return rc;
    }
    s->desc.assign(B, TmCambiDesc{});
    *out = s;
    return TM_OK;
}

void tm_cambi_destroy(tm_cambi *s)
{
    if (!s) return;
    tmfh_close(&s->c, {s->d_desc, s->d_p0, s->d_mk, s->d_q, s->d_cv, s->d_res}, {s->h_desc, s->h_res});
    delete s;
}

size_t tm_cambi_mem_usage(const tm_cambi *s) { return s ? s->c.bytes : 0; }

int tm_cambi_set_frame(tm_cambi *s, uint32_t slot, const void *y, size_t pitch_y, int mem)
{
    if (!s || slot >= s->c.cap || !y) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const size_t row = tmfh_row_bytes(s->g.fmt, s->g.w[0]);
    if (pitch_y < row) return TM_ERR_INVALID_ARG;
    if (((uintptr_t)y | pitch_y) & (tmfh_align(s->g.fmt) - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    if ((rc = tmfh_sync(&s->c))) return rc; // whatever `mem` is: the staging surfaces may still be read
    TMFH_CHK(hipSetDevice(s->c.device));
    TmCambiDesc d{};
    if (mem == TM_MEM_DEVICE) {
        d.p = y; d.pitch = pitch_y;
    } else {
        if ((rc = tmfh_upload(&s->c, slot, y, pitch_y, row, s->g.h[0], &d.p, &d.pitch))) return rc;
        if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(s->c.stream));
    }
    d.vec = tmfh_vec((uintptr_t)d.p | d.pitch);
    s->desc[slot] = d;
    s->c.have[slot] = 1;
    return TM_OK;
}

int tm_cambi_compute_async(tm_cambi *s, uint32_t n_slots)
{
    if (!s) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&s->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = s->c.stream;
    memcpy(s->h_desc, s->desc.data(), n_slots * sizeof(TmCambiDesc));
    TMFH_CHK(hipMemcpyAsync(s->d_desc, s->h_desc, n_slots * sizeof(TmCambiDesc), hipMemcpyHostToDevice, stream));
    const TmCambiGeom g = s->g;
    const dim3 block(TMC_THREADS);
    const dim3 gi(blocks((g.w[0] + 3) / 4) * g.h[0], n_slots);
    switch (g.fmt) {
    case TMX_F_U8: k_cambi_ingest<TMX_F_U8><<<gi, block, 0, stream>>>(g, s->d_desc, s->d_p0); break;
    case TMX_F_U16_MSB: k_cambi_ingest<TMX_F_U16_MSB><<<gi, block, 0, stream>>>(g, s->d_desc, s->d_p0); break;
    case TMX_F_U16_LOW: k_cambi_ingest<TMX_F_U16_LOW><<<gi, block, 0, stream>>>(g, s->d_desc, s->d_p0); break;
    default: k_cambi_ingest<TMX_F_P10><<<gi, block, 0, stream>>>(g, s->d_desc, s->d_p0); break;
    }
    TMFH_CHK_QUEUED(&s->c, hipGetLastError());
    k_cambi_mask<<<dim3(((g.w[0] + TMC_MASK_TW - 1) / TMC_MASK_TW) * ((g.h[0] + TMC_MASK_TH - 1) / TMC_MASK_TH), n_slots), block, 0, stream>>>(g, s->d_p0, s->d_mk);
    TMFH_CHK_QUEUED(&s->c, hipGetLastError());
    for (int sc = 0; sc < TMC_SCALES; ++sc) {
        const dim3 gm(blocks((unsigned long long)g.w[sc] * g.h[sc]), n_slots);
        if (sc == 0) k_cambi_mode<true><<<gm, block, 0, stream>>>(g, sc, s->d_p0, s->d_mk, s->d_q);
        else k_cambi_mode<false><<<gm, block, 0, stream>>>(g, sc, s->d_q, s->d_mk, s->d_q);
        TMFH_CHK_QUEUED(&s->c, hipGetLastError());
        const dim3 gc(((g.w[sc] + g.oc - 1) / g.oc) * ((g.h[sc] + g.band_rows - 1) / g.band_rows), n_slots);
        k_cambi_cvalues<<<gc, block, 0, stream>>>(g, sc, s->d_q, s->d_cv);
        TMFH_CHK_QUEUED(&s->c, hipGetLastError());
    }
    k_cambi_pool<<<dim3(TMC_SCALES, n_slots), block, 0, stream>>>(g, s->d_cv, s->d_res);
    TMFH_CHK_QUEUED(&s->c, hipGetLastError());
    TMFH_CHK_QUEUED(&s->c, hipMemcpyAsync(s->h_res, s->d_res, (size_t)n_slots * sizeof(TmCambiRes), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&s->c, n_slots, 1);
    return TM_OK;
}

int tm_cambi_sync(tm_cambi *s) { return s ? tmfh_sync(&s->c) : TM_ERR_INVALID_ARG; }

int tm_cambi_get(tm_cambi *s, uint32_t first_slot, uint32_t n, tm_cambi_frame *out)
{
    if (!s || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&s->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&s->c);
    if (rc) return rc;
    memcpy(out, s->h_res + first_slot, (size_t)n * sizeof(tm_cambi_frame));
    return TM_OK;
}

int tm_cambi_get_map(tm_cambi *s, uint32_t slot, uint32_t scale, float *out, size_t pitch)
{
    if (!s || !out || scale >= TMC_SCALES) return TM_ERR_INVALID_ARG;
    const size_t row = (size_t)s->g.w[scale] * sizeof(float);
    if (pitch < row || (pitch & 3)) return TM_ERR_INVALID_ARG;
    if (slot >= s->c.n_last) return TM_ERR_STATE;
    const int rc = tmfh_sync(&s->c);
    if (rc) return rc;
    TMFH_CHK(hipSetDevice(s->c.device));
    const float *src = s->d_cv + (size_t)slot * s->g.tot + s->g.off[scale];
    TMFH_CHK(hipMemcpy2DAsync(out, pitch, src, row, row, s->g.h[scale], hipMemcpyDeviceToHost, s->c.stream));
    TMFH_CHK(hipStreamSynchronize(s->c.stream));
    return TM_OK;
}

} // extern "C"
