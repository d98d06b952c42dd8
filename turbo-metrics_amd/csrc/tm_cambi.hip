// tm_cambi.hip -- host side of libturbometrics_cambi.so (include/turbo_metrics_cambi.h): frame upload, the launches of a batch, the
// heat-map read-back and the host functions of the definition.  Kernels: tm_cambi_kernels.h; definition: DESIGN.md section 13.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_cambi.h"
#include "tm_cambi_kernels.h"

namespace {

static_assert(TMC_Y8 == TM_CAMBI_Y8 && TMC_Y16_MSB == TM_CAMBI_Y16_MSB && TMC_Y16_LOW == TM_CAMBI_Y16_LOW && TMC_Y10_PACKED == TM_CAMBI_Y10_PACKED, "layouts");
static_assert(TMC_SCALES == TM_CAMBI_SCALES && sizeof(tm_cambi_frame) == sizeof(TmCambiRes), "one result is the device's cell");

#define CCHK(call)                                      \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

} // namespace

struct tm_cambi {
    TmCambiGeom g;
    uint32_t cap;
    int device;
    hipStream_t stream = nullptr;
    TmCambiDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmCambiDesc> desc;                    // what set_frame wrote
    std::vector<unsigned char> have;                  // [slot]: set since the last compute
    std::vector<void *> staging;                      // [slot]: device copy of a host picture (lazily allocated)
    unsigned short *d_p0 = nullptr;                   // [slot][h][w]: the 10-bit plane before the mode filter
    unsigned char *d_mk = nullptr;                    // [slot][h][w]: the scale-0 mask
    unsigned short *d_q = nullptr;                    // [slot][pyramid]: mode-filtered planes, the mask in bit 15
    float *d_cv = nullptr;                            // [slot][pyramid]: c-values
    TmCambiRes *d_res = nullptr, *h_res = nullptr;    // [slot]
    size_t bytes = 0;
    bool pending = false;
    uint32_t n_last = 0;
};

namespace {

int dev_alloc(tm_cambi *s, void **p, size_t n)
{
    const hipError_t r = hipMalloc(p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    CCHK(r);
    s->bytes += n;
    return TM_OK;
}

// bytes of one luma row
size_t row_bytes(const tm_cambi *s)
{
    switch (s->g.fmt) {
    case TMX_F_U8: return (size_t)s->g.w[0];
    case TMX_F_P10: return (size_t)tm_p10_row_words(s->g.w[0]) * 4;
    default: return (size_t)s->g.w[0] * 2;
    }
}

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
    int rc;
    // ---- first device call
    tm_cambi *s = new tm_cambi();
    s->g = g; s->cap = batch_capacity;
    auto fail = [&](int e) { tm_cambi_destroy(s); return e; };
    if (hipGetDevice(&s->device) != hipSuccess) { (void)hipGetLastError(); delete s; return TM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); s->stream = nullptr; return fail(TM_ERR_HIP); }
    const size_t B = batch_capacity, px = (size_t)w * h, res = B * sizeof(TmCambiRes);
    if ((rc = dev_alloc(s, (void **)&s->d_desc, B * sizeof(TmCambiDesc)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_p0, B * px * sizeof(unsigned short)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_mk, B * px))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_q, B * g.tot * sizeof(unsigned short)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_cv, B * g.tot * sizeof(float)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_res, res))) return fail(rc);
    if (hipHostMalloc((void **)&s->h_desc, B * sizeof(TmCambiDesc), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); s->h_desc = nullptr; return fail(TM_ERR_OOM); }
    if (hipHostMalloc((void **)&s->h_res, res, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); s->h_res = nullptr; return fail(TM_ERR_OOM); }
    s->bytes += B * sizeof(TmCambiDesc) + res;
    s->desc.assign(B, TmCambiDesc{});
    s->have.assign(B, 0);
    s->staging.assign(B, nullptr);
    *out = s;
    return TM_OK;
}

void tm_cambi_destroy(tm_cambi *s)
{
    if (!s) return;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (void *p : s->staging) if (p) (void)hipFree(p);
    if (s->d_desc) (void)hipFree(s->d_desc);
    if (s->d_p0) (void)hipFree(s->d_p0);
    if (s->d_mk) (void)hipFree(s->d_mk);
    if (s->d_q) (void)hipFree(s->d_q);
    if (s->d_cv) (void)hipFree(s->d_cv);
    if (s->d_res) (void)hipFree(s->d_res);
    if (s->h_desc) (void)hipHostFree(s->h_desc);
    if (s->h_res) (void)hipHostFree(s->h_res);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    (void)hipGetLastError();
    delete s;
}

size_t tm_cambi_mem_usage(const tm_cambi *s) { return s ? s->bytes : 0; }

int tm_cambi_set_frame(tm_cambi *s, uint32_t slot, const void *y, size_t pitch_y, int mem)
{
    if (!s || slot >= s->cap || !y) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE && mem != TM_MEM_HOST_PINNED) return TM_ERR_INVALID_ARG;
    const size_t row = row_bytes(s);
    if (pitch_y < row) return TM_ERR_INVALID_ARG;
    const size_t align = s->g.fmt == TMX_F_P10 ? 4 : (s->g.fmt == TMX_F_U8 ? 1 : 2);
    if (((uintptr_t)y | pitch_y) & (align - 1)) return TM_ERR_INVALID_ARG;
    if (s->pending) {
        const int rc = tm_cambi_sync(s); // the staging surfaces may still be read
        if (rc) return rc;
    }
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const size_t rows = s->g.h[0];
    TmCambiDesc d{};
    if (mem == TM_MEM_DEVICE) {
        d.p = y; d.pitch = pitch_y;
    } else {
        const size_t sp = (row + 255) / 256 * 256;
        if (!s->staging[slot]) {
            const int rc = dev_alloc(s, &s->staging[slot], sp * rows);
            if (rc) return rc;
        }
        CCHK(hipMemcpy2DAsync(s->staging[slot], sp, y, pitch_y, row, rows, hipMemcpyHostToDevice, s->stream));
        if (mem == TM_MEM_HOST) CCHK(hipStreamSynchronize(s->stream));
        d.p = s->staging[slot]; d.pitch = sp;
    }
    d.vec = (((uintptr_t)d.p | d.pitch) & 15) == 0;
    s->desc[slot] = d;
    s->have[slot] = 1;
    return TM_OK;
}

int tm_cambi_compute_async(tm_cambi *s, uint32_t n_slots)
{
    if (!s || n_slots == 0 || n_slots > s->cap) return TM_ERR_INVALID_ARG;
    if (s->pending) return TM_ERR_STATE;
    for (uint32_t i = 0; i < n_slots; ++i)
        if (!s->have[i]) return TM_ERR_STATE;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    memcpy(s->h_desc, s->desc.data(), n_slots * sizeof(TmCambiDesc));
    CCHK(hipMemcpyAsync(s->d_desc, s->h_desc, n_slots * sizeof(TmCambiDesc), hipMemcpyHostToDevice, s->stream));
    const TmCambiGeom g = s->g;
    const dim3 block(TMC_THREADS);
    const dim3 gi(blocks((g.w[0] + 3) / 4) * g.h[0], n_slots);
    switch (g.fmt) {
    case TMX_F_U8: k_cambi_ingest<TMX_F_U8><<<gi, block, 0, s->stream>>>(g, s->d_desc, s->d_p0); break;
    case TMX_F_U16_MSB: k_cambi_ingest<TMX_F_U16_MSB><<<gi, block, 0, s->stream>>>(g, s->d_desc, s->d_p0); break;
    case TMX_F_U16_LOW: k_cambi_ingest<TMX_F_U16_LOW><<<gi, block, 0, s->stream>>>(g, s->d_desc, s->d_p0); break;
    default: k_cambi_ingest<TMX_F_P10><<<gi, block, 0, s->stream>>>(g, s->d_desc, s->d_p0); break;
    }
    CCHK(hipGetLastError());
    k_cambi_mask<<<dim3(((g.w[0] + TMC_MASK_TW - 1) / TMC_MASK_TW) * ((g.h[0] + TMC_MASK_TH - 1) / TMC_MASK_TH), n_slots), block, 0, s->stream>>>(g, s->d_p0, s->d_mk);
    CCHK(hipGetLastError());
    for (int sc = 0; sc < TMC_SCALES; ++sc) {
        const dim3 gm(blocks((unsigned long long)g.w[sc] * g.h[sc]), n_slots);
        if (sc == 0) k_cambi_mode<true><<<gm, block, 0, s->stream>>>(g, sc, s->d_p0, s->d_mk, s->d_q);
        else k_cambi_mode<false><<<gm, block, 0, s->stream>>>(g, sc, s->d_q, s->d_mk, s->d_q);
        CCHK(hipGetLastError());
        const dim3 gc(((g.w[sc] + g.oc - 1) / g.oc) * ((g.h[sc] + g.band_rows - 1) / g.band_rows), n_slots);
        k_cambi_cvalues<<<gc, block, 0, s->stream>>>(g, sc, s->d_q, s->d_cv);
        CCHK(hipGetLastError());
    }
    k_cambi_pool<<<dim3(TMC_SCALES, n_slots), block, 0, s->stream>>>(g, s->d_cv, s->d_res);
    CCHK(hipGetLastError());
    CCHK(hipMemcpyAsync(s->h_res, s->d_res, (size_t)n_slots * sizeof(TmCambiRes), hipMemcpyDeviceToHost, s->stream));
    s->pending = true;
    // every batch hands its pictures over anew: a slot not set again before the next compute is TM_ERR_STATE, not a stale picture
    std::fill(s->have.begin(), s->have.begin() + n_slots, 0);
    s->n_last = n_slots;
    return TM_OK;
}

int tm_cambi_sync(tm_cambi *s)
{
    if (!s) return TM_ERR_INVALID_ARG;
    if (!s->pending) return TM_OK;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    CCHK(hipStreamSynchronize(s->stream));
    s->pending = false;
    return TM_OK;
}

int tm_cambi_get(tm_cambi *s, uint32_t first_slot, uint32_t n, tm_cambi_frame *out)
{
    if (!s || !out) return TM_ERR_INVALID_ARG;
    if (s->n_last == 0 || first_slot + (uint64_t)n > s->n_last) return TM_ERR_STATE;
    const int rc = tm_cambi_sync(s);
    if (rc) return rc;
    memcpy(out, s->h_res + first_slot, (size_t)n * sizeof(tm_cambi_frame));
    return TM_OK;
}

int tm_cambi_get_map(tm_cambi *s, uint32_t slot, uint32_t scale, float *out, size_t pitch)
{
    if (!s || !out || scale >= TMC_SCALES) return TM_ERR_INVALID_ARG;
    const size_t row = (size_t)s->g.w[scale] * sizeof(float);
    if (pitch < row || (pitch & 3)) return TM_ERR_INVALID_ARG;
    if (slot >= s->n_last) return TM_ERR_STATE;
    const int rc = tm_cambi_sync(s);
    if (rc) return rc;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const float *src = s->d_cv + (size_t)slot * s->g.tot + s->g.off[scale];
    CCHK(hipMemcpy2DAsync(out, pitch, src, row, row, s->g.h[scale], hipMemcpyDeviceToHost, s->stream));
    CCHK(hipStreamSynchronize(s->stream));
    return TM_OK;
}

} // extern "C"
