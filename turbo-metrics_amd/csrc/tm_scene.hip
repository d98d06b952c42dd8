// tm_scene.hip -- host side of libturbometrics_scene.so (include/turbo_metrics_scene.h): frame upload, two launches per batch, and the
// host functions of the definition.  Kernels: tm_scene_kernels.h; definition: DESIGN.md section 12; the host core it shares:
// tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_scene.h"
#include "tm_scene_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMS_Y8 == TM_SCENE_Y8 && TMS_Y16_MSB == TM_SCENE_Y16_MSB && TMS_Y16_LOW == TM_SCENE_Y16_LOW && TMS_Y10_PACKED == TM_SCENE_Y10_PACKED, "layouts");
static_assert(sizeof(tm_scene_frame) == TMS_BINS * sizeof(unsigned), "one result is the 256 counters");
TMFH_FORMATS_AGREE;

} // namespace

struct tm_scene {
    TmSceneGeom g;
    TmFeatureHost c;                                  // have, staging: [slot]
    TmSceneDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmSceneDesc> desc;                    // what set_frame wrote
    unsigned *d_cells = nullptr;                      // [slot][band][256]: every cell is written by every compute
    unsigned *d_hist = nullptr, *h_hist = nullptr;    // [slot][256]
};

extern "C" {

int tm_scene_distance(const uint32_t a[256], const uint32_t b[256], int bins, uint64_t *out)
{
    if (!a || !b || !out) return TM_ERR_INVALID_ARG;
    if (bins != 8 && bins != 16 && bins != 32 && bins != 64 && bins != 128 && bins != 256) return TM_ERR_INVALID_ARG;
    const int run = 256 / bins;
    uint64_t d = 0;
    for (int k = 0; k < bins; ++k) {
        uint64_t sa = 0, sb = 0;
        for (int j = 0; j < run; ++j) { sa += a[k * run + j]; sb += b[k * run + j]; }
        d += sa > sb ? sa - sb : sb - sa;
    }
    *out = d;
    return TM_OK;
}

double tm_scene_score(uint64_t distance, uint32_t w, uint32_t h) { return (double)distance / (2.0 * (double)w * (double)h); }

int tm_scene_is_cut(double score, double threshold) { return score >= threshold; }

int tm_scene_stats(const uint32_t hist[256], uint32_t *min_bin, uint32_t *max_bin, double *mean_bin)
{
    if (!hist) return TM_ERR_INVALID_ARG;
    uint64_t n = 0, sum = 0;
    uint32_t lo = 256, hi = 0;
    for (uint32_t b = 0; b < 256; ++b) {
        if (!hist[b]) continue;
        if (lo == 256) lo = b;
        hi = b;
        n += hist[b];
        sum += (uint64_t)b * hist[b];
    }
    if (n == 0) return TM_ERR_INVALID_ARG;
    if (min_bin) *min_bin = lo;
    if (max_bin) *max_bin = hi;
    if (mean_bin) *mean_bin = (double)sum / (double)n;
    return TM_OK;
}

int tm_scene_create(tm_scene **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmSceneGeom g;
    if (tms_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launch's grid y
    tm_scene *s = new tm_scene();
    s->g = g;
    const size_t B = batch_capacity, res = B * TMS_BINS * sizeof(unsigned);
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&s->c, batch_capacity, B, B))) { delete s; return rc; }
    if ((rc = tmfh_dev_alloc(&s->c, &s->d_desc, B * sizeof(TmSceneDesc))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_cells, res * g.bands)) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_hist, res)) ||
        (rc = tmfh_pinned_alloc(&s->c, &s->h_desc, B * sizeof(TmSceneDesc))) ||
        (rc = tmfh_pinned_alloc(&s->c, &s->h_hist, res))) {
        tm_scene_destroy(s);
        return rc;
    }
    s->desc.assign(B, TmSceneDesc{});
    *out = s;
    return TM_OK;
}

void tm_scene_destroy(tm_scene *s)
{
    if (!s) return;
    tmfh_close(&s->c, {s->d_desc, s->d_cells, s->d_hist}, {s->h_desc, s->h_hist});
    delete s;
}

size_t tm_scene_mem_usage(const tm_scene *s) { return s ? s->c.bytes : 0; }

int tm_scene_set_frame(tm_scene *s, uint32_t slot, const void *y, size_t pitch_y, int mem)
{
    if (!s || slot >= s->c.cap || !y) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const size_t row = tmfh_row_bytes(s->g.fmt, s->g.w);
    if (pitch_y < row) return TM_ERR_INVALID_ARG;
    if (((uintptr_t)y | pitch_y) & (tmfh_align(s->g.fmt) - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    if ((rc = tmfh_sync(&s->c))) return rc; // whatever `mem` is: the staging surfaces may still be read
    TMFH_CHK(hipSetDevice(s->c.device));
    TmSceneDesc d{};
    if (mem == TM_MEM_DEVICE) {
        d.p = y; d.pitch = pitch_y;
    } else {
        if ((rc = tmfh_upload(&s->c, slot, y, pitch_y, row, s->g.h, &d.p, &d.pitch))) return rc;
        if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(s->c.stream));
    }
    d.vec = tmfh_vec((uintptr_t)d.p | d.pitch);
    s->desc[slot] = d;
    s->c.have[slot] = 1;
    return TM_OK;
}

int tm_scene_compute_async(tm_scene *s, uint32_t n_slots)
{
    if (!s) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&s->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = s->c.stream;
    memcpy(s->h_desc, s->desc.data(), n_slots * sizeof(TmSceneDesc));
    TMFH_CHK(hipMemcpyAsync(s->d_desc, s->h_desc, n_slots * sizeof(TmSceneDesc), hipMemcpyHostToDevice, stream));
    const TmSceneGeom g = s->g;
    const dim3 grid(g.bands, n_slots), block(TMS_THREADS);
    switch (g.fmt) {
    case TMX_F_U8: k_scene_hist<TMX_F_U8><<<grid, block, 0, stream>>>(g, s->d_desc, s->d_cells); break;
    case TMX_F_U16_MSB: k_scene_hist<TMX_F_U16_MSB><<<grid, block, 0, stream>>>(g, s->d_desc, s->d_cells); break;
    case TMX_F_U16_LOW: k_scene_hist<TMX_F_U16_LOW><<<grid, block, 0, stream>>>(g, s->d_desc, s->d_cells); break;
    default: k_scene_hist<TMX_F_P10><<<grid, block, 0, stream>>>(g, s->d_desc, s->d_cells); break;
    }
    TMFH_CHK_QUEUED(&s->c, hipGetLastError());
    k_scene_finish<<<dim3(n_slots), block, 0, stream>>>(g.bands, s->d_cells, s->d_hist);
    TMFH_CHK_QUEUED(&s->c, hipGetLastError());
    TMFH_CHK_QUEUED(&s->c, hipMemcpyAsync(s->h_hist, s->d_hist, (size_t)n_slots * TMS_BINS * sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&s->c, n_slots, 1);
    return TM_OK;
}

int tm_scene_sync(tm_scene *s) { return s ? tmfh_sync(&s->c) : TM_ERR_INVALID_ARG; }

int tm_scene_get(tm_scene *s, uint32_t first_slot, uint32_t n, tm_scene_frame *out)
{
    if (!s || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&s->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&s->c);
    if (rc) return rc;
    memcpy(out, s->h_hist + (size_t)first_slot * TMS_BINS, (size_t)n * sizeof(tm_scene_frame));
    return TM_OK;
}

} // extern "C"
