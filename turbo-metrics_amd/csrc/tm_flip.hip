// tm_flip.hip -- host side of libturbometrics_flip.so (include/turbo_metrics_flip.h): pair upload, the two launches of a batch, the map
// read-back and the host function of the definition.  Kernels: tm_flip_kernels.h; definition: DESIGN.md section 14; the host core it
// shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_flip.h"
#include "tm_flip_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMF_RGB8 == TM_FLIP_RGB8 && TMF_MAP == TM_FLIP_MAP && TMF_MAP_COLOR == TM_FLIP_MAP_COLOR && TMF_MAP_FEATURE == TM_FLIP_MAP_FEATURE, "layouts and kinds");
static_assert(sizeof(tm_flip_frame) == sizeof(TmFlipRes) && TMF_HALO == TM_FLIP_MAX_RADIUS, "one result is the device's cell");

} // namespace

struct tm_flip {
    TmFlipGeom g;
    TmFeatureHost c;                                 // have: [slot]; staging: [slot][side]
    TmFlipTables *d_tabs = nullptr;
    TmFlipDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmFlipDesc> desc;                    // what set_pair wrote
    float *d_maps = nullptr;                         // [slot][kind][h][w]
    TmFlipCell *d_cells = nullptr;                   // [slot][tile]
    TmFlipRes *d_res = nullptr, *h_res = nullptr;    // [slot]
};

extern "C" {

int tm_flip_radius(double ppd, uint32_t *r_spatial, uint32_t *r_feature)
{
    if (!r_spatial || !r_feature) return TM_ERR_INVALID_ARG;
    if (ppd == 0.0) ppd = TM_FLIP_DEFAULT_PPD;
    if (!(ppd > 0.0) || !(ppd <= 1e6)) return TM_ERR_INVALID_ARG; // (beyond 1e6 the radii leave 32 bits)
    unsigned rs, rf;
    tmf_radius(ppd, &rs, &rf);
    *r_spatial = rs; *r_feature = rf;
    return TM_OK;
}

int tm_flip_create(tm_flip **out, uint32_t w, uint32_t h, int layout, double ppd, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0 || batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launches' grid y
    if (ppd == 0.0) ppd = TM_FLIP_DEFAULT_PPD;
    TmFlipGeom g;
    TmFlipTables tabs;
    if (tmf_make_geom(&g, &tabs, w, h, layout, ppd)) return TM_ERR_UNSUPPORTED;
    tm_flip *s = new tm_flip();
    s->g = g;
    const size_t B = batch_capacity, px = (size_t)w * h, tiles = (size_t)g.tiles_x * g.tiles_y, res = B * sizeof(TmFlipRes);
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&s->c, batch_capacity, B, 2 * B))) { delete s; return rc; }
    if ((rc = tmfh_dev_alloc(&s->c, &s->d_tabs, sizeof(TmFlipTables))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_desc, B * sizeof(TmFlipDesc))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_maps, B * TMF_MAPS * px * sizeof(float))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_cells, B * tiles * sizeof(TmFlipCell))) ||
        (rc = tmfh_dev_alloc(&s->c, &s->d_res, res)) ||
        (rc = tmfh_pinned_alloc(&s->c, &s->h_desc, B * sizeof(TmFlipDesc))) ||
        (rc = tmfh_pinned_alloc(&s->c, &s->h_res, res))) {
        tm_flip_destroy(s);
        return rc;
    }
    if (hipMemcpy(s->d_tabs, &tabs, sizeof tabs, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        tm_flip_destroy(s);
        return TM_ERR_HIP;
    }
    s->desc.assign(B, TmFlipDesc{});
    *out = s;
    return TM_OK;
}

void tm_flip_destroy(tm_flip *s)
{
    if (!s) return;
    tmfh_close(&s->c, {s->d_tabs, s->d_desc, s->d_maps, s->d_cells, s->d_res}, {s->h_desc, s->h_res});
    delete s;
}

size_t tm_flip_mem_usage(const tm_flip *s) { return s ? s->c.bytes : 0; }

int tm_flip_set_pair(tm_flip *s, uint32_t slot, const void *ref, size_t ref_pitch, const void *dis, size_t dis_pitch, int mem)
{
    if (!s || slot >= s->c.cap || !ref || !dis) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE) return TM_ERR_INVALID_ARG; // (no pinned pictures here)
    const size_t row = (size_t)s->g.w * 3, rows = s->g.h;
    if (ref_pitch < row || dis_pitch < row) return TM_ERR_INVALID_ARG;
    int rc;
    if ((rc = tmfh_sync(&s->c))) return rc; // whatever `mem` is: the staging surfaces may still be read
    TMFH_CHK(hipSetDevice(s->c.device));
    const void *src[2] = {ref, dis};
    const size_t pitch[2] = {ref_pitch, dis_pitch};
    TmFlipDesc d{};
    for (int side = 0; side < 2; ++side) {
        const void *p = src[side];
        d.pitch[side] = pitch[side];
        if (mem != TM_MEM_DEVICE && (rc = tmfh_upload(&s->c, 2 * (size_t)slot + side, src[side], pitch[side], row, rows, &p, &d.pitch[side]))) return rc;
        d.p[side] = (const unsigned char *)p;
    }
    if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(s->c.stream));
    s->desc[slot] = d;
    s->c.have[slot] = 1;
    return TM_OK;
}

int tm_flip_compute_async(tm_flip *s, uint32_t n_slots)
{
    if (!s) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&s->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = s->c.stream;
    memcpy(s->h_desc, s->desc.data(), n_slots * sizeof(TmFlipDesc));
    TMFH_CHK(hipMemcpyAsync(s->d_desc, s->h_desc, n_slots * sizeof(TmFlipDesc), hipMemcpyHostToDevice, stream));
    const TmFlipGeom g = s->g;
    k_flip_tile<<<dim3(g.tiles_x * g.tiles_y, n_slots), dim3(TMF_THREADS), 0, stream>>>(g, s->d_tabs, s->d_desc, s->d_maps, s->d_cells);
    TMFH_CHK_QUEUED(&s->c, hipGetLastError());
    k_flip_finish<<<dim3(n_slots), dim3(TMF_THREADS), 0, stream>>>(g, s->d_cells, s->d_res);
    TMFH_CHK_QUEUED(&s->c, hipGetLastError());
    TMFH_CHK_QUEUED(&s->c, hipMemcpyAsync(s->h_res, s->d_res, (size_t)n_slots * sizeof(TmFlipRes), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&s->c, n_slots, 1);
    return TM_OK;
}

int tm_flip_sync(tm_flip *s) { return s ? tmfh_sync(&s->c) : TM_ERR_INVALID_ARG; }

int tm_flip_get(tm_flip *s, uint32_t first_slot, uint32_t n, tm_flip_frame *out)
{
    if (!s || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&s->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&s->c);
    if (rc) return rc;
    memcpy(out, s->h_res + first_slot, (size_t)n * sizeof(tm_flip_frame));
    return TM_OK;
}

int tm_flip_get_map(tm_flip *s, uint32_t slot, int kind, float *out, size_t pitch)
{
    if (!s || !out || kind < 0 || kind >= TMF_MAPS) return TM_ERR_INVALID_ARG;
    const size_t row = (size_t)s->g.w * sizeof(float);
    if (pitch < row || (pitch & 3)) return TM_ERR_INVALID_ARG;
    if (slot >= s->c.n_last) return TM_ERR_STATE;
    const int rc = tmfh_sync(&s->c);
    if (rc) return rc;
    TMFH_CHK(hipSetDevice(s->c.device));
    const size_t px = (size_t)s->g.w * s->g.h;
    const float *src = s->d_maps + ((size_t)slot * TMF_MAPS + (size_t)kind) * px;
    TMFH_CHK(hipMemcpy2DAsync(out, pitch, src, row, row, s->g.h, hipMemcpyDeviceToHost, s->c.stream));
    TMFH_CHK(hipStreamSynchronize(s->c.stream));
    return TM_OK;
}

} // extern "C"
