// tm_haarpsi.hip -- host side of libturbometrics_haarpsi.so (include/turbo_metrics_haarpsi.h): pair upload, the two launches per batch,
// the map read-back and the host function.  Kernels: tm_haarpsi_kernels.h; definition: DESIGN.md section 21; the host core it shares:
// tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_haarpsi.h"
#include "tm_haarpsi_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMP_Y8 == TM_HAARPSI_Y8 && TMP_Y16_MSB == TM_HAARPSI_Y16_MSB && TMP_Y16_LOW == TM_HAARPSI_Y16_LOW && TMP_Y10_PACKED == TM_HAARPSI_Y10_PACKED, "layouts");
TMFH_FORMATS_AGREE;

} // namespace

#ifdef TM_EMULATE
// tests/host/haarpsi_host_test.cpp compiles this file with a host compiler against a fake runtime, where nothing can be launched: the
// two launches are the test's own function
void tm_haarpsi_host_test_launch(const TmHaarpsiGeom &g, unsigned n_slots, const TmHaarpsiDesc *desc, float *maps, TmHaarpsiCell *cells, TmHaarpsiCell *res);
#endif

struct tm_haarpsi {
    TmHaarpsiGeom g;
    TmFeatureHost c;                                        // have: [slot]; staging: [slot][2]
    TmHaarpsiDesc *d_desc = nullptr, *h_desc = nullptr;     // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmHaarpsiDesc> desc;                        // what set_pair wrote
    float *d_maps = nullptr;                                // TM_HAARPSI_MAPS: [slot][g.h2][g.w2]: every value is written by every compute
    TmHaarpsiCell *d_cells = nullptr;                       // [slot][g.cells]: every cell is written by every compute
    TmHaarpsiCell *d_res = nullptr, *h_res = nullptr;       // [slot]
};

extern "C" {

double tm_haarpsi_score(double q, uint64_t ws)
{
    if (ws == 0) return NAN; // both pictures flat: 0 / 0
    const double x = q / (double)ws;
    const double s = log((1.0 - x) / x) / (double)TMP_A; // the f32 alpha the device multiplied by
    return s * s;
}

int tm_haarpsi_create(tm_haarpsi **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity, uint32_t flags)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0 || (flags & ~(uint32_t)TM_HAARPSI_MAPS)) return TM_ERR_INVALID_ARG;
    TmHaarpsiGeom g;
    if (tmp_make_geom(&g, w, h, layout, bits, (flags & TM_HAARPSI_MAPS) != 0)) return TM_ERR_UNSUPPORTED;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launch's grid y
    tm_haarpsi *v = new tm_haarpsi();
    v->g = g;
    const size_t B = batch_capacity;
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&v->c, batch_capacity, B, 2 * B))) { delete v; return rc; }
    if ((rc = tmfh_dev_alloc(&v->c, &v->d_cells, B * (size_t)g.cells * sizeof(TmHaarpsiCell))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_desc, B * sizeof(TmHaarpsiDesc))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_res, B * sizeof(TmHaarpsiCell))) ||
        (g.maps && (rc = tmfh_dev_alloc(&v->c, &v->d_maps, B * (size_t)g.w2 * g.h2 * sizeof(float)))) ||
        (rc = tmfh_pinned_alloc(&v->c, &v->h_desc, B * sizeof(TmHaarpsiDesc))) ||
        (rc = tmfh_pinned_alloc(&v->c, &v->h_res, B * sizeof(TmHaarpsiCell)))) {
        tm_haarpsi_destroy(v);
        return rc;
    }
    v->desc.assign(B, TmHaarpsiDesc{});
    *out = v;
    return TM_OK;
}

void tm_haarpsi_destroy(tm_haarpsi *v)
{
    if (!v) return;
    tmfh_close(&v->c, {v->d_cells, v->d_desc, v->d_res, v->d_maps}, {v->h_desc, v->h_res});
    delete v;
}

size_t tm_haarpsi_mem_usage(const tm_haarpsi *v) { return v ? v->c.bytes : 0; }

int tm_haarpsi_set_pair(tm_haarpsi *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem)
{
    if (!v || slot >= v->c.cap || !ref_y || !dis_y) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const size_t row = tmfh_row_bytes(v->g.fmt, v->g.w);
    if (pitch_ref < row || pitch_dis < row) return TM_ERR_INVALID_ARG;
    if (((uintptr_t)ref_y | (uintptr_t)dis_y | pitch_ref | pitch_dis) & (tmfh_align(v->g.fmt) - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    if ((rc = tmfh_sync(&v->c))) return rc; // whatever `mem` is: the staging surfaces may still be read
    TMFH_CHK(hipSetDevice(v->c.device));
    const void *src[2] = {ref_y, dis_y};
    const size_t pitch[2] = {pitch_ref, pitch_dis};
    TmHaarpsiDesc d{};
    d.vec = 1;
    for (int p = 0; p < 2; ++p) {
        if (mem == TM_MEM_DEVICE) {
            d.p[p] = src[p]; d.pitch[p] = pitch[p];
        } else if ((rc = tmfh_upload(&v->c, 2 * slot + p, src[p], pitch[p], row, v->g.h, &d.p[p], &d.pitch[p]))) {
            return rc;
        }
        if (!tmfh_vec((uintptr_t)d.p[p] | d.pitch[p])) d.vec = 0;
    }
    if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(v->c.stream));
    v->desc[slot] = d;
    v->c.have[slot] = 1;
    return TM_OK;
}

int tm_haarpsi_compute_async(tm_haarpsi *v, uint32_t n_slots)
{
    if (!v) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&v->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = v->c.stream;
    memcpy(v->h_desc, v->desc.data(), n_slots * sizeof(TmHaarpsiDesc));
    TMFH_CHK(hipMemcpyAsync(v->d_desc, v->h_desc, n_slots * sizeof(TmHaarpsiDesc), hipMemcpyHostToDevice, stream));
    const TmHaarpsiGeom g = v->g;
#ifdef TM_EMULATE
    tm_haarpsi_host_test_launch(g, n_slots, v->d_desc, v->d_maps, v->d_cells, v->d_res);
#else
    const dim3 grid(g.cells, n_slots), block(TMP_THREADS);
#define TMP_LAUNCH(F) k_haarpsi<F><<<grid, block, 0, stream>>>(g, v->d_desc, v->d_maps, v->d_cells)
    TMP_DISPATCH(g, TMP_LAUNCH);
#undef TMP_LAUNCH
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    k_haarpsi_finish<<<dim3(n_slots), block, 0, stream>>>(g, v->d_cells, v->d_res);
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
#endif
    TMFH_CHK_QUEUED(&v->c, hipMemcpyAsync(v->h_res, v->d_res, n_slots * sizeof(TmHaarpsiCell), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&v->c, n_slots, 1);
    return TM_OK;
}

int tm_haarpsi_sync(tm_haarpsi *v) { return v ? tmfh_sync(&v->c) : TM_ERR_INVALID_ARG; }

int tm_haarpsi_get(tm_haarpsi *v, uint32_t first_slot, uint32_t n, tm_haarpsi_frame *out)
{
    if (!v || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&v->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&v->c);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        out[i].q = v->h_res[first_slot + i].q;
        out[i].ws = v->h_res[first_slot + i].ws;
    }
    return TM_OK;
}

int tm_haarpsi_map(tm_haarpsi *v, uint32_t slot, float *dst, size_t pitch)
{
    if (!v || !dst) return TM_ERR_INVALID_ARG;
    const TmHaarpsiGeom &g = v->g;
    const size_t row = (size_t)g.w2 * sizeof(float);
    if (pitch < row || (pitch & 3)) return TM_ERR_INVALID_ARG;
    if (!v->d_maps || slot >= v->c.n_last) return TM_ERR_STATE;
    const int rc = tmfh_sync(&v->c);
    if (rc) return rc;
    TMFH_CHK(hipSetDevice(v->c.device));
    TMFH_CHK(hipMemcpy2D(dst, pitch, v->d_maps + (size_t)slot * g.w2 * g.h2, row, row, g.h2, hipMemcpyDeviceToHost));
    return TM_OK;
}

} // extern "C"
