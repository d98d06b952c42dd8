// tm_gmsd.hip -- host side of libturbometrics_gmsd.so (include/turbo_metrics_gmsd.h): pair upload, the two launches per batch, the map
// read-back and the host functions.  Kernels: tm_gmsd_kernels.h; definition: DESIGN.md section 20; the host core it shares:
// tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_gmsd.h"
#include "tm_gmsd_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMG_Y8 == TM_GMSD_Y8 && TMG_Y16_MSB == TM_GMSD_Y16_MSB && TMG_Y16_LOW == TM_GMSD_Y16_LOW && TMG_Y10_PACKED == TM_GMSD_Y10_PACKED, "layouts");
TMFH_FORMATS_AGREE;

} // namespace

#ifdef TM_EMULATE
// tests/host/gmsd_host_test.cpp compiles this file with a host compiler against a fake runtime, where nothing can be launched: the two
// launches are the test's own function
void tm_gmsd_host_test_launch(const TmGmsdGeom &g, unsigned n_slots, const TmGmsdDesc *desc, float *maps, TmGmsdCell *cells, TmGmsdCell *res);
#endif

struct tm_gmsd {
    TmGmsdGeom g;
    TmFeatureHost c;                                  // have: [slot]; staging: [slot][2]
    TmGmsdDesc *d_desc = nullptr, *h_desc = nullptr;  // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmGmsdDesc> desc;                     // what set_pair wrote
    float *d_maps = nullptr;                          // TM_GMSD_MAPS: [slot][g.h2][g.w2]: every value is written by every compute
    TmGmsdCell *d_cells = nullptr;                    // [slot][g.cells]: every cell is written by every compute
    TmGmsdCell *d_res = nullptr, *h_res = nullptr;    // [slot]
};

extern "C" {

double tm_gmsd_score(double e1, double e2, uint64_t n, int population)
{
    if (n < 2) return NAN;
    const double N = (double)n;
    const double var = (e2 - e1 * e1 / N) / (population ? N : N - 1.0);
    return sqrt(var > 0.0 ? var : 0.0);
}

double tm_gmsd_mean(double e1, uint64_t n)
{
    if (n < 2) return NAN;
    return 1.0 - e1 / (double)n;
}

int tm_gmsd_create(tm_gmsd **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity, uint32_t flags)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0 || (flags & ~(uint32_t)TM_GMSD_MAPS)) return TM_ERR_INVALID_ARG;
    TmGmsdGeom g;
    if (tmg_make_geom(&g, w, h, layout, bits, (flags & TM_GMSD_MAPS) != 0)) return TM_ERR_UNSUPPORTED;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launch's grid y
    tm_gmsd *v = new tm_gmsd();
    v->g = g;
    const size_t B = batch_capacity;
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&v->c, batch_capacity, B, 2 * B))) { delete v; return rc; }
    if ((rc = tmfh_dev_alloc(&v->c, &v->d_cells, B * (size_t)g.cells * sizeof(TmGmsdCell))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_desc, B * sizeof(TmGmsdDesc))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_res, B * sizeof(TmGmsdCell))) ||
        (g.maps && (rc = tmfh_dev_alloc(&v->c, &v->d_maps, B * (size_t)g.w2 * g.h2 * sizeof(float)))) ||
        (rc = tmfh_pinned_alloc(&v->c, &v->h_desc, B * sizeof(TmGmsdDesc))) ||
        (rc = tmfh_pinned_alloc(&v->c, &v->h_res, B * sizeof(TmGmsdCell)))) {
        tm_gmsd_destroy(v);
        return rc;
    }
    v->desc.assign(B, TmGmsdDesc{});
    *out = v;
    return TM_OK;
}

void tm_gmsd_destroy(tm_gmsd *v)
{
    if (!v) return;
    tmfh_close(&v->c, {v->d_cells, v->d_desc, v->d_res, v->d_maps}, {v->h_desc, v->h_res});
    delete v;
}

size_t tm_gmsd_mem_usage(const tm_gmsd *v) { return v ? v->c.bytes : 0; }

int tm_gmsd_set_pair(tm_gmsd *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem)
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
    TmGmsdDesc d{};
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

int tm_gmsd_compute_async(tm_gmsd *v, uint32_t n_slots)
{
    if (!v) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&v->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = v->c.stream;
    memcpy(v->h_desc, v->desc.data(), n_slots * sizeof(TmGmsdDesc));
    TMFH_CHK(hipMemcpyAsync(v->d_desc, v->h_desc, n_slots * sizeof(TmGmsdDesc), hipMemcpyHostToDevice, stream));
    const TmGmsdGeom g = v->g;
#ifdef TM_EMULATE
    tm_gmsd_host_test_launch(g, n_slots, v->d_desc, v->d_maps, v->d_cells, v->d_res);
#else
    const dim3 grid(g.cells, n_slots), block(TMG_THREADS);
#define TMG_LAUNCH(F) k_gmsd<F><<<grid, block, 0, stream>>>(g, v->d_desc, v->d_maps, v->d_cells)
    TMG_DISPATCH(g, TMG_LAUNCH);
#undef TMG_LAUNCH
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    k_gmsd_finish<<<dim3(n_slots), block, 0, stream>>>(g, v->d_cells, v->d_res);
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
#endif
    TMFH_CHK_QUEUED(&v->c, hipMemcpyAsync(v->h_res, v->d_res, n_slots * sizeof(TmGmsdCell), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&v->c, n_slots, 1);
    return TM_OK;
}

int tm_gmsd_sync(tm_gmsd *v) { return v ? tmfh_sync(&v->c) : TM_ERR_INVALID_ARG; }

int tm_gmsd_get(tm_gmsd *v, uint32_t first_slot, uint32_t n, tm_gmsd_frame *out)
{
    if (!v || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&v->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&v->c);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        out[i].e1 = v->h_res[first_slot + i].e1;
        out[i].e2 = v->h_res[first_slot + i].e2;
        out[i].e_max = v->h_res[first_slot + i].e_max;
        out[i].n = (uint64_t)v->g.w2 * v->g.h2;
    }
    return TM_OK;
}

int tm_gmsd_map(tm_gmsd *v, uint32_t slot, float *dst, size_t pitch)
{
    if (!v || !dst) return TM_ERR_INVALID_ARG;
    const TmGmsdGeom &g = v->g;
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
