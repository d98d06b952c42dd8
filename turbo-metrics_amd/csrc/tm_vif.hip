// tm_vif.hip -- host side of libturbometrics_vif.so (include/turbo_metrics_vif.h): pair upload, one launch per scale and the
// finish.  Kernels: tm_vif_kernels.h; definition: DESIGN.md section 10; the host core it shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_vif.h"
#include "tm_vif_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMV_Y8 == TM_VIF_Y8 && TMV_Y16_MSB == TM_VIF_Y16_MSB && TMV_Y16_LOW == TM_VIF_Y16_LOW && TMV_Y10_PACKED == TM_VIF_Y10_PACKED, "layouts");
TMFH_FORMATS_AGREE;

} // namespace

struct tm_vif {
    TmVifGeom g;
    TmFeatureHost c;                                // have: [slot]; staging: [slot][2]
    TmVifDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmVifDesc> desc;                    // what set_pair wrote
    unsigned short *planes = nullptr;               // [slot]: the pictures of scales 1 .. 3
    double *d_cell = nullptr;                       // [slot][cells][2]: one (num, den) per workgroup
    double *d_res = nullptr, *h_res = nullptr;      // [slot][scale][2]
};

namespace {

template <int FMT>
void launch_scale0(const tm_vif *v, uint32_t n)
{
    k_vif<FMT, 0><<<dim3((unsigned)v->g.tiles[0], n), dim3(TMV_THREADS), 0, v->c.stream>>>(v->g, v->d_desc, v->planes, v->d_cell);
}

} // namespace

extern "C" {

void tm_vif_scores(const tm_vif_frame *f, double out[5])
{
    double num = 0.0, den = 0.0;
    for (int s = 0; s < 4; ++s) {
        out[s] = f->num[s] / f->den[s];
        num += f->num[s];
        den += f->den[s];
    }
    out[4] = num / den;
}

int tm_vif_create(tm_vif **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmVifGeom g;
    if (tmv_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    tm_vif *v = new tm_vif();
    v->g = g;
    const size_t B = batch_capacity, res = B * TMV_SCALES * 2 * sizeof(double);
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&v->c, batch_capacity, B, 2 * B))) { delete v; return rc; }
    if ((rc = tmfh_dev_alloc(&v->c, &v->planes, B * g.pslot * sizeof(unsigned short))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_cell, B * (size_t)g.cells * 2 * sizeof(double))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_desc, B * sizeof(TmVifDesc))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_res, res)) ||
        (rc = tmfh_pinned_alloc(&v->c, &v->h_desc, B * sizeof(TmVifDesc))) ||
        (rc = tmfh_pinned_alloc(&v->c, &v->h_res, res))) {
        tm_vif_destroy(v);
        return rc;
    }
    v->desc.assign(B, TmVifDesc{});
    *out = v;
    return TM_OK;
}

void tm_vif_destroy(tm_vif *v)
{
    if (!v) return;
    tmfh_close(&v->c, {v->planes, v->d_cell, v->d_desc, v->d_res}, {v->h_desc, v->h_res});
    delete v;
}

size_t tm_vif_mem_usage(const tm_vif *v) { return v ? v->c.bytes : 0; }

int tm_vif_set_pair(tm_vif *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem)
{
    if (!v || slot >= v->c.cap || !ref_y || !dis_y) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const size_t row = tmfh_row_bytes(v->g.fmt, v->g.w[0]);
    if (pitch_ref < row || pitch_dis < row) return TM_ERR_INVALID_ARG;
    if (((uintptr_t)ref_y | (uintptr_t)dis_y | pitch_ref | pitch_dis) & (tmfh_align(v->g.fmt) - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    if ((rc = tmfh_sync(&v->c))) return rc; // whatever `mem` is: the staging surfaces may still be read
    TMFH_CHK(hipSetDevice(v->c.device));
    const void *src[2] = {ref_y, dis_y};
    const size_t pitch[2] = {pitch_ref, pitch_dis};
    TmVifDesc d{};
    for (int p = 0; p < 2; ++p) {
        if (mem == TM_MEM_DEVICE) {
            d.p[p] = src[p]; d.pitch[p] = pitch[p];
        } else if ((rc = tmfh_upload(&v->c, 2 * slot + p, src[p], pitch[p], row, v->g.h[0], &d.p[p], &d.pitch[p]))) {
            return rc;
        }
        d.vec[p] = tmfh_vec((uintptr_t)d.p[p] | d.pitch[p]);
    }
    if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(v->c.stream));
    v->desc[slot] = d;
    v->c.have[slot] = 1;
    return TM_OK;
}

int tm_vif_compute_async(tm_vif *v, uint32_t n_slots)
{
    if (!v) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&v->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = v->c.stream;
    memcpy(v->h_desc, v->desc.data(), n_slots * sizeof(TmVifDesc));
    TMFH_CHK(hipMemcpyAsync(v->d_desc, v->h_desc, n_slots * sizeof(TmVifDesc), hipMemcpyHostToDevice, stream));
    const TmVifGeom &g = v->g;
    const dim3 block(TMV_THREADS);
    switch (g.fmt) {
    case TMX_F_U8: launch_scale0<TMX_F_U8>(v, n_slots); break;
    case TMX_F_U16_MSB: launch_scale0<TMX_F_U16_MSB>(v, n_slots); break;
    case TMX_F_U16_LOW: launch_scale0<TMX_F_U16_LOW>(v, n_slots); break;
    default: launch_scale0<TMX_F_P10>(v, n_slots); break;
    }
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    k_vif<TMX_F_HIST, 1><<<dim3((unsigned)g.tiles[1], n_slots), block, 0, stream>>>(g, v->d_desc, v->planes, v->d_cell);
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    k_vif<TMX_F_HIST, 2><<<dim3((unsigned)g.tiles[2], n_slots), block, 0, stream>>>(g, v->d_desc, v->planes, v->d_cell);
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    k_vif<TMX_F_HIST, 3><<<dim3((unsigned)g.tiles[3], n_slots), block, 0, stream>>>(g, v->d_desc, v->planes, v->d_cell);
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    k_vif_finish<<<dim3(TMV_SCALES, n_slots), block, 0, stream>>>(g, v->d_cell, v->d_res);
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    TMFH_CHK_QUEUED(&v->c, hipMemcpyAsync(v->h_res, v->d_res, (size_t)n_slots * TMV_SCALES * 2 * sizeof(double), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&v->c, n_slots, 1);
    return TM_OK;
}

int tm_vif_sync(tm_vif *v) { return v ? tmfh_sync(&v->c) : TM_ERR_INVALID_ARG; }

int tm_vif_get(tm_vif *v, uint32_t first_slot, uint32_t n, tm_vif_frame *out)
{
    if (!v || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&v->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&v->c);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const double *r = v->h_res + (size_t)(first_slot + i) * TMV_SCALES * 2;
        for (int s = 0; s < TMV_SCALES; ++s) {
            out[i].num[s] = r[2 * s];
            out[i].den[s] = r[2 * s + 1];
        }
    }
    return TM_OK;
}

} // extern "C"
