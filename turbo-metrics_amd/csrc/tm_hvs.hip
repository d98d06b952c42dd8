// tm_hvs.hip -- host side of libturbometrics_hvs.so (include/turbo_metrics_hvs.h): pair upload, the two launches per batch and the
// host functions.  Kernels: tm_hvs_kernels.h; definition: DESIGN.md section 16; the host core it shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_hvs.h"
#include "tm_hvs_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMH_Y8 == TM_HVS_Y8 && TMH_Y16_MSB == TM_HVS_Y16_MSB && TMH_Y16_LOW == TM_HVS_Y16_LOW && TMH_Y10_PACKED == TM_HVS_Y10_PACKED, "layouts");
TMFH_FORMATS_AGREE;

// the host's copies of the kernel's tables
const float kHostCsf[64] = TMH_CSF_VALUES;
const float kHostMask[64] = TMH_MASK_VALUES;

} // namespace

struct tm_hvs {
    TmHvsGeom g;
    TmFeatureHost c;                                // have: [slot]; staging: [slot][2]
    TmHvsDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmHvsDesc> desc;                    // what set_pair wrote
    TmHvsCell *d_cells = nullptr;                   // [slot][g.cells]: every cell is written by every compute
    TmHvsCell *d_res = nullptr, *h_res = nullptr;   // [slot]
};

extern "C" {

double tm_hvs_psnr(double s, uint64_t blocks, uint32_t bits)
{
    if (bits < 8 || bits > 16 || blocks == 0) return NAN;
    if (s == 0.0) return INFINITY;
    const double peak = (double)((1ull << bits) - 1);
    return 10.0 * log10(((peak * peak) * (64.0 * (double)blocks)) / s);
}

const float *tm_hvs_csf(void) { return kHostCsf; }
const float *tm_hvs_mask(void) { return kHostMask; }

int tm_hvs_create(tm_hvs **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmHvsGeom g;
    if (tmh_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launch's grid y
    tm_hvs *v = new tm_hvs();
    v->g = g;
    const size_t B = batch_capacity;
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&v->c, batch_capacity, B, 2 * B))) { delete v; return rc; }
    if ((rc = tmfh_dev_alloc(&v->c, &v->d_cells, B * (size_t)g.cells * sizeof(TmHvsCell))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_desc, B * sizeof(TmHvsDesc))) ||
        (rc = tmfh_dev_alloc(&v->c, &v->d_res, B * sizeof(TmHvsCell))) ||
        (rc = tmfh_pinned_alloc(&v->c, &v->h_desc, B * sizeof(TmHvsDesc))) ||
        (rc = tmfh_pinned_alloc(&v->c, &v->h_res, B * sizeof(TmHvsCell)))) {
        tm_hvs_destroy(v);
        return rc;
    }
    v->desc.assign(B, TmHvsDesc{});
    *out = v;
    return TM_OK;
}

void tm_hvs_destroy(tm_hvs *v)
{
    if (!v) return;
    tmfh_close(&v->c, {v->d_cells, v->d_desc, v->d_res}, {v->h_desc, v->h_res});
    delete v;
}

size_t tm_hvs_mem_usage(const tm_hvs *v) { return v ? v->c.bytes : 0; }

int tm_hvs_set_pair(tm_hvs *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem)
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
    TmHvsDesc d{};
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

int tm_hvs_compute_async(tm_hvs *v, uint32_t n_slots)
{
    if (!v) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&v->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = v->c.stream;
    memcpy(v->h_desc, v->desc.data(), n_slots * sizeof(TmHvsDesc));
    TMFH_CHK(hipMemcpyAsync(v->d_desc, v->h_desc, n_slots * sizeof(TmHvsDesc), hipMemcpyHostToDevice, stream));
    const TmHvsGeom g = v->g;
    const dim3 grid(g.cells, n_slots), block(TMH_THREADS);
#define TMH_LAUNCH(F) k_hvs<F><<<grid, block, 0, stream>>>(g, v->d_desc, v->d_cells)
    TMH_DISPATCH(g, TMH_LAUNCH);
#undef TMH_LAUNCH
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    k_hvs_finish<<<dim3(n_slots), block, 0, stream>>>(g, v->d_cells, v->d_res);
    TMFH_CHK_QUEUED(&v->c, hipGetLastError());
    TMFH_CHK_QUEUED(&v->c, hipMemcpyAsync(v->h_res, v->d_res, n_slots * sizeof(TmHvsCell), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&v->c, n_slots, 1);
    return TM_OK;
}

int tm_hvs_sync(tm_hvs *v) { return v ? tmfh_sync(&v->c) : TM_ERR_INVALID_ARG; }

int tm_hvs_get(tm_hvs *v, uint32_t first_slot, uint32_t n, tm_hvs_frame *out)
{
    if (!v || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&v->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&v->c);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        out[i].s_hvs = v->h_res[first_slot + i].s_hvs;
        out[i].s_hvsm = v->h_res[first_slot + i].s_hvsm;
        out[i].blocks = (uint64_t)v->g.bw * v->g.bh;
    }
    return TM_OK;
}

} // extern "C"
