// tm_motion.hip -- host side of libturbometrics_motion.so (include/turbo_metrics_motion.h): frame upload, one launch per batch
// and the history plane.  Kernel: tm_motion_kernels.h; definition: DESIGN.md section 9; the host core it shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_motion.h"
#include "tm_motion_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMM_Y8 == TM_MOTION_Y8 && TMM_Y16_MSB == TM_MOTION_Y16_MSB && TMM_Y16_LOW == TM_MOTION_Y16_LOW && TMM_Y10_PACKED == TM_MOTION_Y10_PACKED, "layouts");
TMFH_FORMATS_AGREE;

} // namespace

struct tm_motion {
    TmMotionGeom g;
    TmFeatureHost c;                                   // have, staging: [slot]
    TmMotionDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmMotionDesc> desc;                    // what set_frame wrote
    unsigned short *hist = nullptr;                    // the last blurred picture of the sequence
    unsigned long long *d_sad = nullptr, *h_sad = nullptr; // [slot][TMM_BINS]
    bool first = true;                                 // the next compute starts a sequence
};

extern "C" {

double tm_motion_from_sad(uint64_t sad, uint32_t w, uint32_t h)
{
    const float scaled = (float)((double)sad / 256.0);
    return (double)(scaled / (float)((uint64_t)w * h));
}

double tm_motion2(double motion_i, double motion_next) { return motion_next < motion_i ? motion_next : motion_i; }

int tm_motion_create(tm_motion **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmMotionGeom g;
    if (tmm_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    tm_motion *m = new tm_motion();
    m->g = g;
    const size_t B = batch_capacity, res = B * TMM_BINS * sizeof(unsigned long long);
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&m->c, batch_capacity, B, B))) { delete m; return rc; }
    if ((rc = tmfh_dev_alloc(&m->c, &m->hist, (size_t)g.hpitch * g.h * sizeof(unsigned short))) ||
        (rc = tmfh_dev_alloc(&m->c, &m->d_desc, B * sizeof(TmMotionDesc))) ||
        (rc = tmfh_dev_alloc(&m->c, &m->d_sad, res)) ||
        (rc = tmfh_pinned_alloc(&m->c, &m->h_desc, B * sizeof(TmMotionDesc))) ||
        (rc = tmfh_pinned_alloc(&m->c, &m->h_sad, res))) {
        tm_motion_destroy(m);
        return rc;
    }
    m->desc.assign(B, TmMotionDesc{});
    *out = m;
    return TM_OK;
}

void tm_motion_destroy(tm_motion *m)
{
    if (!m) return;
    tmfh_close(&m->c, {m->hist, m->d_desc, m->d_sad}, {m->h_desc, m->h_sad});
    delete m;
}

size_t tm_motion_mem_usage(const tm_motion *m) { return m ? m->c.bytes : 0; }

int tm_motion_set_frame(tm_motion *m, uint32_t slot, const void *y, size_t pitch_y, int mem)
{
    if (!m || slot >= m->c.cap || !y) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const size_t row = tmfh_row_bytes(m->g.fmt, m->g.w);
    if (pitch_y < row) return TM_ERR_INVALID_ARG;
    if (((uintptr_t)y | pitch_y) & (tmfh_align(m->g.fmt) - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    if ((rc = tmfh_sync(&m->c))) return rc; // whatever `mem` is: the staging surfaces may still be read
    TMFH_CHK(hipSetDevice(m->c.device));
    TmMotionDesc d{};
    if (mem == TM_MEM_DEVICE) {
        d.p = y; d.pitch = pitch_y;
    } else {
        if ((rc = tmfh_upload(&m->c, slot, y, pitch_y, row, m->g.h, &d.p, &d.pitch))) return rc;
        if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(m->c.stream));
    }
    d.vec = tmfh_vec((uintptr_t)d.p | d.pitch);
    m->desc[slot] = d;
    m->c.have[slot] = 1;
    return TM_OK;
}

int tm_motion_compute_async(tm_motion *m, uint32_t n_slots)
{
    if (!m) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&m->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = m->c.stream;
    memcpy(m->h_desc, m->desc.data(), n_slots * sizeof(TmMotionDesc));
    TMFH_CHK(hipMemcpyAsync(m->d_desc, m->h_desc, n_slots * sizeof(TmMotionDesc), hipMemcpyHostToDevice, stream));
    const size_t res = (size_t)n_slots * TMM_BINS * sizeof(unsigned long long);
    TMFH_CHK_QUEUED(&m->c, hipMemsetAsync(m->d_sad, 0, res, stream));
    TmMotionGeom g = m->g;
    g.n = (int)n_slots;
    g.first = m->first;
    const dim3 grid((unsigned)g.tiles), block(TMM_THREADS);
    switch (g.fmt) {
    case TMX_F_U8: k_motion<TMX_F_U8><<<grid, block, 0, stream>>>(g, m->d_desc, m->hist, m->d_sad); break;
    case TMX_F_U16_MSB: k_motion<TMX_F_U16_MSB><<<grid, block, 0, stream>>>(g, m->d_desc, m->hist, m->d_sad); break;
    case TMX_F_U16_LOW: k_motion<TMX_F_U16_LOW><<<grid, block, 0, stream>>>(g, m->d_desc, m->hist, m->d_sad); break;
    default: k_motion<TMX_F_P10><<<grid, block, 0, stream>>>(g, m->d_desc, m->hist, m->d_sad); break;
    }
    TMFH_CHK_QUEUED(&m->c, hipGetLastError());
    TMFH_CHK_QUEUED(&m->c, hipMemcpyAsync(m->h_sad, m->d_sad, res, hipMemcpyDeviceToHost, stream));
    m->first = false;
    tmfh_queued(&m->c, n_slots, 1);
    return TM_OK;
}

int tm_motion_sync(tm_motion *m) { return m ? tmfh_sync(&m->c) : TM_ERR_INVALID_ARG; }

int tm_motion_get(tm_motion *m, uint32_t first_slot, uint32_t n, tm_motion_frame *out)
{
    if (!m || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&m->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&m->c);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned long long *r = m->h_sad + (size_t)(first_slot + i) * TMM_BINS;
        uint64_t sad = 0;
        for (int b = 0; b < TMM_BINS; ++b) sad += r[b];
        out[i].sad = sad;
        out[i].motion = tm_motion_from_sad(sad, (uint32_t)m->g.w, (uint32_t)m->g.h);
    }
    return TM_OK;
}

int tm_motion_reset(tm_motion *m)
{
    if (!m) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_sync(&m->c);
    if (rc) return rc;
    m->first = true;
    std::fill(m->c.have.begin(), m->c.have.end(), 0);
    return TM_OK;
}

} // extern "C"
