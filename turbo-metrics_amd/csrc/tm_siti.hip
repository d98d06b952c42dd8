// tm_siti.hip -- host side of libturbometrics_siti.so (include/turbo_metrics_siti.h): frame upload, one launch per batch and the
// history plane.  Kernel: tm_siti_kernels.h; definition: DESIGN.md section 19; the host core it shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_siti.h"
#include "tm_siti_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMI_Y8 == TM_SITI_Y8 && TMI_Y16_MSB == TM_SITI_Y16_MSB && TMI_Y16_LOW == TM_SITI_Y16_LOW && TMI_Y10_PACKED == TM_SITI_Y10_PACKED, "layouts");
TMFH_FORMATS_AGREE;

// sqrt(n b - a^2) / n, the radicand exact: n <= 2^26, b < 2^63, |a| < 2^45 for the sums of a picture the library accepts
double stddev(unsigned __int128 a_abs, uint64_t b, uint64_t n)
{
    if (n == 0) return 0.0;
    const unsigned __int128 nb = (unsigned __int128)n * b, aa = a_abs * a_abs;
    if (nb <= aa) return 0.0; // equal for a constant; below only for sums no picture has
    return std::sqrt((double)(nb - aa)) / (double)n;
}

} // namespace

#ifdef TM_EMULATE
// tests/host/siti_host_test.cpp compiles this file with a host compiler against a fake runtime, where nothing can be launched: the
// launch is the test's own function
void tm_siti_host_test_launch(const TmSitiGeom &g, const TmSitiDesc *desc, unsigned short *hist, unsigned long long *acc);
#endif

struct tm_siti {
    TmSitiGeom g;
    TmFeatureHost c;                                   // have, staging: [slot]
    TmSitiDesc *d_desc = nullptr, *h_desc = nullptr;   // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmSitiDesc> desc;                      // what set_frame wrote
    unsigned short *hist = nullptr;                    // the last picture of the sequence, its code values
    unsigned long long *d_acc = nullptr, *h_acc = nullptr; // [slot][TMI_BINS][TMI_SUMS]
    bool first = true;                                 // the next compute starts a sequence
    bool first_last = true;                            // slot 0 of the last compute started one
};

extern "C" {

double tm_siti_si(uint64_t s1, uint64_t s2, uint64_t n_si, double gain) { return gain * stddev(s1, s2, n_si) / 256.0; }

double tm_siti_ti(int64_t t1, uint64_t t2, uint64_t n, uint32_t bits, double gain)
{
    const unsigned __int128 a = t1 < 0 ? (unsigned __int128)(-(__int128)t1) : (unsigned __int128)t1;
    return gain * stddev(a, t2, n) / std::ldexp(1.0, (int)bits - 8);
}

int tm_siti_create(tm_siti **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmSitiGeom g;
    if (tmi_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    tm_siti *m = new tm_siti();
    m->g = g;
    const size_t B = batch_capacity, res = B * TMI_BINS * TMI_SUMS * sizeof(unsigned long long);
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&m->c, batch_capacity, B, B))) { delete m; return rc; }
    if ((rc = tmfh_dev_alloc(&m->c, &m->hist, (size_t)g.hpitch * g.h * sizeof(unsigned short))) ||
        (rc = tmfh_dev_alloc(&m->c, &m->d_desc, B * sizeof(TmSitiDesc))) ||
        (rc = tmfh_dev_alloc(&m->c, &m->d_acc, res)) ||
        (rc = tmfh_pinned_alloc(&m->c, &m->h_desc, B * sizeof(TmSitiDesc))) ||
        (rc = tmfh_pinned_alloc(&m->c, &m->h_acc, res))) {
        tm_siti_destroy(m);
        return rc;
    }
    m->desc.assign(B, TmSitiDesc{});
    *out = m;
    return TM_OK;
}

void tm_siti_destroy(tm_siti *m)
{
    if (!m) return;
    tmfh_close(&m->c, {m->hist, m->d_desc, m->d_acc}, {m->h_desc, m->h_acc});
    delete m;
}

size_t tm_siti_mem_usage(const tm_siti *m) { return m ? m->c.bytes : 0; }

int tm_siti_set_frame(tm_siti *m, uint32_t slot, const void *y, size_t pitch_y, int mem)
{
    if (!m || slot >= m->c.cap || !y) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const size_t row = tmfh_row_bytes(m->g.fmt, m->g.w);
    if (pitch_y < row) return TM_ERR_INVALID_ARG;
    if (((uintptr_t)y | pitch_y) & (tmfh_align(m->g.fmt) - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    if ((rc = tmfh_sync(&m->c))) return rc; // whatever `mem` is: the staging surfaces may still be read
    TMFH_CHK(hipSetDevice(m->c.device));
    TmSitiDesc d{};
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

int tm_siti_compute_async(tm_siti *m, uint32_t n_slots)
{
    if (!m) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&m->c, n_slots, 1);
    if (rc) return rc;
    hipStream_t stream = m->c.stream;
    memcpy(m->h_desc, m->desc.data(), n_slots * sizeof(TmSitiDesc));
    TMFH_CHK(hipMemcpyAsync(m->d_desc, m->h_desc, n_slots * sizeof(TmSitiDesc), hipMemcpyHostToDevice, stream));
    const size_t res = (size_t)n_slots * TMI_BINS * TMI_SUMS * sizeof(unsigned long long);
    TMFH_CHK_QUEUED(&m->c, hipMemsetAsync(m->d_acc, 0, res, stream));
    TmSitiGeom g = m->g;
    g.n = (int)n_slots;
    g.first = m->first;
#ifdef TM_EMULATE
    tm_siti_host_test_launch(g, m->d_desc, m->hist, m->d_acc);
#else
    const dim3 grid((unsigned)g.tiles), block(TMI_THREADS);
    switch (g.fmt) {
    case TMX_F_U8: k_siti<TMX_F_U8><<<grid, block, 0, stream>>>(g, m->d_desc, m->hist, m->d_acc); break;
    case TMX_F_U16_MSB: k_siti<TMX_F_U16_MSB><<<grid, block, 0, stream>>>(g, m->d_desc, m->hist, m->d_acc); break;
    case TMX_F_U16_LOW: k_siti<TMX_F_U16_LOW><<<grid, block, 0, stream>>>(g, m->d_desc, m->hist, m->d_acc); break;
    default: k_siti<TMX_F_P10><<<grid, block, 0, stream>>>(g, m->d_desc, m->hist, m->d_acc); break;
    }
#endif
    TMFH_CHK_QUEUED(&m->c, hipGetLastError());
    TMFH_CHK_QUEUED(&m->c, hipMemcpyAsync(m->h_acc, m->d_acc, res, hipMemcpyDeviceToHost, stream));
    m->first_last = m->first;
    m->first = false;
    tmfh_queued(&m->c, n_slots, 1);
    return TM_OK;
}

int tm_siti_sync(tm_siti *m) { return m ? tmfh_sync(&m->c) : TM_ERR_INVALID_ARG; }

int tm_siti_get(tm_siti *m, uint32_t first_slot, uint32_t n, tm_siti_frame *out)
{
    if (!m || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&m->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&m->c);
    if (rc) return rc;
    const uint64_t np = (uint64_t)m->g.w * m->g.h, ni = (uint64_t)(m->g.w - 2) * (m->g.h - 2);
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned long long *r = m->h_acc + (size_t)(first_slot + i) * TMI_BINS * TMI_SUMS;
        uint64_t v[TMI_SUMS] = {0, 0, 0, 0};
        for (int b = 0; b < TMI_BINS; ++b)
            for (int k = 0; k < TMI_SUMS; ++k) v[k] += r[b * TMI_SUMS + k];
        tm_siti_frame &f = out[i];
        f.s1 = v[0]; f.s2 = v[1];
        f.t1 = (int64_t)v[2]; f.t2 = v[3]; // the kernel adds T1 in two's complement
        f.ti_valid = !(first_slot + i == 0 && m->first_last);
        f.si = tm_siti_si(f.s1, f.s2, ni, 1.0);
        f.ti = f.ti_valid ? tm_siti_ti(f.t1, f.t2, np, (uint32_t)m->g.bits, 1.0) : 0.0;
    }
    return TM_OK;
}

int tm_siti_reset(tm_siti *m)
{
    if (!m) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_sync(&m->c);
    if (rc) return rc;
    m->first = true;
    std::fill(m->c.have.begin(), m->c.have.end(), 0);
    return TM_OK;
}

} // extern "C"
