// tm_xpsnr.hip -- host side of libturbometrics_xpsnr.so (include/turbo_metrics_xpsnr.h): geometry of the definition
// (DESIGN.md section 8), frame upload, the two launches per batch and the double-buffered history.  Kernels: tm_xpsnr_kernels.h; the
// host core it shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_xpsnr.h"
#include "tm_xpsnr_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMX_NV12 == TM_XPSNR_NV12 && TMX_P016 == TM_XPSNR_P016 && TMX_I420 == TM_XPSNR_I420 && TMX_I420P10 == TM_XPSNR_I420P10_PACKED, "layouts");

} // namespace

struct tm_xpsnr {
    TmXpsnrGeom g;
    int layout;
    uint32_t bits;
    TmFeatureHost c;                                  // have, staging: [slot][side]
    TmXpsnrDesc *d_desc = nullptr, *h_desc = nullptr; // [slot][side]; h_desc is page-locked, copied at each compute
    std::vector<TmXpsnrDesc> desc;                    // what set_frame wrote
    unsigned short *hist[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; // [buffer][m1, m2]
    int parity = 0;                                   // the next launch reads hist[parity] and writes hist[parity ^ 1]
    unsigned long long *d_blk = nullptr, *d_res = nullptr, *h_res = nullptr;
    double *d_wgt = nullptr;
};

namespace {

// bytes of one luma / chroma row of this layout, and the number of chroma planes
void plane_rows(const tm_xpsnr *x, size_t *row_y, size_t *row_c, int *nc)
{
    const TmXpsnrGeom &g = x->g;
    const size_t bps = x->bits == 8 ? 1 : 2;
    switch (x->layout) {
    case TM_XPSNR_NV12: case TM_XPSNR_P016: *row_y = g.w * bps; *row_c = 2 * (size_t)g.cw * bps; *nc = 1; break;
    case TM_XPSNR_I420: *row_y = g.w * bps; *row_c = g.cw * bps; *nc = 2; break;
    default: *row_y = (size_t)tm_p10_row_words(g.w) * 4; *row_c = (size_t)tm_p10_row_words(g.cw) * 4; *nc = 2; break;
    }
}

} // namespace

extern "C" {

uint32_t tm_xpsnr_block_size(uint32_t w, uint32_t h)
{
    return tmx_block_size(w, h);
}

double tm_xpsnr_from_wsse(uint64_t wsse, uint32_t plane_w, uint32_t plane_h, uint32_t bits)
{
    if (wsse == 0) return INFINITY;
    const uint64_t peak = (1ull << bits) - 1;
    const double num = (double)((uint64_t)plane_w * plane_h * peak * peak);
    const double s = sqrt((double)wsse);
    return 10.0 * log10(num / (s * s));
}

double tm_xpsnr_sequence(double sum_sqrt_wsse, double sum_xpsnr, uint64_t n_frames, uint32_t plane_w, uint32_t plane_h, uint32_t bits)
{
    if (n_frames == 0) return NAN;
    const double n = (double)n_frames;
    if (sum_sqrt_wsse >= n) {
        const uint64_t peak = (1ull << bits) - 1;
        const double num = (double)((uint64_t)plane_w * plane_h * peak * peak);
        const double m = sum_sqrt_wsse / n;
        return 10.0 * log10(num / (m * m));
    }
    return sum_xpsnr / n;
}

int tm_xpsnr_create(tm_xpsnr **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t fps_num, uint32_t fps_den,
                    uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (w == 0 || h == 0 || fps_num == 0 || fps_den == 0 || batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmXpsnrGeom g;
    if (tmx_make_geom(&g, w, h, layout, bits, fps_num, fps_den)) return TM_ERR_UNSUPPORTED;
    tm_xpsnr *x = new tm_xpsnr();
    x->g = g; x->layout = layout; x->bits = bits;
    const size_t B = batch_capacity, hist = (size_t)g.hpitch * g.h * sizeof(unsigned short);
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&x->c, batch_capacity, B * 2, B * 2))) { delete x; return rc; }
    if ((rc = tmfh_dev_alloc(&x->c, &x->hist[0][0], hist)) || (rc = tmfh_dev_alloc(&x->c, &x->hist[0][1], hist)) ||
        (rc = tmfh_dev_alloc(&x->c, &x->hist[1][0], hist)) || (rc = tmfh_dev_alloc(&x->c, &x->hist[1][1], hist)) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_desc, B * 2 * sizeof(TmXpsnrDesc))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_blk, B * g.nblk * 5 * sizeof(unsigned long long))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_wgt, B * g.nblk * sizeof(double))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_res, B * 3 * sizeof(unsigned long long))) ||
        (rc = tmfh_pinned_alloc(&x->c, &x->h_desc, B * 2 * sizeof(TmXpsnrDesc))) ||
        (rc = tmfh_pinned_alloc(&x->c, &x->h_res, B * 3 * sizeof(unsigned long long)))) {
        tm_xpsnr_destroy(x);
        return rc;
    }
    x->desc.assign(B * 2, TmXpsnrDesc{});
    if ((rc = tm_xpsnr_reset(x))) { tm_xpsnr_destroy(x); return rc; }
    *out = x;
    return TM_OK;
}

void tm_xpsnr_destroy(tm_xpsnr *x)
{
    if (!x) return;
    tmfh_close(&x->c, {x->hist[0][0], x->hist[0][1], x->hist[1][0], x->hist[1][1], x->d_desc, x->d_blk, x->d_wgt, x->d_res}, {x->h_desc, x->h_res});
    delete x;
}

size_t tm_xpsnr_mem_usage(const tm_xpsnr *x) { return x ? x->c.bytes : 0; }

int tm_xpsnr_set_frame(tm_xpsnr *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y,
                       size_t pitch_uv, int mem)
{
    if (!x || slot >= x->c.cap || (side != TM_SIDE_REF && side != TM_SIDE_DIS) || !y || !u) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const bool biplanar = x->layout == TM_XPSNR_NV12 || x->layout == TM_XPSNR_P016;
    if (biplanar) v = nullptr;
    else if (!v) return TM_ERR_INVALID_ARG;
    size_t row_y, row_c;
    int nc;
    plane_rows(x, &row_y, &row_c, &nc);
    if (pitch_y < row_y || pitch_uv < row_c) return TM_ERR_INVALID_ARG;
    const size_t align = x->layout == TM_XPSNR_I420P10_PACKED ? 4 : (x->bits == 8 ? 1 : 2);
    if (((uintptr_t)y | (uintptr_t)u | (uintptr_t)v | pitch_y | pitch_uv) & (align - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    if ((rc = tmfh_sync(&x->c))) return rc; // whatever `mem` is: the staging surfaces may still be read
    TMFH_CHK(hipSetDevice(x->c.device));
    const size_t idx = (size_t)slot * 2 + side;
    const void *p[3] = {y, u, v};
    unsigned long long pitch[2] = {pitch_y, pitch_uv};
    if (mem != TM_MEM_DEVICE) {
        if ((rc = tmfh_upload_420(&x->c, idx, y, u, v, pitch_y, pitch_uv, row_y, row_c, x->g.h, x->g.ch, nc, p, pitch))) return rc;
        if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(x->c.stream));
    }
    TmXpsnrDesc d{};
    d.p0 = p[0]; d.p1 = p[1]; d.p2 = p[2]; d.pitch = pitch[0]; d.pitch2 = pitch[1];
    d.vec = tmfh_vec((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2);
    x->desc[idx] = d;
    x->c.have[idx] = 1;
    return TM_OK;
}

int tm_xpsnr_compute_async(tm_xpsnr *x, uint32_t n_slots)
{
    if (!x) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&x->c, n_slots, 2);
    if (rc) return rc;
    hipStream_t stream = x->c.stream;
    memcpy(x->h_desc, x->desc.data(), 2 * n_slots * sizeof(TmXpsnrDesc));
    TMFH_CHK(hipMemcpyAsync(x->d_desc, x->h_desc, 2 * n_slots * sizeof(TmXpsnrDesc), hipMemcpyHostToDevice, stream));
    TmXpsnrGeom g = x->g;
    g.n = (int)n_slots;
    unsigned short *const *hin = x->hist[x->parity], *const *hout = x->hist[x->parity ^ 1];
    k_xpsnr_blocks<<<dim3((unsigned)g.nblk, n_slots), dim3(TMX_THREADS), 0, stream>>>(g, x->d_desc, hin[0], hin[1], hout[0], hout[1], x->d_blk);
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    k_xpsnr_finish<<<dim3((n_slots + 63) / 64), dim3(64), 0, stream>>>(g, x->d_blk, x->d_wgt, x->d_res);
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    TMFH_CHK_QUEUED(&x->c, hipMemcpyAsync(x->h_res, x->d_res, n_slots * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    x->parity ^= 1;
    tmfh_queued(&x->c, n_slots, 2);
    return TM_OK;
}

int tm_xpsnr_sync(tm_xpsnr *x) { return x ? tmfh_sync(&x->c) : TM_ERR_INVALID_ARG; }

int tm_xpsnr_get(tm_xpsnr *x, uint32_t first_slot, uint32_t n, tm_xpsnr_frame *out)
{
    if (!x || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&x->c, first_slot, n)) return TM_ERR_STATE;
    int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    const TmXpsnrGeom &g = x->g;
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned long long *r = x->h_res + (size_t)(first_slot + i) * 3;
        for (int c = 0; c < 3; ++c) {
            out[i].wsse[c] = r[c];
            out[i].xpsnr[c] = tm_xpsnr_from_wsse(r[c], c ? g.cw : g.w, c ? g.ch : g.h, x->bits);
        }
    }
    return TM_OK;
}

int tm_xpsnr_reset(tm_xpsnr *x)
{
    if (!x) return TM_ERR_INVALID_ARG;
    int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    TMFH_CHK(hipSetDevice(x->c.device));
    const size_t hist = (size_t)x->g.hpitch * x->g.h * sizeof(unsigned short);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) TMFH_CHK(hipMemsetAsync(x->hist[i][j], 0, hist, x->c.stream));
    TMFH_CHK(hipStreamSynchronize(x->c.stream));
    x->parity = 0;
    std::fill(x->c.have.begin(), x->c.have.end(), 0);
    return TM_OK;
}

} // extern "C"
