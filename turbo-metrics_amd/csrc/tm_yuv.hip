// tm_yuv.hip -- host side of libturbometrics_yuv.so (include/turbo_metrics_yuv.h): geometry of the definition,
// frame upload, the two launches per batch and the host functions.  Kernels: tm_yuv_kernels.h; the host core it shares:
// tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_yuv.h"
#include "tm_yuv_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMY_NV12 == TM_YUV_NV12 && TMY_P016 == TM_YUV_P016 && TMY_I420 == TM_YUV_I420 && TMY_I420P10 == TM_YUV_I420P10_PACKED, "layouts");

} // namespace

struct tm_yuv {
    TmYuvGeom g;
    TmFeatureHost c;                                // have, staging: [slot][side]
    TmYuvDesc *d_desc = nullptr, *h_desc = nullptr; // [slot][side]; h_desc is page-locked, copied at each compute
    std::vector<TmYuvDesc> desc;                    // what set_frame wrote
    float *d_maps = nullptr;                        // [slot][g.map_floats]: every value is written by every compute
    TmYuvCell *d_cells = nullptr;                   // [slot][g.cells]: likewise
    TmYuvRes *d_res = nullptr, *h_res = nullptr;    // [slot]
};

namespace {

// bytes of one luma / chroma row of this layout, and the number of chroma planes
void plane_rows(const tm_yuv *x, size_t *row_y, size_t *row_c, int *nc)
{
    const TmYuvGeom &g = x->g;
    const size_t bps = g.bits == 8 ? 1 : 2;
    switch (g.layout) {
    case TM_YUV_NV12: case TM_YUV_P016: *row_y = g.w * bps; *row_c = 2 * (size_t)g.pw[1] * bps; *nc = 1; break;
    case TM_YUV_I420: *row_y = g.w * bps; *row_c = g.pw[1] * bps; *nc = 2; break;
    default: *row_y = (size_t)tm_p10_row_words(g.w) * 4; *row_c = (size_t)tm_p10_row_words(g.pw[1]) * 4; *nc = 2; break;
    }
}

} // namespace

extern "C" {

double tm_yuv_psnr(uint64_t sse, uint64_t n_samples, uint32_t bits, double cap)
{
    if (bits < 8 || bits > 16) return NAN;
    if (sse == 0) return cap > 0 ? cap : INFINITY;
    const double mx = (double)((1ull << bits) - 1);
    const double v = 10.0 * log10(((mx * mx) * (double)n_samples) / (double)sse);
    return cap > 0 && v > cap ? cap : v;
}

double tm_yuv_ssim_db(double s)
{
    if (s >= 1.0) return INFINITY;
    return -10.0 * log10(1.0 - s);
}

double tm_yuv_ssim_all(const double ssim[3], uint32_t w, uint32_t h)
{
    const double ny = (double)w * (double)h, nc = (double)((w + 1) / 2) * (double)((h + 1) / 2);
    return (ny * ssim[0] + nc * ssim[1] + nc * ssim[2]) / (ny + nc + nc);
}

int tm_yuv_map_size(uint32_t w, uint32_t h, int plane, uint32_t *mw, uint32_t *mh)
{
    if (!mw || !mh || plane < 0 || plane > 2) return TM_ERR_INVALID_ARG;
    if (w < 16 || h < 16) return TM_ERR_UNSUPPORTED;
    const uint32_t pw = plane ? (uint32_t)(((uint64_t)w + 1) / 2) : w, ph = plane ? (uint32_t)(((uint64_t)h + 1) / 2) : h;
    *mw = (pw >> 2) - 1; *mh = (ph >> 2) - 1;
    return TM_OK;
}

int tm_yuv_create(tm_yuv **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmYuvGeom g;
    if (tmy_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launch's grid y
    tm_yuv *x = new tm_yuv();
    x->g = g;
    const size_t B = batch_capacity;
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&x->c, batch_capacity, B * 2, B * 2))) { delete x; return rc; }
    if ((rc = tmfh_dev_alloc(&x->c, &x->d_desc, B * 2 * sizeof(TmYuvDesc))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_maps, B * g.map_floats * sizeof(float))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_cells, B * g.cells * sizeof(TmYuvCell))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_res, B * sizeof(TmYuvRes))) ||
        (rc = tmfh_pinned_alloc(&x->c, &x->h_desc, B * 2 * sizeof(TmYuvDesc))) ||
        (rc = tmfh_pinned_alloc(&x->c, &x->h_res, B * sizeof(TmYuvRes)))) {
        tm_yuv_destroy(x);
        return rc;
    }
    x->desc.assign(B * 2, TmYuvDesc{});
    *out = x;
    return TM_OK;
}

void tm_yuv_destroy(tm_yuv *x)
{
    if (!x) return;
    tmfh_close(&x->c, {x->d_desc, x->d_maps, x->d_cells, x->d_res}, {x->h_desc, x->h_res});
    delete x;
}

size_t tm_yuv_mem_usage(const tm_yuv *x) { return x ? x->c.bytes : 0; }

int tm_yuv_set_frame(tm_yuv *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y,
                     size_t pitch_uv, int mem)
{
    if (!x || slot >= x->c.cap || (side != TM_SIDE_REF && side != TM_SIDE_DIS) || !y || !u) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const TmYuvGeom &g = x->g;
    const bool biplanar = g.layout == TM_YUV_NV12 || g.layout == TM_YUV_P016;
    if (biplanar) v = nullptr;
    else if (!v) return TM_ERR_INVALID_ARG;
    size_t row_y, row_c;
    int nc;
    plane_rows(x, &row_y, &row_c, &nc);
    if (pitch_y < row_y || pitch_uv < row_c) return TM_ERR_INVALID_ARG;
    const size_t align = g.layout == TM_YUV_I420P10_PACKED ? 4 : (g.bits == 8 ? 1 : 2);
    if (((uintptr_t)y | (uintptr_t)u | (uintptr_t)v | pitch_y | pitch_uv) & (align - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    // not for TM_MEM_DEVICE: the staging surface may still be read; a device surface is only noted in a host-side descriptor
    if (mem != TM_MEM_DEVICE && (rc = tmfh_sync(&x->c))) return rc;
    TMFH_CHK(hipSetDevice(x->c.device));
    const size_t idx = (size_t)slot * 2 + side;
    const void *p[3] = {y, u, v};
    unsigned long long pitch[2] = {pitch_y, pitch_uv};
    if (mem != TM_MEM_DEVICE) {
        if ((rc = tmfh_upload_420(&x->c, idx, y, u, v, pitch_y, pitch_uv, row_y, row_c, g.h, g.ph[1], nc, p, pitch))) return rc;
        if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(x->c.stream));
    }
    TmYuvDesc d{};
    d.p0 = p[0]; d.p1 = p[1]; d.p2 = p[2]; d.pitch = pitch[0]; d.pitch2 = pitch[1];
    d.vec = tmfh_vec((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2);
    x->desc[idx] = d;
    x->c.have[idx] = 1;
    return TM_OK;
}

int tm_yuv_compute_async(tm_yuv *x, uint32_t n_slots)
{
    if (!x) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&x->c, n_slots, 2);
    if (rc) return rc;
    hipStream_t stream = x->c.stream;
    memcpy(x->h_desc, x->desc.data(), 2 * n_slots * sizeof(TmYuvDesc));
    TMFH_CHK(hipMemcpyAsync(x->d_desc, x->h_desc, 2 * n_slots * sizeof(TmYuvDesc), hipMemcpyHostToDevice, stream));
    const TmYuvGeom g = x->g;
    const dim3 grid(g.grid, n_slots), block(TMY_THREADS);
#define TMY_LAUNCH(L, F) k_yuv<L, F><<<grid, block, 0, stream>>>(g, x->d_desc, x->d_maps, x->d_cells)
    TMY_DISPATCH(g, TMY_LAUNCH);
#undef TMY_LAUNCH
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    k_yuv_finish<<<dim3(n_slots), block, 0, stream>>>(g, x->d_cells, x->d_res);
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    TMFH_CHK_QUEUED(&x->c, hipMemcpyAsync(x->h_res, x->d_res, n_slots * sizeof(TmYuvRes), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&x->c, n_slots, 2);
    return TM_OK;
}

int tm_yuv_sync(tm_yuv *x) { return x ? tmfh_sync(&x->c) : TM_ERR_INVALID_ARG; }

int tm_yuv_get(tm_yuv *x, uint32_t first_slot, uint32_t n, tm_yuv_frame *out)
{
    if (!x || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&x->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    const TmYuvGeom &g = x->g;
    for (uint32_t i = 0; i < n; ++i) {
        const TmYuvRes &r = x->h_res[first_slot + i];
        for (int p = 0; p < 3; ++p) {
            const int c = p != 0;
            out[i].sse[p] = r.sse[p];
            out[i].ssim_sum[p] = r.ssim_sum[p];
            out[i].ssim[p] = r.ssim_sum[p] / (double)((uint64_t)(g.bw[c] - 1) * (g.bh[c] - 1));
        }
    }
    return TM_OK;
}

int tm_yuv_get_ssim_map(tm_yuv *x, uint32_t slot, int plane, float *dst, size_t pitch)
{
    if (!x || !dst || plane < 0 || plane > 2) return TM_ERR_INVALID_ARG;
    const TmYuvGeom &g = x->g;
    const int c = plane != 0;
    const size_t mw = g.bw[c] - 1, mh = g.bh[c] - 1;
    if (pitch < mw * sizeof(float) || (pitch & 3)) return TM_ERR_INVALID_ARG;
    if (slot >= x->c.n_last) return TM_ERR_STATE;
    const int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    TMFH_CHK(hipSetDevice(x->c.device));
    const float *src = x->d_maps + (size_t)slot * g.map_floats + g.map_off[plane];
    TMFH_CHK(hipMemcpy2D(dst, pitch, src, mw * sizeof(float), mw * sizeof(float), mh, hipMemcpyDeviceToHost));
    return TM_OK;
}

} // extern "C"
