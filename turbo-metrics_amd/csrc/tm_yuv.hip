// tm_yuv.hip -- host side of libturbometrics_yuv.so (include/turbo_metrics_yuv.h): geometry of the definition,
// frame upload, the two launches per batch and the host functions.  Kernels: tm_yuv_kernels.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_yuv.h"
#include "tm_yuv_kernels.h"

namespace {

static_assert(TMY_NV12 == TM_YUV_NV12 && TMY_P016 == TM_YUV_P016 && TMY_I420 == TM_YUV_I420 && TMY_I420P10 == TM_YUV_I420P10_PACKED, "layouts");

#define YCHK(call)                                      \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

} // namespace

struct tm_yuv {
    TmYuvGeom g;
    uint32_t cap;
    int device;
    hipStream_t stream = nullptr;
    TmYuvDesc *d_desc = nullptr, *h_desc = nullptr; // [slot][side]; h_desc is page-locked, copied at each compute
    std::vector<TmYuvDesc> desc;                    // what set_frame wrote
    std::vector<unsigned char> have;                // [slot][side]: set since the last compute
    std::vector<void *> staging;                    // [slot][side]: device copy of a host picture (lazily allocated)
    float *d_maps = nullptr;                        // [slot][g.map_floats]: every value is written by every compute
    TmYuvCell *d_cells = nullptr;                   // [slot][g.cells]: likewise
    TmYuvRes *d_res = nullptr, *h_res = nullptr;    // [slot]
    size_t bytes = 0;
    bool pending = false;
    uint32_t n_last = 0;
};

namespace {

int dev_alloc(tm_yuv *x, void **p, size_t n)
{
    const hipError_t r = hipMalloc(p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    YCHK(r);
    x->bytes += n;
    return TM_OK;
}

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
    int rc;
    // ---- first device call
    tm_yuv *x = new tm_yuv();
    x->g = g; x->cap = batch_capacity;
    auto fail = [&](int e) { tm_yuv_destroy(x); return e; };
    if (hipGetDevice(&x->device) != hipSuccess) { (void)hipGetLastError(); delete x; return TM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); x->stream = nullptr; return fail(TM_ERR_HIP); }
    const size_t B = batch_capacity;
    if ((rc = dev_alloc(x, (void **)&x->d_desc, B * 2 * sizeof(TmYuvDesc)))) return fail(rc);
    if ((rc = dev_alloc(x, (void **)&x->d_maps, B * g.map_floats * sizeof(float)))) return fail(rc);
    if ((rc = dev_alloc(x, (void **)&x->d_cells, B * g.cells * sizeof(TmYuvCell)))) return fail(rc);
    if ((rc = dev_alloc(x, (void **)&x->d_res, B * sizeof(TmYuvRes)))) return fail(rc);
    if (hipHostMalloc((void **)&x->h_desc, B * 2 * sizeof(TmYuvDesc), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); x->h_desc = nullptr; return fail(TM_ERR_OOM); }
    if (hipHostMalloc((void **)&x->h_res, B * sizeof(TmYuvRes), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); x->h_res = nullptr; return fail(TM_ERR_OOM); }
    x->bytes += B * 2 * sizeof(TmYuvDesc) + B * sizeof(TmYuvRes);
    x->desc.assign(B * 2, TmYuvDesc{});
    x->have.assign(B * 2, 0);
    x->staging.assign(B * 2, nullptr);
    *out = x;
    return TM_OK;
}

void tm_yuv_destroy(tm_yuv *x)
{
    if (!x) return;
    if (x->stream) (void)hipStreamSynchronize(x->stream);
    for (void *p : x->staging) if (p) (void)hipFree(p);
    if (x->d_desc) (void)hipFree(x->d_desc);
    if (x->d_maps) (void)hipFree(x->d_maps);
    if (x->d_cells) (void)hipFree(x->d_cells);
    if (x->d_res) (void)hipFree(x->d_res);
    if (x->h_desc) (void)hipHostFree(x->h_desc);
    if (x->h_res) (void)hipHostFree(x->h_res);
    if (x->stream) (void)hipStreamDestroy(x->stream);
    (void)hipGetLastError();
    delete x;
}

size_t tm_yuv_mem_usage(const tm_yuv *x) { return x ? x->bytes : 0; }

int tm_yuv_set_frame(tm_yuv *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y,
                     size_t pitch_uv, int mem)
{
    if (!x || slot >= x->cap || (side != TM_SIDE_REF && side != TM_SIDE_DIS) || !y || !u) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE && mem != TM_MEM_HOST_PINNED) return TM_ERR_INVALID_ARG;
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
    if (x->pending && mem != TM_MEM_DEVICE) {
        const int rc = tm_yuv_sync(x); // the staging surface may still be read; a device surface is only noted in a host-side descriptor
        if (rc) return rc;
    }
    if (hipSetDevice(x->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const unsigned ph = g.h, ch = g.ph[1];
    const size_t idx = (size_t)slot * 2 + side;
    TmYuvDesc d{};
    if (mem == TM_MEM_DEVICE) {
        d.p0 = y; d.p1 = u; d.p2 = v; d.pitch = pitch_y; d.pitch2 = pitch_uv;
    } else {
        const size_t sp_y = (row_y + 255) / 256 * 256, sp_c = (row_c + 255) / 256 * 256;
        const size_t need = sp_y * ph + nc * sp_c * ch;
        if (!x->staging[idx]) {
            const int rc = dev_alloc(x, &x->staging[idx], need);
            if (rc) return rc;
        }
        char *s = (char *)x->staging[idx];
        const hipMemcpyKind k = hipMemcpyHostToDevice;
        YCHK(hipMemcpy2DAsync(s, sp_y, y, pitch_y, row_y, ph, k, x->stream));
        YCHK(hipMemcpy2DAsync(s + sp_y * ph, sp_c, u, pitch_uv, row_c, ch, k, x->stream));
        if (!biplanar) YCHK(hipMemcpy2DAsync(s + sp_y * ph + sp_c * ch, sp_c, v, pitch_uv, row_c, ch, k, x->stream));
        if (mem == TM_MEM_HOST) YCHK(hipStreamSynchronize(x->stream));
        d.p0 = s; d.p1 = s + sp_y * ph; d.p2 = biplanar ? nullptr : s + sp_y * ph + sp_c * ch; d.pitch = sp_y; d.pitch2 = sp_c;
    }
    d.vec = (((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2) & 15) == 0;
    x->desc[idx] = d;
    x->have[idx] = 1;
    return TM_OK;
}

int tm_yuv_compute_async(tm_yuv *x, uint32_t n_slots)
{
    if (!x || n_slots == 0 || n_slots > x->cap) return TM_ERR_INVALID_ARG;
    if (x->pending) return TM_ERR_STATE;
    for (uint32_t i = 0; i < 2 * n_slots; ++i)
        if (!x->have[i]) return TM_ERR_STATE;
    if (hipSetDevice(x->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    memcpy(x->h_desc, x->desc.data(), 2 * n_slots * sizeof(TmYuvDesc));
    // after the first queued operation a failure must not leave work behind that still reads the descriptors and the staging surfaces
    // while the caller believes nothing is pending: wait for what was queued, then report
#define YQUEUED(call)                                   \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            (void)hipStreamSynchronize(x->stream);      \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)
    YCHK(hipMemcpyAsync(x->d_desc, x->h_desc, 2 * n_slots * sizeof(TmYuvDesc), hipMemcpyHostToDevice, x->stream));
    const TmYuvGeom g = x->g;
    const dim3 grid(g.grid, n_slots), block(TMY_THREADS);
#define TMY_LAUNCH(L, F) k_yuv<L, F><<<grid, block, 0, x->stream>>>(g, x->d_desc, x->d_maps, x->d_cells)
    TMY_DISPATCH(g, TMY_LAUNCH);
#undef TMY_LAUNCH
    YQUEUED(hipGetLastError());
    k_yuv_finish<<<dim3(n_slots), block, 0, x->stream>>>(g, x->d_cells, x->d_res);
    YQUEUED(hipGetLastError());
    YQUEUED(hipMemcpyAsync(x->h_res, x->d_res, n_slots * sizeof(TmYuvRes), hipMemcpyDeviceToHost, x->stream));
#undef YQUEUED
    x->pending = true;
    // every batch hands its pictures over anew: a slot not set again before the next compute is TM_ERR_STATE, not a stale picture
    std::fill(x->have.begin(), x->have.begin() + 2 * n_slots, 0);
    x->n_last = n_slots;
    return TM_OK;
}

int tm_yuv_sync(tm_yuv *x)
{
    if (!x) return TM_ERR_INVALID_ARG;
    if (!x->pending) return TM_OK;
    if (hipSetDevice(x->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    YCHK(hipStreamSynchronize(x->stream));
    x->pending = false;
    return TM_OK;
}

int tm_yuv_get(tm_yuv *x, uint32_t first_slot, uint32_t n, tm_yuv_frame *out)
{
    if (!x || !out) return TM_ERR_INVALID_ARG;
    if (x->n_last == 0 || first_slot + (uint64_t)n > x->n_last) return TM_ERR_STATE;
    const int rc = tm_yuv_sync(x);
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
    if (slot >= x->n_last) return TM_ERR_STATE;
    const int rc = tm_yuv_sync(x);
    if (rc) return rc;
    if (hipSetDevice(x->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const float *src = x->d_maps + (size_t)slot * g.map_floats + g.map_off[plane];
    YCHK(hipMemcpy2D(dst, pitch, src, mw * sizeof(float), mw * sizeof(float), mh, hipMemcpyDeviceToHost));
    return TM_OK;
}

} // extern "C"
