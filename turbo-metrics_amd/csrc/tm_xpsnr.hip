// tm_xpsnr.hip -- host side of libturbometrics_xpsnr.so (include/turbo_metrics_xpsnr.h): geometry of the definition
// (DESIGN.md section 8), frame upload, the two launches per batch and the double-buffered history.  Kernels: tm_xpsnr_kernels.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_xpsnr.h"
#include "tm_xpsnr_kernels.h"

namespace {

static_assert(TMX_NV12 == TM_XPSNR_NV12 && TMX_P016 == TM_XPSNR_P016 && TMX_I420 == TM_XPSNR_I420 && TMX_I420P10 == TM_XPSNR_I420P10_PACKED, "layouts");

#define XCHK(call)                                      \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

} // namespace

struct tm_xpsnr {
    TmXpsnrGeom g;
    int layout;
    uint32_t bits, cap;
    int device;
    hipStream_t stream = nullptr;
    TmXpsnrDesc *d_desc = nullptr, *h_desc = nullptr; // [slot][side]; h_desc is page-locked, copied at each compute
    std::vector<TmXpsnrDesc> desc;                    // what set_frame wrote
    std::vector<unsigned char> have;                  // [slot][side]: set since create
    std::vector<void *> staging;                      // [slot][side]: device copy of a host picture (lazily allocated)
    unsigned short *hist[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}; // [buffer][m1, m2]
    int parity = 0;                                   // the next launch reads hist[parity] and writes hist[parity ^ 1]
    unsigned long long *d_blk = nullptr, *d_res = nullptr, *h_res = nullptr;
    double *d_wgt = nullptr;
    size_t bytes = 0;
    bool pending = false;
    uint32_t n_last = 0;
};

namespace {

int dev_alloc(tm_xpsnr *x, void **p, size_t n)
{
    const hipError_t r = hipMalloc(p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    XCHK(r);
    x->bytes += n;
    return TM_OK;
}

// device bytes of one picture of this layout, staged with 256-byte row pitches
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
    int rc;
    // ---- first device call
    tm_xpsnr *x = new tm_xpsnr();
    x->g = g; x->layout = layout; x->bits = bits; x->cap = batch_capacity;
    auto fail = [&](int e) { tm_xpsnr_destroy(x); return e; };
    if (hipGetDevice(&x->device) != hipSuccess) { (void)hipGetLastError(); delete x; return TM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); x->stream = nullptr; return fail(TM_ERR_HIP); }
    const size_t B = batch_capacity, hist = (size_t)g.hpitch * g.h * sizeof(unsigned short);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j)
            if ((rc = dev_alloc(x, (void **)&x->hist[i][j], hist))) return fail(rc);
    if ((rc = dev_alloc(x, (void **)&x->d_desc, B * 2 * sizeof(TmXpsnrDesc)))) return fail(rc);
    if ((rc = dev_alloc(x, (void **)&x->d_blk, B * g.nblk * 5 * sizeof(unsigned long long)))) return fail(rc);
    if ((rc = dev_alloc(x, (void **)&x->d_wgt, B * g.nblk * sizeof(double)))) return fail(rc);
    if ((rc = dev_alloc(x, (void **)&x->d_res, B * 3 * sizeof(unsigned long long)))) return fail(rc);
    if (hipHostMalloc((void **)&x->h_desc, B * 2 * sizeof(TmXpsnrDesc), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); x->h_desc = nullptr; return fail(TM_ERR_OOM); }
    if (hipHostMalloc((void **)&x->h_res, B * 3 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); x->h_res = nullptr; return fail(TM_ERR_OOM); }
    x->bytes += B * 2 * sizeof(TmXpsnrDesc) + B * 3 * sizeof(unsigned long long);
    x->desc.assign(B * 2, TmXpsnrDesc{});
    x->have.assign(B * 2, 0);
    x->staging.assign(B * 2, nullptr);
    if ((rc = tm_xpsnr_reset(x))) return fail(rc);
    *out = x;
    return TM_OK;
}

void tm_xpsnr_destroy(tm_xpsnr *x)
{
    if (!x) return;
    if (x->stream) (void)hipStreamSynchronize(x->stream);
    for (void *p : x->staging) if (p) (void)hipFree(p);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) if (x->hist[i][j]) (void)hipFree(x->hist[i][j]);
    if (x->d_desc) (void)hipFree(x->d_desc);
    if (x->d_blk) (void)hipFree(x->d_blk);
    if (x->d_wgt) (void)hipFree(x->d_wgt);
    if (x->d_res) (void)hipFree(x->d_res);
    if (x->h_desc) (void)hipHostFree(x->h_desc);
    if (x->h_res) (void)hipHostFree(x->h_res);
    if (x->stream) (void)hipStreamDestroy(x->stream);
    (void)hipGetLastError();
    delete x;
}

size_t tm_xpsnr_mem_usage(const tm_xpsnr *x) { return x ? x->bytes : 0; }

int tm_xpsnr_set_frame(tm_xpsnr *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y,
                       size_t pitch_uv, int mem)
{
    if (!x || slot >= x->cap || (side != TM_SIDE_REF && side != TM_SIDE_DIS) || !y || !u) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE && mem != TM_MEM_HOST_PINNED) return TM_ERR_INVALID_ARG;
    const bool biplanar = x->layout == TM_XPSNR_NV12 || x->layout == TM_XPSNR_P016;
    if (biplanar) v = nullptr;
    else if (!v) return TM_ERR_INVALID_ARG;
    size_t row_y, row_c;
    int nc;
    plane_rows(x, &row_y, &row_c, &nc);
    if (pitch_y < row_y || pitch_uv < row_c) return TM_ERR_INVALID_ARG;
    const size_t align = x->layout == TM_XPSNR_I420P10_PACKED ? 4 : (x->bits == 8 ? 1 : 2);
    if (((uintptr_t)y | (uintptr_t)u | (uintptr_t)v | pitch_y | pitch_uv) & (align - 1)) return TM_ERR_INVALID_ARG;
    if (x->pending) {
        const int rc = tm_xpsnr_sync(x); // the staging surfaces may still be read
        if (rc) return rc;
    }
    if (hipSetDevice(x->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const TmXpsnrGeom &g = x->g;
    const size_t idx = (size_t)slot * 2 + side;
    TmXpsnrDesc d{};
    if (mem == TM_MEM_DEVICE) {
        d.p0 = y; d.p1 = u; d.p2 = v; d.pitch = pitch_y; d.pitch2 = pitch_uv;
    } else {
        const size_t sp_y = (row_y + 255) / 256 * 256, sp_c = (row_c + 255) / 256 * 256;
        const size_t need = sp_y * g.h + nc * sp_c * g.ch;
        if (!x->staging[idx]) {
            const int rc = dev_alloc(x, &x->staging[idx], need);
            if (rc) return rc;
        }
        char *s = (char *)x->staging[idx];
        const hipMemcpyKind k = hipMemcpyHostToDevice;
        XCHK(hipMemcpy2DAsync(s, sp_y, y, pitch_y, row_y, g.h, k, x->stream));
        XCHK(hipMemcpy2DAsync(s + sp_y * g.h, sp_c, u, pitch_uv, row_c, g.ch, k, x->stream));
        if (!biplanar) XCHK(hipMemcpy2DAsync(s + sp_y * g.h + sp_c * g.ch, sp_c, v, pitch_uv, row_c, g.ch, k, x->stream));
        if (mem == TM_MEM_HOST) XCHK(hipStreamSynchronize(x->stream));
        d.p0 = s; d.p1 = s + sp_y * g.h; d.p2 = biplanar ? nullptr : s + sp_y * g.h + sp_c * g.ch; d.pitch = sp_y; d.pitch2 = sp_c;
    }
    d.vec = (((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2) & 15) == 0;
    x->desc[idx] = d;
    x->have[idx] = 1;
    return TM_OK;
}

int tm_xpsnr_compute_async(tm_xpsnr *x, uint32_t n_slots)
{
    if (!x || n_slots == 0 || n_slots > x->cap) return TM_ERR_INVALID_ARG;
    if (x->pending) return TM_ERR_STATE;
    for (uint32_t i = 0; i < 2 * n_slots; ++i)
        if (!x->have[i]) return TM_ERR_STATE;
    if (hipSetDevice(x->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    memcpy(x->h_desc, x->desc.data(), 2 * n_slots * sizeof(TmXpsnrDesc));
    XCHK(hipMemcpyAsync(x->d_desc, x->h_desc, 2 * n_slots * sizeof(TmXpsnrDesc), hipMemcpyHostToDevice, x->stream));
    TmXpsnrGeom g = x->g;
    g.n = (int)n_slots;
    unsigned short *const *hin = x->hist[x->parity], *const *hout = x->hist[x->parity ^ 1];
    k_xpsnr_blocks<<<dim3((unsigned)g.nblk, n_slots), dim3(TMX_THREADS), 0, x->stream>>>(g, x->d_desc, hin[0], hin[1], hout[0], hout[1], x->d_blk);
    XCHK(hipGetLastError());
    k_xpsnr_finish<<<dim3((n_slots + 63) / 64), dim3(64), 0, x->stream>>>(g, x->d_blk, x->d_wgt, x->d_res);
    XCHK(hipGetLastError());
    XCHK(hipMemcpyAsync(x->h_res, x->d_res, n_slots * 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, x->stream));
    x->parity ^= 1;
    x->pending = true;
    // every batch hands its pictures over anew: a slot not set again before the next compute is TM_ERR_STATE, not a stale picture
    std::fill(x->have.begin(), x->have.begin() + 2 * n_slots, 0);
    x->n_last = n_slots;
    return TM_OK;
}

int tm_xpsnr_sync(tm_xpsnr *x)
{
    if (!x) return TM_ERR_INVALID_ARG;
    if (!x->pending) return TM_OK;
    if (hipSetDevice(x->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    XCHK(hipStreamSynchronize(x->stream));
    x->pending = false;
    return TM_OK;
}

int tm_xpsnr_get(tm_xpsnr *x, uint32_t first_slot, uint32_t n, tm_xpsnr_frame *out)
{
    if (!x || !out) return TM_ERR_INVALID_ARG;
    if (x->n_last == 0 || first_slot + (uint64_t)n > x->n_last) return TM_ERR_STATE;
    int rc = tm_xpsnr_sync(x);
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
    int rc = tm_xpsnr_sync(x);
    if (rc) return rc;
    if (hipSetDevice(x->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const size_t hist = (size_t)x->g.hpitch * x->g.h * sizeof(unsigned short);
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) XCHK(hipMemsetAsync(x->hist[i][j], 0, hist, x->stream));
    XCHK(hipStreamSynchronize(x->stream));
    x->parity = 0;
    std::fill(x->have.begin(), x->have.end(), 0);
    return TM_OK;
}

} // extern "C"
