// tm_hvs.hip -- host side of libturbometrics_hvs.so (include/turbo_metrics_hvs.h): pair upload, the two launches per batch and the
// host functions.  Kernels: tm_hvs_kernels.h; definition: DESIGN.md section 16.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_hvs.h"
#include "tm_hvs_kernels.h"

namespace {

static_assert(TMH_Y8 == TM_HVS_Y8 && TMH_Y16_MSB == TM_HVS_Y16_MSB && TMH_Y16_LOW == TM_HVS_Y16_LOW && TMH_Y10_PACKED == TM_HVS_Y10_PACKED, "layouts");

#define HCHK(call)                                      \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

// the host's copies of the kernel's tables
const float kHostCsf[64] = TMH_CSF_VALUES;
const float kHostMask[64] = TMH_MASK_VALUES;

} // namespace

struct tm_hvs {
    TmHvsGeom g;
    uint32_t cap;
    int device;
    hipStream_t stream = nullptr;
    TmHvsDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmHvsDesc> desc;                    // what set_pair wrote
    std::vector<unsigned char> have;                // [slot]: set since the last compute
    std::vector<void *> staging;                    // [slot][2]: device copy of a host picture (lazily allocated)
    TmHvsCell *d_cells = nullptr;                   // [slot][g.cells]: every cell is written by every compute
    TmHvsCell *d_res = nullptr, *h_res = nullptr;   // [slot]
    size_t bytes = 0;
    bool pending = false;
    uint32_t n_last = 0;
};

namespace {

int dev_alloc(tm_hvs *v, void **p, size_t n)
{
    const hipError_t r = hipMalloc(p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    HCHK(r);
    v->bytes += n;
    return TM_OK;
}

// bytes of one luma row
size_t row_bytes(const tm_hvs *v)
{
    switch (v->g.fmt) {
    case TMX_F_U8: return (size_t)v->g.w;
    case TMX_F_P10: return (size_t)tm_p10_row_words(v->g.w) * 4;
    default: return (size_t)v->g.w * 2;
    }
}

} // namespace

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
    v->g = g; v->cap = batch_capacity;
    auto fail = [&](int e) { tm_hvs_destroy(v); return e; };
    // ---- first device call
    if (hipGetDevice(&v->device) != hipSuccess) { (void)hipGetLastError(); delete v; return TM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); v->stream = nullptr; return fail(TM_ERR_HIP); }
    const size_t B = batch_capacity;
    int rc;
    if ((rc = dev_alloc(v, (void **)&v->d_cells, B * (size_t)g.cells * sizeof(TmHvsCell)))) return fail(rc);
    if ((rc = dev_alloc(v, (void **)&v->d_desc, B * sizeof(TmHvsDesc)))) return fail(rc);
    if ((rc = dev_alloc(v, (void **)&v->d_res, B * sizeof(TmHvsCell)))) return fail(rc);
    if (hipHostMalloc((void **)&v->h_desc, B * sizeof(TmHvsDesc), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); v->h_desc = nullptr; return fail(TM_ERR_OOM); }
    if (hipHostMalloc((void **)&v->h_res, B * sizeof(TmHvsCell), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); v->h_res = nullptr; return fail(TM_ERR_OOM); }
    v->bytes += B * sizeof(TmHvsDesc) + B * sizeof(TmHvsCell);
    v->desc.assign(B, TmHvsDesc{});
    v->have.assign(B, 0);
    v->staging.assign(2 * B, nullptr);
    *out = v;
    return TM_OK;
}

void tm_hvs_destroy(tm_hvs *v)
{
    if (!v) return;
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    for (void *p : v->staging) if (p) (void)hipFree(p);
    if (v->d_cells) (void)hipFree(v->d_cells);
    if (v->d_desc) (void)hipFree(v->d_desc);
    if (v->d_res) (void)hipFree(v->d_res);
    if (v->h_desc) (void)hipHostFree(v->h_desc);
    if (v->h_res) (void)hipHostFree(v->h_res);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    (void)hipGetLastError();
    delete v;
}

size_t tm_hvs_mem_usage(const tm_hvs *v) { return v ? v->bytes : 0; }

int tm_hvs_set_pair(tm_hvs *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem)
{
    if (!v || slot >= v->cap || !ref_y || !dis_y) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE && mem != TM_MEM_HOST_PINNED) return TM_ERR_INVALID_ARG;
    const size_t row = row_bytes(v);
    if (pitch_ref < row || pitch_dis < row) return TM_ERR_INVALID_ARG;
    const size_t align = v->g.fmt == TMX_F_P10 ? 4 : (v->g.fmt == TMX_F_U8 ? 1 : 2);
    if (((uintptr_t)ref_y | (uintptr_t)dis_y | pitch_ref | pitch_dis) & (align - 1)) return TM_ERR_INVALID_ARG;
    if (v->pending) {
        const int rc = tm_hvs_sync(v); // the staging surfaces may still be read
        if (rc) return rc;
    }
    if (hipSetDevice(v->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const void *src[2] = {ref_y, dis_y};
    const size_t pitch[2] = {pitch_ref, pitch_dis};
    TmHvsDesc d{};
    d.vec = 1;
    for (int p = 0; p < 2; ++p) {
        if (mem == TM_MEM_DEVICE) {
            d.p[p] = src[p]; d.pitch[p] = pitch[p];
        } else {
            const size_t sp = (row + 255) / 256 * 256;
            void *&st = v->staging[2 * slot + p];
            if (!st) {
                const int rc = dev_alloc(v, &st, sp * v->g.h);
                if (rc) return rc;
            }
            HCHK(hipMemcpy2DAsync(st, sp, src[p], pitch[p], row, v->g.h, hipMemcpyHostToDevice, v->stream));
            d.p[p] = st; d.pitch[p] = sp;
        }
        if (((uintptr_t)d.p[p] | d.pitch[p]) & 15) d.vec = 0;
    }
    if (mem == TM_MEM_HOST) HCHK(hipStreamSynchronize(v->stream));
    v->desc[slot] = d;
    v->have[slot] = 1;
    return TM_OK;
}

int tm_hvs_compute_async(tm_hvs *v, uint32_t n_slots)
{
    if (!v || n_slots == 0 || n_slots > v->cap) return TM_ERR_INVALID_ARG;
    if (v->pending) return TM_ERR_STATE;
    for (uint32_t i = 0; i < n_slots; ++i)
        if (!v->have[i]) return TM_ERR_STATE;
    if (hipSetDevice(v->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    memcpy(v->h_desc, v->desc.data(), n_slots * sizeof(TmHvsDesc));
    // after the first queued operation a failure must not leave work behind that still reads the descriptors and the staging surfaces
    // while the caller believes nothing is pending: wait for what was queued, then report
#define HQUEUED(call)                                   \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            (void)hipStreamSynchronize(v->stream);      \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)
    HCHK(hipMemcpyAsync(v->d_desc, v->h_desc, n_slots * sizeof(TmHvsDesc), hipMemcpyHostToDevice, v->stream));
    const TmHvsGeom g = v->g;
    const dim3 grid(g.cells, n_slots), block(TMH_THREADS);
#define TMH_LAUNCH(F) k_hvs<F><<<grid, block, 0, v->stream>>>(g, v->d_desc, v->d_cells)
    TMH_DISPATCH(g, TMH_LAUNCH);
#undef TMH_LAUNCH
    HQUEUED(hipGetLastError());
    k_hvs_finish<<<dim3(n_slots), block, 0, v->stream>>>(g, v->d_cells, v->d_res);
    HQUEUED(hipGetLastError());
    HQUEUED(hipMemcpyAsync(v->h_res, v->d_res, n_slots * sizeof(TmHvsCell), hipMemcpyDeviceToHost, v->stream));
#undef HQUEUED
    v->pending = true;
    // every batch hands its pairs over anew: a slot not set again before the next compute is TM_ERR_STATE, not a stale pair
    std::fill(v->have.begin(), v->have.begin() + n_slots, 0);
    v->n_last = n_slots;
    return TM_OK;
}

int tm_hvs_sync(tm_hvs *v)
{
    if (!v) return TM_ERR_INVALID_ARG;
    if (!v->pending) return TM_OK;
    if (hipSetDevice(v->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    HCHK(hipStreamSynchronize(v->stream));
    v->pending = false;
    return TM_OK;
}

int tm_hvs_get(tm_hvs *v, uint32_t first_slot, uint32_t n, tm_hvs_frame *out)
{
    if (!v || !out) return TM_ERR_INVALID_ARG;
    if (v->n_last == 0 || first_slot + (uint64_t)n > v->n_last) return TM_ERR_STATE;
    const int rc = tm_hvs_sync(v);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        out[i].s_hvs = v->h_res[first_slot + i].s_hvs;
        out[i].s_hvsm = v->h_res[first_slot + i].s_hvsm;
        out[i].blocks = (uint64_t)v->g.bw * v->g.bh;
    }
    return TM_OK;
}

} // extern "C"
