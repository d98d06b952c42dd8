// tm_adm.hip -- host side of libturbometrics_adm.so (include/turbo_metrics_adm.h): pair upload, one launch per scale and the
// finish, and the host function of the definition (tm_adm_scores).  Kernels: tm_adm_kernels.h; definition: DESIGN.md section 11.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_adm.h"
#include "tm_adm_kernels.h"

namespace {

static_assert(TMA_Y8 == TM_ADM_Y8 && TMA_Y16_MSB == TM_ADM_Y16_MSB && TMA_Y16_LOW == TM_ADM_Y16_LOW && TMA_Y10_PACKED == TM_ADM_Y10_PACKED, "layouts");

#define VCHK(call)                                      \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

} // namespace

struct tm_adm {
    TmAdmGeom g;
    uint32_t cap;
    int device;
    hipStream_t stream = nullptr;
    TmAdmDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmAdmDesc> desc;                    // what set_pair wrote
    std::vector<unsigned char> have;                // [slot]: set since the last compute
    std::vector<void *> staging;                    // [slot][2]: device copy of a host picture (lazily allocated)
    float *planes = nullptr;                        // [slot]: the a bands of scales 0 .. 2 = the pictures of scales 1 .. 3
    double *d_cell = nullptr;                       // [slot][cells][6]: N[h, v, d], Dn[h, v, d] per workgroup
    double *d_res = nullptr, *h_res = nullptr;      // [slot][scale][6]
    size_t bytes = 0;
    bool pending = false;
    uint32_t n_last = 0;
};

namespace {

int dev_alloc(tm_adm *v, void **p, size_t n)
{
    const hipError_t r = hipMalloc(p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    VCHK(r);
    v->bytes += n;
    return TM_OK;
}

// bytes of one luma row
size_t row_bytes(const tm_adm *v)
{
    switch (v->g.fmt) {
    case TMX_F_U8: return (size_t)v->g.w[0];
    case TMX_F_P10: return (size_t)tm_p10_row_words(v->g.w[0]) * 4;
    default: return (size_t)v->g.w[0] * 2;
    }
}

template <int FMT>
void launch_scale0(const tm_adm *v, uint32_t n)
{
    k_adm<FMT, 0><<<dim3((unsigned)v->g.tiles[0], n), dim3(TMA_THREADS), 0, v->stream>>>(v->g, v->d_desc, v->planes, v->d_cell);
}

} // namespace

extern "C" {

void tm_adm_scores(const tm_adm_frame *f, uint32_t w, uint32_t h, double out[5])
{
    TmAdmGeom g;
    tma_sizes(w, h, &g);
    auto score = [](double n, double d) {
        if (n < 1e-10) n = 0.0;
        if (d < 1e-10) d = 0.0;
        return d == 0.0 ? 1.0 : n / d;
    };
    double num = 0.0, den = 0.0;
    for (int s = 0; s < 4; ++s) {
        const double area = (double)(g.bottom[s] - g.top[s]) * (double)(g.right[s] - g.left[s]);
        const double c = cbrt(area / 32.0);
        double ns = 0.0, ds = 0.0;
        for (int b = 0; b < 3; ++b) {
            ns += cbrt(f->num_cube[s][b]) + c;
            ds += cbrt(f->den_cube[s][b]) + c;
        }
        out[s] = score(ns, ds);
        num += ns;
        den += ds;
    }
    out[4] = score(num, den);
}

int tm_adm_create(tm_adm **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmAdmGeom g;
    if (tma_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    int rc;
    // ---- first device call
    tm_adm *v = new tm_adm();
    v->g = g; v->cap = batch_capacity;
    auto fail = [&](int e) { tm_adm_destroy(v); return e; };
    if (hipGetDevice(&v->device) != hipSuccess) { (void)hipGetLastError(); delete v; return TM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); v->stream = nullptr; return fail(TM_ERR_HIP); }
    const size_t B = batch_capacity, res = B * TMA_SCALES * 6 * sizeof(double);
    if ((rc = dev_alloc(v, (void **)&v->planes, B * g.pslot * sizeof(float)))) return fail(rc);
    if ((rc = dev_alloc(v, (void **)&v->d_cell, B * (size_t)g.cells * 6 * sizeof(double)))) return fail(rc);
    if ((rc = dev_alloc(v, (void **)&v->d_desc, B * sizeof(TmAdmDesc)))) return fail(rc);
    if ((rc = dev_alloc(v, (void **)&v->d_res, res))) return fail(rc);
    if (hipHostMalloc((void **)&v->h_desc, B * sizeof(TmAdmDesc), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); v->h_desc = nullptr; return fail(TM_ERR_OOM); }
    if (hipHostMalloc((void **)&v->h_res, res, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); v->h_res = nullptr; return fail(TM_ERR_OOM); }
    v->bytes += B * sizeof(TmAdmDesc) + res;
    v->desc.assign(B, TmAdmDesc{});
    v->have.assign(B, 0);
    v->staging.assign(2 * B, nullptr);
    *out = v;
    return TM_OK;
}

void tm_adm_destroy(tm_adm *v)
{
    if (!v) return;
    if (v->stream) (void)hipStreamSynchronize(v->stream);
    for (void *p : v->staging) if (p) (void)hipFree(p);
    if (v->planes) (void)hipFree(v->planes);
    if (v->d_cell) (void)hipFree(v->d_cell);
    if (v->d_desc) (void)hipFree(v->d_desc);
    if (v->d_res) (void)hipFree(v->d_res);
    if (v->h_desc) (void)hipHostFree(v->h_desc);
    if (v->h_res) (void)hipHostFree(v->h_res);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    (void)hipGetLastError();
    delete v;
}

size_t tm_adm_mem_usage(const tm_adm *v) { return v ? v->bytes : 0; }

int tm_adm_set_pair(tm_adm *v, uint32_t slot, const void *ref_y, const void *dis_y, size_t pitch_ref, size_t pitch_dis, int mem)
{
    if (!v || slot >= v->cap || !ref_y || !dis_y) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE && mem != TM_MEM_HOST_PINNED) return TM_ERR_INVALID_ARG;
    const size_t row = row_bytes(v);
    if (pitch_ref < row || pitch_dis < row) return TM_ERR_INVALID_ARG;
    const size_t align = v->g.fmt == TMX_F_P10 ? 4 : (v->g.fmt == TMX_F_U8 ? 1 : 2);
    if (((uintptr_t)ref_y | (uintptr_t)dis_y | pitch_ref | pitch_dis) & (align - 1)) return TM_ERR_INVALID_ARG;
    if (v->pending) {
        const int rc = tm_adm_sync(v); // the staging surfaces may still be read
        if (rc) return rc;
    }
    if (hipSetDevice(v->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const void *src[2] = {ref_y, dis_y};
    const size_t pitch[2] = {pitch_ref, pitch_dis};
    TmAdmDesc d{};
    for (int p = 0; p < 2; ++p) {
        if (mem == TM_MEM_DEVICE) {
            d.p[p] = src[p]; d.pitch[p] = pitch[p];
        } else {
            const size_t sp = (row + 255) / 256 * 256;
            void *&st = v->staging[2 * slot + p];
            if (!st) {
                const int rc = dev_alloc(v, &st, sp * v->g.h[0]);
                if (rc) return rc;
            }
            VCHK(hipMemcpy2DAsync(st, sp, src[p], pitch[p], row, v->g.h[0], hipMemcpyHostToDevice, v->stream));
            d.p[p] = st; d.pitch[p] = sp;
        }
        d.vec[p] = (((uintptr_t)d.p[p] | d.pitch[p]) & 15) == 0;
    }
    if (mem == TM_MEM_HOST) VCHK(hipStreamSynchronize(v->stream));
    v->desc[slot] = d;
    v->have[slot] = 1;
    return TM_OK;
}

int tm_adm_compute_async(tm_adm *v, uint32_t n_slots)
{
    if (!v || n_slots == 0 || n_slots > v->cap) return TM_ERR_INVALID_ARG;
    if (v->pending) return TM_ERR_STATE;
    for (uint32_t i = 0; i < n_slots; ++i)
        if (!v->have[i]) return TM_ERR_STATE;
    if (hipSetDevice(v->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    memcpy(v->h_desc, v->desc.data(), n_slots * sizeof(TmAdmDesc));
    VCHK(hipMemcpyAsync(v->d_desc, v->h_desc, n_slots * sizeof(TmAdmDesc), hipMemcpyHostToDevice, v->stream));
    const TmAdmGeom &g = v->g;
    const dim3 block(TMA_THREADS);
    switch (g.fmt) {
    case TMX_F_U8: launch_scale0<TMX_F_U8>(v, n_slots); break;
    case TMX_F_U16_MSB: launch_scale0<TMX_F_U16_MSB>(v, n_slots); break;
    case TMX_F_U16_LOW: launch_scale0<TMX_F_U16_LOW>(v, n_slots); break;
    default: launch_scale0<TMX_F_P10>(v, n_slots); break;
    }
    VCHK(hipGetLastError());
    k_adm<TMX_F_HIST, 1><<<dim3((unsigned)g.tiles[1], n_slots), block, 0, v->stream>>>(g, v->d_desc, v->planes, v->d_cell);
    VCHK(hipGetLastError());
    k_adm<TMX_F_HIST, 2><<<dim3((unsigned)g.tiles[2], n_slots), block, 0, v->stream>>>(g, v->d_desc, v->planes, v->d_cell);
    VCHK(hipGetLastError());
    k_adm<TMX_F_HIST, 3><<<dim3((unsigned)g.tiles[3], n_slots), block, 0, v->stream>>>(g, v->d_desc, v->planes, v->d_cell);
    VCHK(hipGetLastError());
    k_adm_finish<<<dim3(TMA_SCALES, n_slots), block, 0, v->stream>>>(g, v->d_cell, v->d_res);
    VCHK(hipGetLastError());
    VCHK(hipMemcpyAsync(v->h_res, v->d_res, (size_t)n_slots * TMA_SCALES * 6 * sizeof(double), hipMemcpyDeviceToHost, v->stream));
    v->pending = true;
    // every batch hands its pairs over anew: a slot not set again before the next compute is TM_ERR_STATE, not a stale pair
    std::fill(v->have.begin(), v->have.begin() + n_slots, 0);
    v->n_last = n_slots;
    return TM_OK;
}

int tm_adm_sync(tm_adm *v)
{
    if (!v) return TM_ERR_INVALID_ARG;
    if (!v->pending) return TM_OK;
    if (hipSetDevice(v->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    VCHK(hipStreamSynchronize(v->stream));
    v->pending = false;
    return TM_OK;
}

int tm_adm_get(tm_adm *v, uint32_t first_slot, uint32_t n, tm_adm_frame *out)
{
    if (!v || !out) return TM_ERR_INVALID_ARG;
    if (v->n_last == 0 || first_slot + (uint64_t)n > v->n_last) return TM_ERR_STATE;
    const int rc = tm_adm_sync(v);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const double *r = v->h_res + (size_t)(first_slot + i) * TMA_SCALES * 6;
        for (int s = 0; s < TMA_SCALES; ++s)
            for (int b = 0; b < 3; ++b) {
                out[i].num_cube[s][b] = r[6 * s + b];
                out[i].den_cube[s][b] = r[6 * s + 3 + b];
            }
    }
    return TM_OK;
}

} // extern "C"
