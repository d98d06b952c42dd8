// tm_scene.hip -- host side of libturbometrics_scene.so (include/turbo_metrics_scene.h): frame upload, two launches per batch, and the
// host functions of the definition.  Kernels: tm_scene_kernels.h; definition: DESIGN.md section 12.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_scene.h"
#include "tm_scene_kernels.h"

namespace {

static_assert(TMS_Y8 == TM_SCENE_Y8 && TMS_Y16_MSB == TM_SCENE_Y16_MSB && TMS_Y16_LOW == TM_SCENE_Y16_LOW && TMS_Y10_PACKED == TM_SCENE_Y10_PACKED, "layouts");
static_assert(sizeof(tm_scene_frame) == TMS_BINS * sizeof(unsigned), "one result is the 256 counters");

#define SCHK(call)                                      \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

} // namespace

struct tm_scene {
    TmSceneGeom g;
    uint32_t cap;
    int device;
    hipStream_t stream = nullptr;
    TmSceneDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmSceneDesc> desc;                    // what set_frame wrote
    std::vector<unsigned char> have;                  // [slot]: set since the last compute
    std::vector<void *> staging;                      // [slot]: device copy of a host picture (lazily allocated)
    unsigned *d_cells = nullptr;                      // [slot][band][256]: every cell is written by every compute
    unsigned *d_hist = nullptr, *h_hist = nullptr;    // [slot][256]
    size_t bytes = 0;
    bool pending = false;
    uint32_t n_last = 0;
};

namespace {

int dev_alloc(tm_scene *s, void **p, size_t n)
{
    const hipError_t r = hipMalloc(p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    SCHK(r);
    s->bytes += n;
    return TM_OK;
}

// bytes of one luma row
size_t row_bytes(const tm_scene *s)
{
    switch (s->g.fmt) {
    case TMX_F_U8: return (size_t)s->g.w;
    case TMX_F_P10: return (size_t)tm_p10_row_words(s->g.w) * 4;
    default: return (size_t)s->g.w * 2;
    }
}

} // namespace

extern "C" {

int tm_scene_distance(const uint32_t a[256], const uint32_t b[256], int bins, uint64_t *out)
{
    if (!a || !b || !out) return TM_ERR_INVALID_ARG;
    if (bins != 8 && bins != 16 && bins != 32 && bins != 64 && bins != 128 && bins != 256) return TM_ERR_INVALID_ARG;
    const int run = 256 / bins;
    uint64_t d = 0;
    for (int k = 0; k < bins; ++k) {
        uint64_t sa = 0, sb = 0;
        for (int j = 0; j < run; ++j) { sa += a[k * run + j]; sb += b[k * run + j]; }
        d += sa > sb ? sa - sb : sb - sa;
    }
    *out = d;
    return TM_OK;
}

double tm_scene_score(uint64_t distance, uint32_t w, uint32_t h) { return (double)distance / (2.0 * (double)w * (double)h); }

int tm_scene_is_cut(double score, double threshold) { return score >= threshold; }

int tm_scene_stats(const uint32_t hist[256], uint32_t *min_bin, uint32_t *max_bin, double *mean_bin)
{
    if (!hist) return TM_ERR_INVALID_ARG;
    uint64_t n = 0, sum = 0;
    uint32_t lo = 256, hi = 0;
    for (uint32_t b = 0; b < 256; ++b) {
        if (!hist[b]) continue;
        if (lo == 256) lo = b;
        hi = b;
        n += hist[b];
        sum += (uint64_t)b * hist[b];
    }
    if (n == 0) return TM_ERR_INVALID_ARG;
    if (min_bin) *min_bin = lo;
    if (max_bin) *max_bin = hi;
    if (mean_bin) *mean_bin = (double)sum / (double)n;
    return TM_OK;
}

int tm_scene_create(tm_scene **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmSceneGeom g;
    if (tms_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launch's grid y
    int rc;
    // ---- first device call
    tm_scene *s = new tm_scene();
    s->g = g; s->cap = batch_capacity;
    auto fail = [&](int e) { tm_scene_destroy(s); return e; };
    if (hipGetDevice(&s->device) != hipSuccess) { (void)hipGetLastError(); delete s; return TM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); s->stream = nullptr; return fail(TM_ERR_HIP); }
    const size_t B = batch_capacity, res = B * TMS_BINS * sizeof(unsigned);
    if ((rc = dev_alloc(s, (void **)&s->d_desc, B * sizeof(TmSceneDesc)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_cells, res * g.bands))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_hist, res))) return fail(rc);
    if (hipHostMalloc((void **)&s->h_desc, B * sizeof(TmSceneDesc), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); s->h_desc = nullptr; return fail(TM_ERR_OOM); }
    if (hipHostMalloc((void **)&s->h_hist, res, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); s->h_hist = nullptr; return fail(TM_ERR_OOM); }
    s->bytes += B * sizeof(TmSceneDesc) + res;
    s->desc.assign(B, TmSceneDesc{});
    s->have.assign(B, 0);
    s->staging.assign(B, nullptr);
    *out = s;
    return TM_OK;
}

void tm_scene_destroy(tm_scene *s)
{
    if (!s) return;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (void *p : s->staging) if (p) (void)hipFree(p);
    if (s->d_desc) (void)hipFree(s->d_desc);
    if (s->d_cells) (void)hipFree(s->d_cells);
    if (s->d_hist) (void)hipFree(s->d_hist);
    if (s->h_desc) (void)hipHostFree(s->h_desc);
    if (s->h_hist) (void)hipHostFree(s->h_hist);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    (void)hipGetLastError();
    delete s;
}

size_t tm_scene_mem_usage(const tm_scene *s) { return s ? s->bytes : 0; }

int tm_scene_set_frame(tm_scene *s, uint32_t slot, const void *y, size_t pitch_y, int mem)
{
    if (!s || slot >= s->cap || !y) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE && mem != TM_MEM_HOST_PINNED) return TM_ERR_INVALID_ARG;
    const size_t row = row_bytes(s);
    if (pitch_y < row) return TM_ERR_INVALID_ARG;
    const size_t align = s->g.fmt == TMX_F_P10 ? 4 : (s->g.fmt == TMX_F_U8 ? 1 : 2);
    if (((uintptr_t)y | pitch_y) & (align - 1)) return TM_ERR_INVALID_ARG;
    if (s->pending) {
        const int rc = tm_scene_sync(s); // the staging surfaces may still be read
        if (rc) return rc;
    }
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    TmSceneDesc d{};
    if (mem == TM_MEM_DEVICE) {
        d.p = y; d.pitch = pitch_y;
    } else {
        const size_t sp = (row + 255) / 256 * 256;
        if (!s->staging[slot]) {
            const int rc = dev_alloc(s, &s->staging[slot], sp * s->g.h);
            if (rc) return rc;
        }
        SCHK(hipMemcpy2DAsync(s->staging[slot], sp, y, pitch_y, row, s->g.h, hipMemcpyHostToDevice, s->stream));
        if (mem == TM_MEM_HOST) SCHK(hipStreamSynchronize(s->stream));
        d.p = s->staging[slot]; d.pitch = sp;
    }
    d.vec = (((uintptr_t)d.p | d.pitch) & 15) == 0;
    s->desc[slot] = d;
    s->have[slot] = 1;
    return TM_OK;
}

int tm_scene_compute_async(tm_scene *s, uint32_t n_slots)
{
    if (!s || n_slots == 0 || n_slots > s->cap) return TM_ERR_INVALID_ARG;
    if (s->pending) return TM_ERR_STATE;
    for (uint32_t i = 0; i < n_slots; ++i)
        if (!s->have[i]) return TM_ERR_STATE;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    memcpy(s->h_desc, s->desc.data(), n_slots * sizeof(TmSceneDesc));
    SCHK(hipMemcpyAsync(s->d_desc, s->h_desc, n_slots * sizeof(TmSceneDesc), hipMemcpyHostToDevice, s->stream));
    const TmSceneGeom g = s->g;
    const dim3 grid(g.bands, n_slots), block(TMS_THREADS);
    switch (g.fmt) {
    case TMX_F_U8: k_scene_hist<TMX_F_U8><<<grid, block, 0, s->stream>>>(g, s->d_desc, s->d_cells); break;
    case TMX_F_U16_MSB: k_scene_hist<TMX_F_U16_MSB><<<grid, block, 0, s->stream>>>(g, s->d_desc, s->d_cells); break;
    case TMX_F_U16_LOW: k_scene_hist<TMX_F_U16_LOW><<<grid, block, 0, s->stream>>>(g, s->d_desc, s->d_cells); break;
    default: k_scene_hist<TMX_F_P10><<<grid, block, 0, s->stream>>>(g, s->d_desc, s->d_cells); break;
    }
    SCHK(hipGetLastError());
    k_scene_finish<<<dim3(n_slots), block, 0, s->stream>>>(g.bands, s->d_cells, s->d_hist);
    SCHK(hipGetLastError());
    SCHK(hipMemcpyAsync(s->h_hist, s->d_hist, (size_t)n_slots * TMS_BINS * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    s->pending = true;
    // every batch hands its pictures over anew: a slot not set again before the next compute is TM_ERR_STATE, not a stale picture
    std::fill(s->have.begin(), s->have.begin() + n_slots, 0);
    s->n_last = n_slots;
    return TM_OK;
}

int tm_scene_sync(tm_scene *s)
{
    if (!s) return TM_ERR_INVALID_ARG;
    if (!s->pending) return TM_OK;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    SCHK(hipStreamSynchronize(s->stream));
    s->pending = false;
    return TM_OK;
}

int tm_scene_get(tm_scene *s, uint32_t first_slot, uint32_t n, tm_scene_frame *out)
{
    if (!s || !out) return TM_ERR_INVALID_ARG;
    if (s->n_last == 0 || first_slot + (uint64_t)n > s->n_last) return TM_ERR_STATE;
    const int rc = tm_scene_sync(s);
    if (rc) return rc;
    memcpy(out, s->h_hist + (size_t)first_slot * TMS_BINS, (size_t)n * sizeof(tm_scene_frame));
    return TM_OK;
}

} // extern "C"
