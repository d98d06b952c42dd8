// tm_flip.hip -- host side of libturbometrics_flip.so (include/turbo_metrics_flip.h): pair upload, the two launches of a batch, the map
// read-back and the host function of the definition.  Kernels: tm_flip_kernels.h; definition: DESIGN.md section 14.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_flip.h"
#include "tm_flip_kernels.h"

namespace {

static_assert(TMF_RGB8 == TM_FLIP_RGB8 && TMF_MAP == TM_FLIP_MAP && TMF_MAP_COLOR == TM_FLIP_MAP_COLOR && TMF_MAP_FEATURE == TM_FLIP_MAP_FEATURE, "layouts and kinds");
static_assert(sizeof(tm_flip_frame) == sizeof(TmFlipRes) && TMF_HALO == TM_FLIP_MAX_RADIUS, "one result is the device's cell");

#define FCHK(call)                                      \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

} // namespace

struct tm_flip {
    TmFlipGeom g;
    uint32_t cap;
    int device;
    hipStream_t stream = nullptr;
    TmFlipTables *d_tabs = nullptr;
    TmFlipDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmFlipDesc> desc;                    // what set_pair wrote
    std::vector<unsigned char> have;                 // [slot]: set since the last compute
    std::vector<void *> staging;                     // [slot][side]: device copy of a host picture (lazily allocated)
    float *d_maps = nullptr;                         // [slot][kind][h][w]
    TmFlipCell *d_cells = nullptr;                   // [slot][tile]
    TmFlipRes *d_res = nullptr, *h_res = nullptr;    // [slot]
    size_t bytes = 0;
    bool pending = false;
    uint32_t n_last = 0;
};

namespace {

int dev_alloc(tm_flip *s, void **p, size_t n)
{
    const hipError_t r = hipMalloc(p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    FCHK(r);
    s->bytes += n;
    return TM_OK;
}

} // namespace

extern "C" {

int tm_flip_radius(double ppd, uint32_t *r_spatial, uint32_t *r_feature)
{
    if (!r_spatial || !r_feature) return TM_ERR_INVALID_ARG;
    if (ppd == 0.0) ppd = TM_FLIP_DEFAULT_PPD;
    if (!(ppd > 0.0) || !(ppd <= 1e6)) return TM_ERR_INVALID_ARG; // (beyond 1e6 the radii leave 32 bits)
    unsigned rs, rf;
    tmf_radius(ppd, &rs, &rf);
    *r_spatial = rs; *r_feature = rf;
    return TM_OK;
}

int tm_flip_create(tm_flip **out, uint32_t w, uint32_t h, int layout, double ppd, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0 || batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launches' grid y
    if (ppd == 0.0) ppd = TM_FLIP_DEFAULT_PPD;
    TmFlipGeom g;
    TmFlipTables tabs;
    if (tmf_make_geom(&g, &tabs, w, h, layout, ppd)) return TM_ERR_UNSUPPORTED;
    int rc;
    // ---- first device call
    tm_flip *s = new tm_flip();
    s->g = g; s->cap = batch_capacity;
    auto fail = [&](int e) { tm_flip_destroy(s); return e; };
    if (hipGetDevice(&s->device) != hipSuccess) { (void)hipGetLastError(); delete s; return TM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); s->stream = nullptr; return fail(TM_ERR_HIP); }
    const size_t B = batch_capacity, px = (size_t)w * h, tiles = (size_t)g.tiles_x * g.tiles_y, res = B * sizeof(TmFlipRes);
    if ((rc = dev_alloc(s, (void **)&s->d_tabs, sizeof(TmFlipTables)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_desc, B * sizeof(TmFlipDesc)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_maps, B * TMF_MAPS * px * sizeof(float)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_cells, B * tiles * sizeof(TmFlipCell)))) return fail(rc);
    if ((rc = dev_alloc(s, (void **)&s->d_res, res))) return fail(rc);
    if (hipHostMalloc((void **)&s->h_desc, B * sizeof(TmFlipDesc), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); s->h_desc = nullptr; return fail(TM_ERR_OOM); }
    if (hipHostMalloc((void **)&s->h_res, res, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); s->h_res = nullptr; return fail(TM_ERR_OOM); }
    s->bytes += B * sizeof(TmFlipDesc) + res;
    if (hipMemcpy(s->d_tabs, &tabs, sizeof tabs, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return fail(TM_ERR_HIP); }
    s->desc.assign(B, TmFlipDesc{});
    s->have.assign(B, 0);
    s->staging.assign(2 * B, nullptr);
    *out = s;
    return TM_OK;
}

void tm_flip_destroy(tm_flip *s)
{
    if (!s) return;
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (void *p : s->staging) if (p) (void)hipFree(p);
    if (s->d_tabs) (void)hipFree(s->d_tabs);
    if (s->d_desc) (void)hipFree(s->d_desc);
    if (s->d_maps) (void)hipFree(s->d_maps);
    if (s->d_cells) (void)hipFree(s->d_cells);
    if (s->d_res) (void)hipFree(s->d_res);
    if (s->h_desc) (void)hipHostFree(s->h_desc);
    if (s->h_res) (void)hipHostFree(s->h_res);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    (void)hipGetLastError();
    delete s;
}

size_t tm_flip_mem_usage(const tm_flip *s) { return s ? s->bytes : 0; }

int tm_flip_set_pair(tm_flip *s, uint32_t slot, const void *ref, size_t ref_pitch, const void *dis, size_t dis_pitch, int mem)
{
    if (!s || slot >= s->cap || !ref || !dis) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE) return TM_ERR_INVALID_ARG;
    const size_t row = (size_t)s->g.w * 3, rows = s->g.h;
    if (ref_pitch < row || dis_pitch < row) return TM_ERR_INVALID_ARG;
    if (s->pending) {
        const int rc = tm_flip_sync(s); // the staging surfaces may still be read
        if (rc) return rc;
    }
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const void *src[2] = {ref, dis};
    const size_t pitch[2] = {ref_pitch, dis_pitch};
    TmFlipDesc d{};
    for (int side = 0; side < 2; ++side) {
        if (mem == TM_MEM_DEVICE) {
            d.p[side] = (const unsigned char *)src[side]; d.pitch[side] = pitch[side];
            continue;
        }
        const size_t sp = (row + 255) / 256 * 256;
        void *&st = s->staging[2 * (size_t)slot + side];
        if (!st) {
            const int rc = dev_alloc(s, &st, sp * rows);
            if (rc) return rc;
        }
        FCHK(hipMemcpy2DAsync(st, sp, src[side], pitch[side], row, rows, hipMemcpyHostToDevice, s->stream));
        d.p[side] = (const unsigned char *)st; d.pitch[side] = sp;
    }
    if (mem == TM_MEM_HOST) FCHK(hipStreamSynchronize(s->stream));
    s->desc[slot] = d;
    s->have[slot] = 1;
    return TM_OK;
}

int tm_flip_compute_async(tm_flip *s, uint32_t n_slots)
{
    if (!s || n_slots == 0 || n_slots > s->cap) return TM_ERR_INVALID_ARG;
    if (s->pending) return TM_ERR_STATE;
    for (uint32_t i = 0; i < n_slots; ++i)
        if (!s->have[i]) return TM_ERR_STATE;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    memcpy(s->h_desc, s->desc.data(), n_slots * sizeof(TmFlipDesc));
    FCHK(hipMemcpyAsync(s->d_desc, s->h_desc, n_slots * sizeof(TmFlipDesc), hipMemcpyHostToDevice, s->stream));
    const TmFlipGeom g = s->g;
    k_flip_tile<<<dim3(g.tiles_x * g.tiles_y, n_slots), dim3(TMF_THREADS), 0, s->stream>>>(g, s->d_tabs, s->d_desc, s->d_maps, s->d_cells);
    FCHK(hipGetLastError());
    k_flip_finish<<<dim3(n_slots), dim3(TMF_THREADS), 0, s->stream>>>(g, s->d_cells, s->d_res);
    FCHK(hipGetLastError());
    FCHK(hipMemcpyAsync(s->h_res, s->d_res, (size_t)n_slots * sizeof(TmFlipRes), hipMemcpyDeviceToHost, s->stream));
    s->pending = true;
    // every batch hands its pairs over anew: a slot not set again before the next compute is TM_ERR_STATE, not a stale pair
    std::fill(s->have.begin(), s->have.begin() + n_slots, 0);
    s->n_last = n_slots;
    return TM_OK;
}

int tm_flip_sync(tm_flip *s)
{
    if (!s) return TM_ERR_INVALID_ARG;
    if (!s->pending) return TM_OK;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    FCHK(hipStreamSynchronize(s->stream));
    s->pending = false;
    return TM_OK;
}

int tm_flip_get(tm_flip *s, uint32_t first_slot, uint32_t n, tm_flip_frame *out)
{
    if (!s || !out) return TM_ERR_INVALID_ARG;
    if (s->n_last == 0 || first_slot + (uint64_t)n > s->n_last) return TM_ERR_STATE;
    const int rc = tm_flip_sync(s);
    if (rc) return rc;
    memcpy(out, s->h_res + first_slot, (size_t)n * sizeof(tm_flip_frame));
    return TM_OK;
}

int tm_flip_get_map(tm_flip *s, uint32_t slot, int kind, float *out, size_t pitch)
{
    if (!s || !out || kind < 0 || kind >= TMF_MAPS) return TM_ERR_INVALID_ARG;
    const size_t row = (size_t)s->g.w * sizeof(float);
    if (pitch < row || (pitch & 3)) return TM_ERR_INVALID_ARG;
    if (slot >= s->n_last) return TM_ERR_STATE;
    const int rc = tm_flip_sync(s);
    if (rc) return rc;
    if (hipSetDevice(s->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    const size_t px = (size_t)s->g.w * s->g.h;
    const float *src = s->d_maps + ((size_t)slot * TMF_MAPS + (size_t)kind) * px;
    FCHK(hipMemcpy2DAsync(out, pitch, src, row, row, s->g.h, hipMemcpyDeviceToHost, s->stream));
    FCHK(hipStreamSynchronize(s->stream));
    return TM_OK;
}

} // extern "C"
