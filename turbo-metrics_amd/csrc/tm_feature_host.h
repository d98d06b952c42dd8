// tm_feature_host.h -- the host core the fifteen feature libraries share (tm_xpsnr.hip ... tm_mdsi.hip): the state
// every handle carries, create / destroy plumbing, the staging upload of host pictures and the set -> compute_async -> sync -> get
// state machine.  Host code only: a plain struct and free functions, no kernels and no entry points -- every library keeps its own
// create, set_*, compute_async and get, and embeds TmFeatureHost as the member `c`.  tests/host/feature_host_test.cpp compiles this
// header against a fake hip_runtime.h and walks every failure position.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "../../include/turbo_metrics_hip.h"

// a failed HIP call is TM_ERR_HIP, with the runtime's sticky error cleared
#define TMFH_CHK(call)                                  \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

// The same inside compute_async after its first queued operation: a failure must not leave work behind that still reads the descriptors
// and the staging surfaces while the caller believes nothing is pending, so what was queued is waited for before the error is reported.
#define TMFH_CHK_QUEUED(c, call)                        \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            tmfh_drain(c);                              \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

struct TmFeatureHost {
    int device = 0;
    hipStream_t stream = nullptr;        // the object's own non-blocking stream
    uint32_t cap = 0;                    // slots
    size_t bytes = 0;                    // what mem_usage reports
    bool pending = false;                // a compute is queued and not yet waited for
    uint32_t n_last = 0;                 // slots of the last compute
    std::vector<unsigned char> have;     // [slot] or [slot][side]: set since the last compute
    std::vector<void *> staging;         // device copies of host pictures, allocated at a slot's first host picture
};

// the four luma formats of tm_sample_load.h and the packed 10-bit row of tm_geom.h, which this header does not see: a library that
// passes its g.fmt to the row helpers below states TMFH_FORMATS_AGREE where it sees both
enum { TMFH_U8 = 0, TMFH_U16_MSB = 1, TMFH_U16_LOW = 2, TMFH_P10 = 3 };
enum { TMFH_P10_RUN = 128, TMFH_P10_BLOCK = 3 * TMFH_P10_RUN };
#define TMFH_FORMATS_AGREE                                                                                                              \
    static_assert(TMX_F_U8 == TMFH_U8 && TMX_F_U16_MSB == TMFH_U16_MSB && TMX_F_U16_LOW == TMFH_U16_LOW && TMX_F_P10 == TMFH_P10 &&     \
                  TM_P10_RUN == TMFH_P10_RUN && TM_P10_BLOCK == TMFH_P10_BLOCK, "formats")

// bytes of one luma row of w samples
static inline size_t tmfh_row_bytes(int fmt, size_t w)
{
    switch (fmt) {
    case TMFH_U8: return w;
    case TMFH_P10: return (w + TMFH_P10_BLOCK - 1) / TMFH_P10_BLOCK * TMFH_P10_RUN * 4;
    default: return w * 2;
    }
}

// what the plane pointers and pitches of a format are multiples of
static inline size_t tmfh_align(int fmt) { return fmt == TMFH_P10 ? 4 : (fmt == TMFH_U8 ? 1 : 2); }

static inline bool tmfh_mem_ok(int mem) { return mem == TM_MEM_HOST || mem == TM_MEM_DEVICE || mem == TM_MEM_HOST_PINNED; }

// the kernels' 16-byte loads need every plane pointer and pitch or-ed into `bits` to be a multiple of 16
static inline int tmfh_vec(uintptr_t bits) { return (bits & 15) == 0; }

// row pitch of a staging surface
static inline size_t tmfh_pitch(size_t row) { return (row + 255) / 256 * 256; }

// The device and the stream of a new object, `have` and `staging` sized.  After a failure (TM_ERR_HIP) the object holds nothing: the
// caller deletes it without going through its destroy.
static inline int tmfh_open(TmFeatureHost *c, uint32_t cap, size_t n_have, size_t n_staging)
{
    c->cap = cap;
    TMFH_CHK(hipGetDevice(&c->device));
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        c->stream = nullptr;
        return TM_ERR_HIP;
    }
    c->have.assign(n_have, 0);
    c->staging.assign(n_staging, nullptr);
    return TM_OK;
}

// device memory, counted; *p stays as it was on failure
template <class T>
static inline int tmfh_dev_alloc(TmFeatureHost *c, T **p, size_t n)
{
    const hipError_t r = hipMalloc((void **)p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    TMFH_CHK(r);
    c->bytes += n;
    return TM_OK;
}

// page-locked host memory, counted; any failure is TM_ERR_OOM and leaves *p null
template <class T>
static inline int tmfh_pinned_alloc(TmFeatureHost *c, T **p, size_t n)
{
    if (hipHostMalloc((void **)p, n, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; return TM_ERR_OOM; }
    c->bytes += n;
    return TM_OK;
}

// the staging surface `idx`, `need` bytes at its first use
static inline int tmfh_staging(TmFeatureHost *c, size_t idx, size_t need, void **out)
{
    if (!c->staging[idx]) {
        const int rc = tmfh_dev_alloc(c, &c->staging[idx], need);
        if (rc) return rc;
    }
    *out = c->staging[idx];
    return TM_OK;
}

// one host plane of `rows` rows of `row` bytes into staging surface `idx`, queued on the stream: where the kernel reads it
static inline int tmfh_upload(TmFeatureHost *c, size_t idx, const void *src, size_t src_pitch, size_t row, size_t rows, const void **dev,
                              unsigned long long *pitch)
{
    const size_t sp = tmfh_pitch(row);
    void *st;
    const int rc = tmfh_staging(c, idx, sp * rows, &st);
    if (rc) return rc;
    TMFH_CHK(hipMemcpy2DAsync(st, sp, src, src_pitch, row, rows, hipMemcpyHostToDevice, c->stream));
    *dev = st; *pitch = sp;
    return TM_OK;
}

// one host 4:2:0 picture into staging surface `idx`, which is one allocation: the luma plane (rows_y rows of row_y bytes), then `nc`
// chroma planes (rows_c rows of row_c bytes; nc 1: u is the interleaved CbCr plane and v is not read, p[2] is null)
static inline int tmfh_upload_420(TmFeatureHost *c, size_t idx, const void *y, const void *u, const void *v, size_t pitch_y, size_t pitch_uv,
                                  size_t row_y, size_t row_c, size_t rows_y, size_t rows_c, int nc, const void *p[3], unsigned long long pitch[2])
{
    const size_t sp_y = tmfh_pitch(row_y), sp_c = tmfh_pitch(row_c);
    void *st;
    const int rc = tmfh_staging(c, idx, sp_y * rows_y + nc * sp_c * rows_c, &st);
    if (rc) return rc;
    char *s = (char *)st;
    TMFH_CHK(hipMemcpy2DAsync(s, sp_y, y, pitch_y, row_y, rows_y, hipMemcpyHostToDevice, c->stream));
    TMFH_CHK(hipMemcpy2DAsync(s + sp_y * rows_y, sp_c, u, pitch_uv, row_c, rows_c, hipMemcpyHostToDevice, c->stream));
    if (nc == 2) TMFH_CHK(hipMemcpy2DAsync(s + sp_y * rows_y + sp_c * rows_c, sp_c, v, pitch_uv, row_c, rows_c, hipMemcpyHostToDevice, c->stream));
    p[0] = s; p[1] = s + sp_y * rows_y; p[2] = nc == 2 ? s + sp_y * rows_y + sp_c * rows_c : nullptr;
    pitch[0] = sp_y; pitch[1] = sp_c;
    return TM_OK;
}

// waits for the pending compute, if there is one
static inline int tmfh_sync(TmFeatureHost *c)
{
    if (!c->pending) return TM_OK;
    TMFH_CHK(hipSetDevice(c->device));
    TMFH_CHK(hipStreamSynchronize(c->stream));
    c->pending = false;
    return TM_OK;
}

// compute_async's way in: n_slots slots of `per_slot` flags each.  TM_ERR_INVALID_ARG for a count outside 1 .. cap, TM_ERR_STATE while
// a compute is pending or for a slot not set since the last one; then the device is made current.
static inline int tmfh_begin(TmFeatureHost *c, uint32_t n_slots, uint32_t per_slot)
{
    if (n_slots == 0 || n_slots > c->cap) return TM_ERR_INVALID_ARG;
    if (c->pending) return TM_ERR_STATE;
    for (size_t i = 0; i < (size_t)per_slot * n_slots; ++i)
        if (!c->have[i]) return TM_ERR_STATE;
    TMFH_CHK(hipSetDevice(c->device));
    return TM_OK;
}

// after a failed HIP call of compute_async: waits for what was queued before it (TMFH_CHK_QUEUED)
static inline void tmfh_drain(TmFeatureHost *c)
{
    (void)hipGetLastError();
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
}

// compute_async's way out.  Every batch hands its pictures over anew: a slot not set again before the next compute is TM_ERR_STATE,
// not a stale picture.
static inline void tmfh_queued(TmFeatureHost *c, uint32_t n_slots, uint32_t per_slot)
{
    c->pending = true;
    std::fill(c->have.begin(), c->have.begin() + (size_t)per_slot * n_slots, 0);
    c->n_last = n_slots;
}

// get: slots [first, first + n) are slots of the last compute
static inline bool tmfh_in_last(const TmFeatureHost *c, uint32_t first, uint32_t n) { return c->n_last != 0 && first + (uint64_t)n <= c->n_last; }

// destroy: waits for the stream, frees the staging surfaces, the object's device buffers and its page-locked ones (null ones are
// skipped), then the stream
static inline void tmfh_close(TmFeatureHost *c, std::initializer_list<void *> dev, std::initializer_list<void *> pinned)
{
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (void *p : c->staging) if (p) (void)hipFree(p);
    for (void *p : dev) if (p) (void)hipFree(p);
    for (void *p : pinned) if (p) (void)hipHostFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    (void)hipGetLastError();
    c->staging.clear();
    c->stream = nullptr;
}
