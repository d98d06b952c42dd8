// feature_host_test.cpp -- csrc/tm_feature_host.h against tests/host/fake_hip/hip/hip_runtime.h: no GPU, nothing loaded into Python.
// Built and run by tests/test_feature_host_cpu.py with -fsanitize=address,undefined, which catches what the fake's own books do not.
//   1  every position at which create (open, three device and two page-locked buffers) and a first host upload can fail: the
//      return code is the documented one and after close nothing is live and nothing was freed twice
//   2  compute_async: a failure after the first queued operation waits for the stream before it returns and leaves nothing pending;
//      the set -> compute -> sync -> get rules
//   3  the staging pitch and size at rows of 1, 255, 256 and 257 bytes, and the single allocation of a 4:2:0 picture
//   4  row_bytes and align of the four luma formats at widths 1, 383, 384, 385 (the packed 10-bit block is 384 samples)
#include "../../turbo-metrics_amd/csrc/tm_feature_host.h"

#include <cstdio>

#define REQUIRE(cond)                                                                   \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

namespace {

// an object the way the ten libraries build theirs
struct Obj {
    TmFeatureHost c;
    char *d_a = nullptr, *d_b = nullptr, *d_c = nullptr;
    char *h_a = nullptr, *h_b = nullptr;
};

const uint32_t kCap = 2;
const size_t kRow = 100, kRows = 3;

void destroy(Obj *o)
{
    if (!o) return;
    tmfh_close(&o->c, {o->d_a, o->d_b, o->d_c}, {o->h_a, o->h_b});
    delete o;
}

int create(Obj **out)
{
    *out = nullptr;
    Obj *o = new Obj();
    int rc;
    if ((rc = tmfh_open(&o->c, kCap, kCap, 2 * kCap))) { delete o; return rc; }
    if ((rc = tmfh_dev_alloc(&o->c, &o->d_a, 64)) || (rc = tmfh_dev_alloc(&o->c, &o->d_b, 0)) || (rc = tmfh_dev_alloc(&o->c, &o->d_c, 32)) ||
        (rc = tmfh_pinned_alloc(&o->c, &o->h_a, 16)) || (rc = tmfh_pinned_alloc(&o->c, &o->h_b, 8))) {
        destroy(o);
        return rc;
    }
    *out = o;
    return TM_OK;
}

// a pair of host planes into the two staging surfaces of a slot, like set_pair with TM_MEM_HOST
int set_pair(Obj *o, uint32_t slot, const char *a, const char *b)
{
    int rc;
    if ((rc = tmfh_sync(&o->c))) return rc;
    TMFH_CHK(hipSetDevice(o->c.device));
    const char *src[2] = {a, b};
    for (int p = 0; p < 2; ++p) {
        const void *dev;
        unsigned long long pitch;
        if ((rc = tmfh_upload(&o->c, 2 * slot + p, src[p], kRow, kRow, kRows, &dev, &pitch))) return rc;
        REQUIRE(pitch == 256 && dev == o->c.staging[2 * slot + p]);
    }
    TMFH_CHK(hipStreamSynchronize(o->c.stream));
    o->c.have[slot] = 1;
    return TM_OK;
}

// a compute_async of three queued operations
int compute(Obj *o, uint32_t n)
{
    const int rc = tmfh_begin(&o->c, n, 1);
    if (rc) return rc;
    TMFH_CHK(hipMemcpyAsync(o->d_a, o->h_a, 16, hipMemcpyHostToDevice, o->c.stream));
    TMFH_CHK_QUEUED(&o->c, hipMemcpyAsync(o->d_c, o->d_a, 16, hipMemcpyHostToDevice, o->c.stream));
    TMFH_CHK_QUEUED(&o->c, hipMemcpyAsync(o->h_b, o->d_c, 8, hipMemcpyDeviceToHost, o->c.stream));
    tmfh_queued(&o->c, n, 1);
    return TM_OK;
}

void nothing_left()
{
    const fake_hip::State &s = fake_hip::state();
    REQUIRE(s.dev.empty() && s.pinned.empty() && s.streams.empty() && s.bad_frees == 0);
}

// what a failure of `call` with `err` is documented to return
int documented(const std::string &call, hipError_t err)
{
    if (call == "hipHostMalloc") return TM_ERR_OOM;
    if (call == "hipMalloc" && err == hipErrorOutOfMemory) return TM_ERR_OOM;
    return TM_ERR_HIP;
}

void test_every_failure_position()
{
    char plane[kRow * kRows] = {};
    // the clean run: which calls there are
    fake_hip::reset();
    Obj *o;
    REQUIRE(create(&o) == TM_OK && o);
    const size_t counted = 64 + 0 + 32 + 16 + 8;
    REQUIRE(o->c.bytes == counted);
    REQUIRE(set_pair(o, 1, plane, plane) == TM_OK);
    REQUIRE(o->c.bytes == counted + 2 * 256 * kRows);
    REQUIRE(set_pair(o, 1, plane, plane) == TM_OK); // the surfaces are kept
    REQUIRE(o->c.bytes == counted + 2 * 256 * kRows && fake_hip::state().dev_allocs == 5);
    const std::vector<std::string> calls = fake_hip::state().log;
    const long n_create = 7, n_first_set = 6; // set: hipSetDevice, (hipMalloc, hipMemcpy2DAsync) x 2, hipStreamSynchronize
    REQUIRE(calls[0] == "hipGetDevice" && calls[1] == "hipStreamCreateWithFlags" && calls[6] == "hipHostMalloc");
    REQUIRE(calls[n_create] == "hipSetDevice" && calls[n_create + n_first_set - 1] == "hipStreamSynchronize");
    destroy(o);
    nothing_left();

    for (long k = 0; k < n_create + n_first_set; ++k)
        for (hipError_t err : {hipErrorOutOfMemory, hipErrorInvalidValue}) {
            fake_hip::reset(k, err);
            int rc = create(&o);
            if (k < n_create) {
                REQUIRE(o == nullptr && rc == documented(calls[k], err));
            } else {
                REQUIRE(rc == TM_OK);
                rc = set_pair(o, 0, plane, plane);
                REQUIRE(rc == documented(calls[k], err) && !o->c.have[0]);
                REQUIRE(set_pair(o, 0, plane, plane) == TM_OK && o->c.have[0]); // the object goes on after the failure
                destroy(o);
            }
            REQUIRE(fake_hip::state().failed == calls[k]);
            nothing_left();
        }
    // the quirk kept from before: a failing hipGetDevice leaves nothing to close, a failing stream creation no stream to wait for
    fake_hip::reset(0, hipErrorInvalidValue);
    REQUIRE(create(&o) == TM_ERR_HIP && fake_hip::state().calls == 1 && fake_hip::state().waits == 0);
    fake_hip::reset(1, hipErrorInvalidValue);
    REQUIRE(create(&o) == TM_ERR_HIP && fake_hip::state().calls == 2 && fake_hip::state().waits == 0);
}

void test_compute_state_and_drain()
{
    char plane[kRow * kRows] = {};
    fake_hip::reset();
    Obj *o;
    REQUIRE(create(&o) == TM_OK);
    REQUIRE(compute(o, 0) == TM_ERR_INVALID_ARG && compute(o, kCap + 1) == TM_ERR_INVALID_ARG);
    REQUIRE(compute(o, 1) == TM_ERR_STATE);                       // slot 0 is not set
    REQUIRE(!tmfh_in_last(&o->c, 0, 0) && !tmfh_in_last(&o->c, 0, 1));
    REQUIRE(set_pair(o, 0, plane, plane) == TM_OK && set_pair(o, 1, plane, plane) == TM_OK);

    // a failure of operation i of the compute (0: hipSetDevice, 1 .. 3: the three copies)
    for (int i = 0; i < 4; ++i) {
        fake_hip::State &s = fake_hip::state();
        const long waits = s.waits;
        s.fail_at = s.calls + i;
        s.fail_with = hipErrorInvalidValue;
        REQUIRE(compute(o, 2) == TM_ERR_HIP);
        REQUIRE(s.waits == waits + (i >= 2 ? 1 : 0));             // after the first queued operation: waited for, once
        REQUIRE(i < 2 || s.log.back() == "hipStreamSynchronize"); // ... as the last thing before returning
        REQUIRE(!o->c.pending && o->c.n_last == 0 && o->c.have[0] && o->c.have[1]);
    }
    REQUIRE(compute(o, 2) == TM_OK);
    REQUIRE(o->c.pending && o->c.n_last == 2 && !o->c.have[0] && !o->c.have[1]);
    REQUIRE(compute(o, 2) == TM_ERR_STATE);                       // one compute at a time
    REQUIRE(tmfh_in_last(&o->c, 0, 2) && tmfh_in_last(&o->c, 1, 1) && !tmfh_in_last(&o->c, 1, 2) && !tmfh_in_last(&o->c, 2, 1));
    REQUIRE(!tmfh_in_last(&o->c, 0xffffffffu, 2));                // no 32-bit wrap
    const long waits = fake_hip::state().waits;
    REQUIRE(tmfh_sync(&o->c) == TM_OK && !o->c.pending && fake_hip::state().waits == waits + 1);
    REQUIRE(tmfh_sync(&o->c) == TM_OK && fake_hip::state().waits == waits + 1); // nothing pending, nothing waited for
    REQUIRE(compute(o, 1) == TM_ERR_STATE);                       // the compute consumed its slots
    REQUIRE(set_pair(o, 0, plane, plane) == TM_OK && compute(o, 2) == TM_ERR_STATE && compute(o, 1) == TM_OK && o->c.n_last == 1);
    // a failing wait leaves the compute pending
    fake_hip::state().fail_at = fake_hip::state().calls + 1;
    fake_hip::state().fail_with = hipErrorInvalidValue;
    REQUIRE(tmfh_sync(&o->c) == TM_ERR_HIP && o->c.pending);
    destroy(o);                                                   // with a compute pending: close waits first
    nothing_left();
}

void test_staging_geometry()
{
    const size_t rows = 3;
    static char src[257 * rows];
    const size_t row[4] = {1, 255, 256, 257}, want[4] = {256, 256, 256, 512};
    fake_hip::reset();
    TmFeatureHost c;
    REQUIRE(tmfh_open(&c, 4, 4, 6) == TM_OK && c.have.size() == 4 && c.staging.size() == 6 && c.cap == 4);
    size_t bytes = 0;
    for (int i = 0; i < 4; ++i) {
        const void *dev;
        unsigned long long pitch;
        REQUIRE(tmfh_pitch(row[i]) == want[i]);
        REQUIRE(tmfh_upload(&c, i, src, row[i], row[i], rows, &dev, &pitch) == TM_OK);
        REQUIRE(pitch == want[i] && fake_hip::state().last_dev_size == want[i] * rows && dev == c.staging[i]);
        bytes += want[i] * rows;
        REQUIRE(c.bytes == bytes && fake_hip::state().dev_allocs == i + 1);
    }
    // a 4:2:0 picture is one allocation: luma, then the chroma planes
    const void *p[3];
    unsigned long long pitch[2];
    REQUIRE(tmfh_upload_420(&c, 4, src, src, src, 257, 129, 257, 129, 3, 2, 2, p, pitch) == TM_OK);
    REQUIRE(pitch[0] == 512 && pitch[1] == 256 && fake_hip::state().last_dev_size == 512 * 3 + 2 * 256 * 2);
    REQUIRE(p[0] == c.staging[4] && (const char *)p[1] == (const char *)p[0] + 512 * 3 && (const char *)p[2] == (const char *)p[1] + 256 * 2);
    REQUIRE(tmfh_upload_420(&c, 5, src, src, nullptr, 257, 256, 257, 256, 3, 2, 1, p, pitch) == TM_OK);
    REQUIRE(pitch[0] == 512 && pitch[1] == 256 && fake_hip::state().last_dev_size == 512 * 3 + 256 * 2 && p[2] == nullptr);
    REQUIRE(fake_hip::state().dev_allocs == 6);
    tmfh_close(&c, {}, {});
    nothing_left();
}

void test_row_helpers()
{
    const size_t w[4] = {1, 383, 384, 385}, p10[4] = {512, 512, 512, 1024};
    for (int i = 0; i < 4; ++i) {
        REQUIRE(tmfh_row_bytes(TMFH_U8, w[i]) == w[i]);
        REQUIRE(tmfh_row_bytes(TMFH_U16_MSB, w[i]) == 2 * w[i] && tmfh_row_bytes(TMFH_U16_LOW, w[i]) == 2 * w[i]);
        REQUIRE(tmfh_row_bytes(TMFH_P10, w[i]) == p10[i]);
    }
    REQUIRE(tmfh_align(TMFH_U8) == 1 && tmfh_align(TMFH_U16_MSB) == 2 && tmfh_align(TMFH_U16_LOW) == 2 && tmfh_align(TMFH_P10) == 4);
    REQUIRE(tmfh_mem_ok(TM_MEM_HOST) && tmfh_mem_ok(TM_MEM_DEVICE) && tmfh_mem_ok(TM_MEM_HOST_PINNED) && !tmfh_mem_ok(-1) && !tmfh_mem_ok(3));
    REQUIRE(tmfh_vec(0x1000 | 256) && !tmfh_vec(0x1008) && !tmfh_vec(0x1000 | 24));
}

} // namespace

int main()
{
    test_every_failure_position();
    test_compute_state_and_drain();
    test_staging_geometry();
    test_row_helpers();
    fake_hip::reset();
    printf("feature host ok\n");
    return 0;
}
