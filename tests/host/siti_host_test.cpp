// siti_host_test.cpp -- the host file of libturbometrics_siti.so (csrc/tm_siti.hip) against tests/host/fake_hip/hip/hip_runtime.h: no GPU,
// nothing loaded into Python.  Built and run by tests/test_siti_host_cpu.py with -fsanitize=address,undefined, which catches what the
// fake's own books do not.  The file is compiled as it is (TM_EMULATE: the kernel header in its host form); the one thing a host
// compiler cannot do, the launch, is this file's tm_siti_host_test_launch: a plain loop over the 8-bit pictures of the launch that
// follows DESIGN.md section 19, spreads its sums over the bins and keeps the history plane, so that get, first and reset are checked
// on values.
//   1  every position at which create (open, three device and two page-locked buffers) and a first host set_frame can fail: the
//      documented code, nothing live and nothing freed twice afterwards, and the object goes on after a failed set_frame
//   2  every position at which compute_async can fail: a failure after the first queued operation waits for the stream, nothing is
//      pending, the slots stay set and `first` stays what it was -- in the first batch of a sequence and in a later one
//   3  get: both positions of its wait; a failed wait leaves the compute pending and a later get delivers
//   4  the state rules: compute without set, a second compute while one is in flight (no HIP call is made), get synchronises, get
//      beyond the last compute, slots consumed; reset: ti_valid = 0 again, waits for a pending compute, and a failed reset changes nothing
//   5  the argument checks of every entry point, and T1 below zero through the two's-complement sum
#include <hip/hip_runtime.h>

// what tm_siti.hip calls beyond the fake's list
inline hipError_t hipMemsetAsync(void *dst, int v, size_t n, hipStream_t)
{
    FAKE_HIP_CALL("hipMemsetAsync");
    memset(dst, v, n);
    return hipSuccess;
}

#define TM_EMULATE 1
#include "../../turbo-metrics_amd/csrc/tm_siti.hip"

#include <cstdio>

#define REQUIRE(cond)                                                                   \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

namespace {
int g_launches = 0, g_last_first = -1, g_last_n = -1;
}

// the launch: TM_SITI_Y8 only; "device" memory is host memory here
void tm_siti_host_test_launch(const TmSitiGeom &g, const TmSitiDesc *desc, unsigned short *hist, unsigned long long *acc)
{
    ++g_launches;
    g_last_first = g.first;
    g_last_n = g.n;
    REQUIRE(g.fmt == TMX_F_U8 && g.bits == 8);
    for (int s = 0; s < g.n; ++s) {
        const unsigned char *p = (const unsigned char *)desc[s].p;
        const size_t pitch = desc[s].pitch;
        auto F = [&](int x, int y) { return (long long)p[(size_t)y * pitch + x]; };
        for (int y = 0; y < g.h; ++y) {
            unsigned long long *a = acc + ((size_t)s * TMI_BINS + (y % TMI_BINS)) * TMI_SUMS;
            for (int x = 0; x < g.w; ++x) {
                if (x >= 1 && x <= g.w - 2 && y >= 1 && y <= g.h - 2) {
                    const long long gx = (F(x + 1, y - 1) - F(x - 1, y - 1)) + 2 * (F(x + 1, y) - F(x - 1, y)) + (F(x + 1, y + 1) - F(x - 1, y + 1));
                    const long long gy = (F(x - 1, y + 1) - F(x - 1, y - 1)) + 2 * (F(x, y + 1) - F(x, y - 1)) + (F(x + 1, y + 1) - F(x + 1, y - 1));
                    const unsigned long long q = tmi::magnitude((unsigned long long)(gx * gx + gy * gy) << 16);
                    a[0] += q;
                    a[1] += q * q;
                }
                if (s > 0 || !g.first) {
                    const long long d = F(x, y) - (s > 0 ? (long long)((const unsigned char *)desc[s - 1].p)[(size_t)y * desc[s - 1].pitch + x]
                                                         : (long long)hist[(size_t)y * g.hpitch + x]);
                    a[2] += (unsigned long long)d; // two's complement
                    a[3] += (unsigned long long)(d * d);
                }
            }
        }
    }
    const unsigned char *p = (const unsigned char *)desc[g.n - 1].p;
    for (int y = 0; y < g.h; ++y)
        for (int x = 0; x < g.w; ++x) hist[(size_t)y * g.hpitch + x] = p[(size_t)y * desc[g.n - 1].pitch + x];
}

namespace {

const uint32_t W = 7, H = 5, CAP = 3, N = W * H;
unsigned char flat_a[N], flat_b[N], ramp[N];

void pictures()
{
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            flat_a[y * W + x] = 90;
            flat_b[y * W + x] = 84;
            ramp[y * W + x] = (unsigned char)(x + y);
        }
}

void nothing_left()
{
    const fake_hip::State &s = fake_hip::state();
    REQUIRE(s.dev.empty() && s.pinned.empty() && s.streams.empty() && s.bad_frees == 0);
}

int documented(const std::string &call, hipError_t err)
{
    if (call == "hipHostMalloc") return TM_ERR_OOM;
    if (call == "hipMalloc" && err == hipErrorOutOfMemory) return TM_ERR_OOM;
    return TM_ERR_HIP;
}

int set(tm_siti *m, uint32_t slot, const unsigned char *p) { return tm_siti_set_frame(m, slot, p, W, TM_MEM_HOST); }

void fail_next(long i, hipError_t err = hipErrorInvalidValue)
{
    fake_hip::State &s = fake_hip::state();
    s.fail_at = s.calls + i;
    s.fail_with = err;
    s.failed.clear();
}

void test_every_failure_position_of_create_and_set_frame()
{
    fake_hip::reset();
    tm_siti *m = nullptr;
    REQUIRE(tm_siti_create(&m, W, H, TM_SITI_Y8, 8, CAP) == TM_OK && m);
    const size_t res = CAP * TMI_BINS * TMI_SUMS * 8, counted = 64 * H * 2 + 2 * CAP * sizeof(TmSitiDesc) + 2 * res;
    REQUIRE(tm_siti_mem_usage(m) == counted && tm_siti_mem_usage(nullptr) == 0);
    REQUIRE(set(m, 1, ramp) == TM_OK && tm_siti_mem_usage(m) == counted + 256 * H);
    REQUIRE(set(m, 1, ramp) == TM_OK && tm_siti_mem_usage(m) == counted + 256 * H && fake_hip::state().dev_allocs == 4); // the surface is kept
    const std::vector<std::string> calls = fake_hip::state().log;
    const long n_create = 7, n_first_set = 4; // set: hipSetDevice, hipMalloc, hipMemcpy2DAsync, hipStreamSynchronize
    REQUIRE(calls[0] == "hipGetDevice" && calls[1] == "hipStreamCreateWithFlags" && calls[4] == "hipMalloc" && calls[6] == "hipHostMalloc");
    REQUIRE(calls[n_create] == "hipSetDevice" && calls[n_create + 1] == "hipMalloc" && calls[n_create + n_first_set - 1] == "hipStreamSynchronize");
    tm_siti_destroy(m);
    tm_siti_destroy(nullptr);
    nothing_left();

    for (long k = 0; k < n_create + n_first_set; ++k)
        for (hipError_t err : {hipErrorOutOfMemory, hipErrorInvalidValue}) {
            fake_hip::reset(k, err);
            m = (tm_siti *)&m;
            int rc = tm_siti_create(&m, W, H, TM_SITI_Y8, 8, CAP);
            if (k < n_create) {
                REQUIRE(m == nullptr && rc == documented(calls[k], err));
            } else {
                REQUIRE(rc == TM_OK && m);
                rc = set(m, 0, ramp);
                REQUIRE(rc == documented(calls[k], err));
                REQUIRE(tm_siti_compute_async(m, 1) == TM_ERR_STATE);      // the slot does not count as set
                REQUIRE(set(m, 0, ramp) == TM_OK && tm_siti_compute_async(m, 1) == TM_OK); // the object goes on after the failure
                tm_siti_destroy(m);                                         // with a compute pending
            }
            REQUIRE(fake_hip::state().failed == calls[k]);
            nothing_left();
        }
}

// a batch of `n` (<= 3) pictures, set and computed
int batch(tm_siti *m, const unsigned char *const *p, uint32_t n)
{
    for (uint32_t s = 0; s < n; ++s) REQUIRE(set(m, s, p[s]) == TM_OK);
    return tm_siti_compute_async(m, n);
}

void test_compute_get_state_and_reset()
{
    fake_hip::reset();
    fake_hip::State &s = fake_hip::state();
    tm_siti *m = nullptr;
    tm_siti_frame f[CAP];
    REQUIRE(tm_siti_create(&m, W, H, TM_SITI_Y8, 8, CAP) == TM_OK);
    REQUIRE(tm_siti_compute_async(m, 0) == TM_ERR_INVALID_ARG && tm_siti_compute_async(m, CAP + 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_siti_compute_async(m, 1) == TM_ERR_STATE);            // compute without set
    REQUIRE(tm_siti_get(m, 0, 1, f) == TM_ERR_STATE);                 // nothing computed yet
    REQUIRE(set(m, 0, ramp) == TM_OK && tm_siti_compute_async(m, 2) == TM_ERR_STATE); // slot 1 is not set

    const unsigned char *first_batch[3] = {ramp, flat_a, flat_b}, *second_batch[2] = {flat_a, ramp};
    const unsigned long long q = 2896, n_si = (W - 2) * (H - 2);
    for (int later = 0; later < 2; ++later) {
        // ---- a failure of operation i of the compute (0: hipSetDevice, 1: the descriptors, 2: the memset, 3: the results), in the
        // first batch of a sequence and in a later one
        for (uint32_t k = 0; k < (later ? 2u : 3u); ++k) REQUIRE(set(m, k, (later ? second_batch : first_batch)[k]) == TM_OK);
        const uint32_t n = later ? 2 : 3, n_last = m->c.n_last;
        for (int i = 0; i < 4; ++i) {
            const long waits = s.waits;
            fail_next(i);
            REQUIRE(tm_siti_compute_async(m, n) == TM_ERR_HIP && !s.failed.empty());
            REQUIRE(s.waits == waits + (i >= 2 ? 1 : 0));             // after the first queued operation: waited for, once
            REQUIRE(i < 2 || s.log.back() == "hipStreamSynchronize");
            REQUIRE(!m->c.pending && m->c.n_last == n_last && m->first == !later);
            for (uint32_t k = 0; k < n; ++k) REQUIRE(m->c.have[k]);
        }
        // (the launch of i = 3 ran and moved the history plane on: the slots are handed over again, as a caller would after an error)
        if (later) { REQUIRE(tm_siti_reset(m) == TM_OK && batch(m, first_batch, 3) == TM_OK && tm_siti_sync(m) == TM_OK); }
        const int launches = g_launches;
        REQUIRE(batch(m, later ? second_batch : first_batch, n) == TM_OK && g_launches == launches + 1);
        REQUIRE(g_last_first == !later && g_last_n == (int)n && !m->first && m->c.pending && m->c.n_last == n);
        // ---- a second compute while one is in flight: refused before any HIP call, whatever the slots are
        m->c.have[0] = 1;
        const long calls = s.calls;
        REQUIRE(tm_siti_compute_async(m, 1) == TM_ERR_STATE && s.calls == calls && m->c.pending);
        m->c.have[0] = 0;
        // ---- get synchronises; both positions of its wait can fail, the compute stays pending and a later get delivers
        for (int i = 0; i < 2; ++i) {
            fail_next(i);
            REQUIRE(tm_siti_get(m, 0, n, f) == TM_ERR_HIP && m->c.pending);
        }
        REQUIRE(tm_siti_get(m, n, 1, f) == TM_ERR_STATE && tm_siti_get(m, 1, n, f) == TM_ERR_STATE && m->c.pending); // beyond the last compute
        const long waits = s.waits;
        REQUIRE(tm_siti_get(m, 0, n, f) == TM_OK && !m->c.pending && s.waits == waits + 1);
        REQUIRE(tm_siti_get(m, 1, 1, f + 1) == TM_OK && s.waits == waits + 1);
        if (!later) {
            REQUIRE(f[0].ti_valid == 0 && f[0].t1 == 0 && f[0].t2 == 0 && f[0].ti == 0.0);
            REQUIRE(f[0].s1 == q * n_si && f[0].s2 == q * q * n_si && f[0].si == 0.0); // F = x + y: m2 = 128 everywhere
            REQUIRE(f[1].ti_valid == 1 && f[1].s1 == 0 && f[1].s2 == 0 && f[1].t1 == 90 * N - (0 + 1 + 2 + 3 + 4 + 5 + 6) * 5 - (0 + 1 + 2 + 3 + 4) * 7);
            REQUIRE(f[2].ti_valid == 1 && f[2].t1 == -6 * (int64_t)N && f[2].t2 == 36 * N && f[2].ti == 0.0); // T1 below zero
        } else {
            REQUIRE(f[0].ti_valid == 1 && f[0].t1 == 6 * (int64_t)N && f[0].t2 == 36 * N);  // against the last picture of the batch before
            REQUIRE(f[1].ti_valid == 1 && f[1].s1 == q * n_si && f[1].t1 == -(int64_t)(90 * N - 175));
        }
        REQUIRE(tm_siti_compute_async(m, 1) == TM_ERR_STATE);        // the compute consumed its slots
    }

    // ---- reset: a failed one changes nothing; one while a compute is pending waits for it; ti_valid = 0 again
    REQUIRE(batch(m, second_batch, 2) == TM_OK && m->c.pending);
    fail_next(0);
    REQUIRE(tm_siti_reset(m) == TM_ERR_HIP && !m->first && m->c.pending);
    const long waits = s.waits;
    REQUIRE(tm_siti_reset(m) == TM_OK && m->first && !m->c.pending && s.waits == waits + 1);
    REQUIRE(set(m, 0, flat_a) == TM_OK && tm_siti_reset(m) == TM_OK && tm_siti_compute_async(m, 1) == TM_ERR_STATE); // reset forgets the slots
    REQUIRE(batch(m, second_batch, 2) == TM_OK && g_last_first == 1);
    REQUIRE(tm_siti_get(m, 0, 2, f) == TM_OK && f[0].ti_valid == 0 && f[0].t2 == 0 && f[1].ti_valid == 1 && f[1].t2 > 0);
    REQUIRE(tm_siti_get(m, 1, 1, f) == TM_OK && f[0].ti_valid == 1); // slot 1 alone is not the first picture
    tm_siti_destroy(m);
    nothing_left();
}

void test_argument_checks()
{
    fake_hip::reset();
    tm_siti *m = (tm_siti *)&m;
    tm_siti_frame f;
    REQUIRE(tm_siti_create(nullptr, W, H, TM_SITI_Y8, 8, 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_siti_create(&m, W, H, TM_SITI_Y8, 8, 0) == TM_ERR_INVALID_ARG && m == nullptr);
    const uint32_t bad[][4] = {{2, 5, TM_SITI_Y8, 8}, {5, 2, TM_SITI_Y8, 8}, {8192, 8193, TM_SITI_Y8, 8}, {7, 5, TM_SITI_Y8, 10}, {7, 5, TM_SITI_Y16_MSB, 8},
                               {7, 5, TM_SITI_Y16_LOW, 17}, {7, 5, TM_SITI_Y10_PACKED, 12}, {7, 5, 4, 8}};
    for (const auto &b : bad) REQUIRE(tm_siti_create(&m, b[0], b[1], (int)b[2], b[3], 1) == TM_ERR_UNSUPPORTED && m == nullptr);
    REQUIRE(fake_hip::state().calls == 0);                             // refused before any device call
    REQUIRE(tm_siti_create(&m, W, H, TM_SITI_Y16_LOW, 10, 2) == TM_OK);
    static unsigned short y[W * H + 1];
    REQUIRE(tm_siti_set_frame(nullptr, 0, y, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_siti_set_frame(m, 2, y, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_siti_set_frame(m, 0, nullptr, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_siti_set_frame(m, 0, y, 2 * W, 7) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_siti_set_frame(m, 0, y, 2 * W - 2, TM_MEM_HOST) == TM_ERR_INVALID_ARG);                    // pitch below a row
    REQUIRE(tm_siti_set_frame(m, 0, (const char *)y + 1, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG);      // odd base of 16-bit samples
    REQUIRE(tm_siti_set_frame(m, 0, y, 2 * W + 1, TM_MEM_HOST) == TM_ERR_INVALID_ARG);                    // odd pitch
    REQUIRE(tm_siti_set_frame(m, 0, y, 2 * W, TM_MEM_DEVICE) == TM_OK && tm_siti_mem_usage(m) > 0);      // in place: no staging surface
    REQUIRE(fake_hip::state().dev_allocs == 3);
    REQUIRE(tm_siti_compute_async(nullptr, 1) == TM_ERR_INVALID_ARG && tm_siti_sync(nullptr) == TM_ERR_INVALID_ARG && tm_siti_reset(nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_siti_get(nullptr, 0, 1, &f) == TM_ERR_INVALID_ARG && tm_siti_get(m, 0, 1, nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_siti_sync(m) == TM_OK);
    tm_siti_destroy(m);
    nothing_left();
}

} // namespace

int main()
{
    pictures();
    test_every_failure_position_of_create_and_set_frame();
    test_compute_get_state_and_reset();
    test_argument_checks();
    fake_hip::reset();
    printf("siti host ok\n");
    return 0;
}
