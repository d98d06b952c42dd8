// haarpsi_host_test.cpp -- the host file of libturbometrics_haarpsi.so (csrc/tm_haarpsi.hip) against tests/host/fake_hip/hip/hip_runtime.h:
// no GPU, nothing loaded into Python.  Built and run by tests/test_haarpsi_host_cpu.py with -fsanitize=address,undefined, which catches
// what the fake's own books do not.  The file is compiled as it is (TM_EMULATE: the kernel header in its host form); the one thing a
// host compiler cannot do, the two launches, is this file's tm_haarpsi_host_test_launch: a plain loop over the 8-bit pairs of the launch
// that follows DESIGN.md section 21 position by position, every window summed tap by tap (the kernel's own s_of / q_of / w_of for the
// f32 expression), so that get and map are checked on values.
//   1  every position at which create (open, three or four device and two page-locked buffers) and a first host set_pair can fail: the
//      documented code, nothing live and nothing freed twice afterwards, and the object goes on after a failed set_pair
//   2  every position at which compute_async can fail: a failure after the first queued operation waits for the stream, nothing is
//      pending and the slots stay set
//   3  get and map: every position of their waits and copies; a failed wait leaves the compute pending and a later call delivers
//   4  the state rules: compute without set, a second compute while one is in flight (no HIP call is made), get synchronises, get
//      beyond the last compute, slots consumed, map without TM_HAARPSI_MAPS
//   5  the argument checks of every entry point and the host function
#include <hip/hip_runtime.h>

// what tm_haarpsi.hip calls beyond the fake's list
inline hipError_t hipMemcpy2D(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind)
{
    FAKE_HIP_CALL("hipMemcpy2D");
    for (size_t r = 0; r < height; ++r) memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
    return hipSuccess;
}

#define TM_EMULATE 1
#include "../../turbo-metrics_amd/csrc/tm_haarpsi.hip"

#include <cstdio>

thread_local uint3_ threadIdx, blockIdx; // the kernel header's host form names them; nothing here runs a kernel
thread_local dim3 blockDim, gridDim;
void tm_emul_syncthreads() {}
void tm_emul_wave_barrier() {}
void tm_emul_yield() {}

#define REQUIRE(cond)                                                                   \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "%s:%d: REQUIRE(%s) failed\n", __FILE__, __LINE__, #cond);   \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

namespace {
int g_launches = 0;
unsigned g_last_n = 0;
}

// the two launches: TM_HAARPSI_Y8 only; "device" memory is host memory here.  All of a slot's sums go to its first cell.
void tm_haarpsi_host_test_launch(const TmHaarpsiGeom &g, unsigned n_slots, const TmHaarpsiDesc *desc, float *maps, TmHaarpsiCell *cells, TmHaarpsiCell *res)
{
    ++g_launches;
    g_last_n = n_slots;
    REQUIRE(g.fmt == TMX_F_U8 && g.bits == 8 && g.c[0] == 1920 && g.c[1] == 7680 && (g.maps != 0) == (maps != nullptr));
    for (unsigned s = 0; s < n_slots; ++s) {
        auto S = [&](int p, int y, int x) -> int {
            if (y < 0 || x < 0 || y >= (int)g.h2 || x >= (int)g.w2) return 0;
            int v = 0;
            for (int dy = 0; dy < 2; ++dy)
                for (int dx = 0; dx < 2; ++dx)
                    if (2 * y + dy < (int)g.h && 2 * x + dx < (int)g.w) v += ((const unsigned char *)desc[s].p[p])[(size_t)(2 * y + dy) * desc[s].pitch[p] + 2 * x + dx];
            return v;
        };
        // the Haar coefficient of picture p at (y, x), scale k, orientation o (0: upper minus lower rows, 1: left minus right columns)
        auto H = [&](int p, int y, int x, int k, int o) -> int {
            const int K = 1 << k;
            int v = 0;
            for (int dy = -K / 2 + 1; dy <= K / 2; ++dy)
                for (int dx = -K / 2 + 1; dx <= K / 2; ++dx) v += ((o ? dx : dy) <= 0 ? 1 : -1) * S(p, y + dy, x + dx);
            return v;
        };
        TmHaarpsiCell out = {0.0, 0ull};
        for (int y = 0; y < (int)g.h2; ++y)
            for (int x = 0; x < (int)g.w2; ++x) {
                float sm = 0.0f;
                for (int o = 0; o < 2; ++o) {
                    const float so = tmp::s_of(H(0, y, x, 1, o), H(1, y, x, 1, o), H(0, y, x, 2, o), H(1, y, x, 2, o), g.c[0], g.c[1]);
                    const unsigned w = tmp::w_of(H(0, y, x, 3, o), H(1, y, x, 3, o));
                    out.q += (double)tmp::q_of(so) * (double)w;
                    out.ws += w;
                    sm += so;
                }
                if (maps) maps[((size_t)s * g.h2 + y) * g.w2 + x] = 0.5f * sm;
            }
        for (unsigned c = 0; c < g.cells; ++c) cells[(size_t)s * g.cells + c] = TmHaarpsiCell{0.0, 0ull};
        cells[(size_t)s * g.cells] = out;
        res[s] = out;
    }
}

namespace {

const uint32_t W = 7, H = 5, CAP = 3, N = W * H, W2 = 4, H2 = 3;
unsigned char zero[N], flat[N], ramp[N];

void pictures()
{
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            zero[y * W + x] = 0;
            flat[y * W + x] = 90;
            ramp[y * W + x] = (unsigned char)(3 * x + 5 * y);
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

int set(tm_haarpsi *m, uint32_t slot, const unsigned char *a, const unsigned char *b) { return tm_haarpsi_set_pair(m, slot, a, b, W, W, TM_MEM_HOST); }

void fail_next(long i, hipError_t err = hipErrorInvalidValue)
{
    fake_hip::State &s = fake_hip::state();
    s.fail_at = s.calls + i;
    s.fail_with = err;
    s.failed.clear();
}

void test_every_failure_position_of_create_and_set_pair()
{
    for (uint32_t flags : {0u, (uint32_t)TM_HAARPSI_MAPS}) {
        fake_hip::reset();
        tm_haarpsi *m = nullptr;
        REQUIRE(tm_haarpsi_create(&m, W, H, TM_HAARPSI_Y8, 8, CAP, flags) == TM_OK && m);
        const size_t counted = CAP * sizeof(TmHaarpsiCell) * 3 + 2 * CAP * sizeof(TmHaarpsiDesc) + (flags ? CAP * W2 * H2 * sizeof(float) : 0);
        REQUIRE(tm_haarpsi_mem_usage(m) == counted && tm_haarpsi_mem_usage(nullptr) == 0);
        REQUIRE(set(m, 1, ramp, flat) == TM_OK && tm_haarpsi_mem_usage(m) == counted + 2 * 256 * H);
        REQUIRE(set(m, 1, ramp, flat) == TM_OK && tm_haarpsi_mem_usage(m) == counted + 2 * 256 * H); // the surfaces are kept
        const std::vector<std::string> calls = fake_hip::state().log;
        const long n_dev = flags ? 4 : 3, n_create = 2 + n_dev + 2, n_first_set = 6; // set: hipSetDevice, 2 x (hipMalloc, hipMemcpy2DAsync), hipStreamSynchronize
        REQUIRE(calls[0] == "hipGetDevice" && calls[1] == "hipStreamCreateWithFlags" && calls[2] == "hipMalloc" && calls[n_create - 1] == "hipHostMalloc");
        REQUIRE(calls[n_create] == "hipSetDevice" && calls[n_create + 1] == "hipMalloc" && calls[n_create + n_first_set - 1] == "hipStreamSynchronize");
        REQUIRE((long)fake_hip::state().dev_allocs == n_dev + 2);
        tm_haarpsi_destroy(m);
        tm_haarpsi_destroy(nullptr);
        nothing_left();

        for (long k = 0; k < n_create + n_first_set; ++k)
            for (hipError_t err : {hipErrorOutOfMemory, hipErrorInvalidValue}) {
                fake_hip::reset(k, err);
                m = (tm_haarpsi *)&m;
                int rc = tm_haarpsi_create(&m, W, H, TM_HAARPSI_Y8, 8, CAP, flags);
                if (k < n_create) {
                    REQUIRE(m == nullptr && rc == documented(calls[k], err));
                } else {
                    REQUIRE(rc == TM_OK && m);
                    rc = set(m, 0, ramp, flat);
                    REQUIRE(rc == documented(calls[k], err));
                    REQUIRE(tm_haarpsi_compute_async(m, 1) == TM_ERR_STATE);                              // the slot does not count as set
                    REQUIRE(set(m, 0, ramp, flat) == TM_OK && tm_haarpsi_compute_async(m, 1) == TM_OK);   // the object goes on after the failure
                    tm_haarpsi_destroy(m);                                                                // with a compute pending
                }
                REQUIRE(fake_hip::state().failed == calls[k]);
                nothing_left();
            }
    }
}

void test_compute_get_map_and_state()
{
    fake_hip::reset();
    fake_hip::State &s = fake_hip::state();
    tm_haarpsi *m = nullptr;
    tm_haarpsi_frame f[CAP];
    float map[H2][W2 + 1];
    REQUIRE(tm_haarpsi_create(&m, W, H, TM_HAARPSI_Y8, 8, CAP, TM_HAARPSI_MAPS) == TM_OK);
    REQUIRE(tm_haarpsi_compute_async(m, 0) == TM_ERR_INVALID_ARG && tm_haarpsi_compute_async(m, CAP + 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_compute_async(m, 1) == TM_ERR_STATE);                 // compute without set
    REQUIRE(tm_haarpsi_get(m, 0, 1, f) == TM_ERR_STATE && tm_haarpsi_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_STATE); // nothing computed yet
    REQUIRE(set(m, 0, ramp, ramp) == TM_OK && tm_haarpsi_compute_async(m, 2) == TM_ERR_STATE); // slot 1 is not set
    REQUIRE(set(m, 1, zero, flat) == TM_OK && set(m, 2, ramp, flat) == TM_OK);

    // ---- a failure of operation i of the compute (0: hipSetDevice, 1: the descriptors, 2: the results)
    for (int i = 0; i < 3; ++i) {
        const long waits = s.waits;
        fail_next(i);
        REQUIRE(tm_haarpsi_compute_async(m, 3) == TM_ERR_HIP && !s.failed.empty());
        REQUIRE(s.waits == waits + (i >= 2 ? 1 : 0));                      // after the first queued operation: waited for, once
        REQUIRE(i < 2 || s.log.back() == "hipStreamSynchronize");
        REQUIRE(!m->c.pending && m->c.n_last == 0);
        for (uint32_t k = 0; k < 3; ++k) REQUIRE(m->c.have[k]);
    }
    const int launches = g_launches;
    REQUIRE(tm_haarpsi_compute_async(m, 3) == TM_OK && g_launches == launches + 1 && g_last_n == 3 && m->c.pending && m->c.n_last == 3);
    // ---- a second compute while one is in flight: refused before any HIP call, whatever the slots are
    m->c.have[0] = 1;
    const long calls = s.calls;
    REQUIRE(tm_haarpsi_compute_async(m, 1) == TM_ERR_STATE && s.calls == calls && m->c.pending);
    m->c.have[0] = 0;
    // ---- get and map synchronise; both positions of the wait can fail, the compute stays pending and a later call delivers
    for (int i = 0; i < 2; ++i) {
        fail_next(i);
        REQUIRE(tm_haarpsi_get(m, 0, 3, f) == TM_ERR_HIP && m->c.pending);
        fail_next(i);
        REQUIRE(tm_haarpsi_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_HIP && m->c.pending);
    }
    REQUIRE(tm_haarpsi_get(m, 3, 1, f) == TM_ERR_STATE && tm_haarpsi_get(m, 1, 3, f) == TM_ERR_STATE && tm_haarpsi_map(m, 3, &map[0][0], sizeof map[0]) == TM_ERR_STATE && m->c.pending);
    const long waits = s.waits;
    REQUIRE(tm_haarpsi_get(m, 0, 3, f) == TM_OK && !m->c.pending && s.waits == waits + 1);
    REQUIRE(tm_haarpsi_get(m, 1, 1, f + 1) == TM_OK && s.waits == waits + 1);
    // identical pictures: q is one constant, the score is 1 to its f32 rounding
    REQUIRE(f[0].ws > 0 && fabs(f[0].q / (double)f[0].ws - (double)tmp::q_of(1.0f)) < 1e-12 && fabs(tm_haarpsi_score(f[0].q, f[0].ws) - 1.0) < 1e-6);
    // zero against flat 90, 7 x 5 (S = 360 inside, 180 in column 3 and row 2, 90 at their crossing): every scale-3 window holds the whole
    // plane.  Hv_3(y): rows <= y minus rows > y of the row sums 1260, 1260, 630; Hh_3(x) likewise of the column sums 900, 900, 900, 450
    REQUIRE(f[1].ws == 4 * (630 + 1890 + 3150) + 3 * (1350 + 450 + 2250 + 3150));
    const double s1 = tm_haarpsi_score(f[1].q, f[1].ws), s2 = tm_haarpsi_score(f[2].q, f[2].ws);
    REQUIRE(s1 > 0.0 && s1 < 0.2 && s2 > 0.0 && s2 < 1.0);
    // ---- map: the two positions of its copy (hipSetDevice, hipMemcpy2D), a caller's pitch, the values
    for (int i = 0; i < 2; ++i) {
        fail_next(i);
        REQUIRE(tm_haarpsi_map(m, 1, &map[0][0], sizeof map[0]) == TM_ERR_HIP);
    }
    for (auto &r : map) for (float &v : r) v = -7.0f;
    REQUIRE(tm_haarpsi_map(m, 1, &map[0][0], sizeof map[0]) == TM_OK);
    for (uint32_t y = 0; y < H2; ++y) {
        REQUIRE(map[y][W2] == -7.0f);                                      // nothing beyond a row
        for (uint32_t x = 0; x < W2; ++x) REQUIRE(map[y][x] <= 1.0f && map[y][x] > 0.0f);
    }
    // position (0, 0) of zero against flat 90: Hv_1 = 720 - 720 = 0 = Hh_1; Hv_2 = S rows 0 minus rows 1, 2 over columns 0 .. 2:
    // 1080 - (1080 + 540) = -540, Hh_2 = columns 0 minus columns 1, 2 over rows 0 .. 2: 900 - 1800 = -900
    {
        const double ev = 0.5 * (540.0 * 540.0 / (540.0 * 540.0 + 7680.0)), eh = 0.5 * (900.0 * 900.0 / (900.0 * 900.0 + 7680.0));
        REQUIRE(fabs((double)map[0][0] - (1.0 - 0.5 * (ev + eh))) < 1e-6);
    }
    REQUIRE(tm_haarpsi_map(m, 0, &map[0][0], sizeof map[0]) == TM_OK && map[1][2] == 1.0f);
    REQUIRE(tm_haarpsi_map(m, 0, &map[0][0], 4 * W2 - 4) == TM_ERR_INVALID_ARG && tm_haarpsi_map(m, 0, &map[0][0], 4 * W2 + 2) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_map(m, 0, nullptr, sizeof map[0]) == TM_ERR_INVALID_ARG && tm_haarpsi_map(nullptr, 0, &map[0][0], sizeof map[0]) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_compute_async(m, 1) == TM_ERR_STATE);              // the compute consumed its slots
    // ---- set_pair waits for a pending compute first ("sync before set"); a smaller compute narrows what get covers
    REQUIRE(set(m, 0, ramp, flat) == TM_OK && tm_haarpsi_compute_async(m, 1) == TM_OK && m->c.pending);
    const long w2 = s.waits;
    REQUIRE(set(m, 0, flat, ramp) == TM_OK && !m->c.pending && s.waits == w2 + 2); // the pending compute, then the upload
    REQUIRE(tm_haarpsi_get(m, 0, 1, f) == TM_OK && tm_haarpsi_get(m, 1, 1, f) == TM_ERR_STATE && f[0].q == f[2].q && f[0].ws == f[2].ws);
    tm_haarpsi_destroy(m);
    nothing_left();

    REQUIRE(tm_haarpsi_create(&m, W, H, TM_HAARPSI_Y8, 8, 1, 0) == TM_OK);
    REQUIRE(set(m, 0, ramp, flat) == TM_OK && tm_haarpsi_compute_async(m, 1) == TM_OK);
    REQUIRE(tm_haarpsi_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_STATE); // created without TM_HAARPSI_MAPS
    REQUIRE(tm_haarpsi_get(m, 0, 1, f + 1) == TM_OK && f[1].q == f[2].q && f[1].ws == f[2].ws);
    tm_haarpsi_destroy(m);
    nothing_left();
}

void test_argument_checks_and_host_function()
{
    fake_hip::reset();
    tm_haarpsi *m = (tm_haarpsi *)&m;
    tm_haarpsi_frame f;
    REQUIRE(tm_haarpsi_create(nullptr, W, H, TM_HAARPSI_Y8, 8, 1, 0) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_create(&m, W, H, TM_HAARPSI_Y8, 8, 0, 0) == TM_ERR_INVALID_ARG && m == nullptr);
    REQUIRE(tm_haarpsi_create(&m, W, H, TM_HAARPSI_Y8, 8, 65536, 0) == TM_ERR_INVALID_ARG && tm_haarpsi_create(&m, W, H, TM_HAARPSI_Y8, 8, 1, 2) == TM_ERR_INVALID_ARG);
    const uint32_t bad[][4] = {{3, 5, TM_HAARPSI_Y8, 8}, {5, 3, TM_HAARPSI_Y8, 8}, {32769, 8, TM_HAARPSI_Y8, 8}, {8, 32769, TM_HAARPSI_Y8, 8}, {7, 5, TM_HAARPSI_Y8, 10},
                               {7, 5, TM_HAARPSI_Y16_MSB, 8}, {7, 5, TM_HAARPSI_Y16_LOW, 17}, {7, 5, TM_HAARPSI_Y10_PACKED, 12}, {7, 5, 4, 8}, {7, 5, TM_HAARPSI_Y8, 7}};
    for (const auto &b : bad) REQUIRE(tm_haarpsi_create(&m, b[0], b[1], (int)b[2], b[3], 1, 0) == TM_ERR_UNSUPPORTED && m == nullptr);
    REQUIRE(fake_hip::state().calls == 0);                                 // refused before any device call
    REQUIRE(tm_haarpsi_create(&m, W, H, TM_HAARPSI_Y16_LOW, 10, 2, 0) == TM_OK);
    static unsigned short y[W * H + 1];
    REQUIRE(tm_haarpsi_set_pair(nullptr, 0, y, y, 2 * W, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_haarpsi_set_pair(m, 2, y, y, 2 * W, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_set_pair(m, 0, nullptr, y, 2 * W, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_haarpsi_set_pair(m, 0, y, nullptr, 2 * W, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_set_pair(m, 0, y, y, 2 * W, 2 * W, 7) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_set_pair(m, 0, y, y, 2 * W - 2, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_haarpsi_set_pair(m, 0, y, y, 2 * W, 2 * W - 2, TM_MEM_HOST) == TM_ERR_INVALID_ARG); // pitch below a row
    REQUIRE(tm_haarpsi_set_pair(m, 0, (const char *)y + 1, y, 2 * W, 2 * W, TM_MEM_HOST) == TM_ERR_INVALID_ARG);  // odd base of 16-bit samples
    REQUIRE(tm_haarpsi_set_pair(m, 0, y, y, 2 * W, 2 * W + 1, TM_MEM_HOST) == TM_ERR_INVALID_ARG);                // odd pitch
    REQUIRE(tm_haarpsi_set_pair(m, 0, y, y, 2 * W, 2 * W, TM_MEM_DEVICE) == TM_OK && tm_haarpsi_mem_usage(m) > 0);  // in place: no staging surface
    REQUIRE(fake_hip::state().dev_allocs == 3);
    REQUIRE(tm_haarpsi_compute_async(nullptr, 1) == TM_ERR_INVALID_ARG && tm_haarpsi_sync(nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_get(nullptr, 0, 1, &f) == TM_ERR_INVALID_ARG && tm_haarpsi_get(m, 0, 1, nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_haarpsi_sync(m) == TM_OK);
    tm_haarpsi_destroy(m);
    nothing_left();

    REQUIRE(std::isnan(tm_haarpsi_score(0.0, 0)) && std::isnan(tm_haarpsi_score(1.0, 0)));
    const double a = (double)4.2f;
    REQUIRE(tm_haarpsi_score(0.25, 1) == (log(3.0) / a) * (log(3.0) / a) && tm_haarpsi_score(0.5, 1) == 0.0);
    const double x = 1.0 / (1.0 + exp(a * 0.75));                          // logit(sigmoid(A s)) / A = s with the f32 alpha
    REQUIRE(fabs(tm_haarpsi_score(x * 4096.0, 4096) - 0.75 * 0.75) < 1e-12);
}

} // namespace

int main()
{
    pictures();
    test_every_failure_position_of_create_and_set_pair();
    test_compute_get_map_and_state();
    test_argument_checks_and_host_function();
    fake_hip::reset();
    printf("haarpsi host ok\n");
    return 0;
}
