// itp_host_test.cpp -- the host file of libturbometrics_itp.so (csrc/tm_itp.hip) against tests/host/fake_hip/hip/hip_runtime.h: no GPU,
// nothing loaded into Python.  Built and run by tests/test_itp_host_cpu.py with -fsanitize=address,undefined, which catches what the
// fake's own books do not.  The file is compiled as it is (TM_EMULATE: the kernel header in its host form); the one thing a host
// compiler cannot do, the two launches, is this file's tm_itp_host_test_launch: a plain loop over the 8-bit I420 pairs of the launch that
// follows DESIGN.md section 22 position by position with the kernel's own tmi::ictcp_of / de_itp, so that get and get_map are checked
// on values.
//   1  every position at which create (open, three or four device and two page-locked buffers) and a first host set_frame can fail: the
//      documented code, nothing live and nothing freed twice afterwards, and the object goes on after a failed set_frame
//   2  every position at which compute_async can fail: a failure after the first queued operation waits for the stream, nothing is
//      pending and the slots stay set
//   3  get and get_map: every position of their waits and copies; a failed wait leaves the compute pending and a later call delivers
//   4  the state rules: compute without set, a second compute while one is in flight (no HIP call is made), get synchronises, get
//      beyond the last compute, slots consumed, get_map without want_map
//   5  the argument checks of every entry point and the host functions
#include <hip/hip_runtime.h>

// what tm_itp.hip calls beyond the fake's list
inline hipError_t hipMemcpy2D(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind)
{
    FAKE_HIP_CALL("hipMemcpy2D");
    for (size_t r = 0; r < height; ++r) memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
    return hipSuccess;
}

#define TM_EMULATE 1
#include "../../turbo-metrics_amd/csrc/tm_itp.hip"

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

// the two launches: TM_ITP_I420 at 8 bits only; "device" memory is host memory here.  All of a slot's sums go to its first cell.
void tm_itp_host_test_launch(const TmItpGeom &gi, unsigned n_slots, const TmCiedeDesc *desc, float *maps, TmCiedeCell *cells, TmCiedeCell *res)
{
    const TmCiedeGeom &g = gi.b;
    ++g_launches;
    g_last_n = n_slots;
    REQUIRE(g.fmt == TMX_F_U8 && g.bits == 8 && g.layout == TMC_I420 && g.yoff == 16 && g.coff == 128 && g.c[0] == 1.4746f);
    for (unsigned s = 0; s < n_slots; ++s) {
        TmCiedeCell out = {0.0, 0.0f, 0.0f};
        for (unsigned y = 0; y < g.h; ++y)
            for (unsigned x = 0; x < g.w; ++x) {
                tmi::Itp t[2];
                for (int side = 0; side < 2; ++side) {
                    const TmCiedeDesc &d = desc[2 * s + side];
                    const int Y = ((const unsigned char *)d.p0)[(size_t)y * d.pitch + x];
                    const int U = ((const unsigned char *)d.p1)[(size_t)(y >> 1) * d.pitch2 + (x >> 1)];
                    const int V = ((const unsigned char *)d.p2)[(size_t)(y >> 1) * d.pitch2 + (x >> 1)];
                    const float yn = (float)(Y - g.yoff) / g.ydiv, un = (float)(U - g.coff) / g.cdiv, vn = (float)(V - g.coff) / g.cdiv;
                    t[side] = tmi::ictcp_of(yn, g.c[0] * vn, g.c[1] * un, g.c[2] * vn, g.c[3] * un, gi.transfer);
                }
                const float de = tmi::de_itp(t[0], t[1]);
                out.sum += (double)de;
                out.max = fmaxf(out.max, de);
                if (maps) maps[((size_t)s * g.h + y) * g.w + x] = de;
            }
        for (unsigned c = 0; c < g.cells; ++c) cells[(size_t)s * g.cells + c] = TmCiedeCell{0.0, 0.0f, 0.0f};
        cells[(size_t)s * g.cells] = out;
        res[s] = out;
    }
}

namespace {

const uint32_t W = 7, H = 5, CAP = 3, CW = 4, CH = 3;
unsigned char grey[W * H], step[W * H], ramp[W * H], cn[CW * CH], cr[CW * CH];

void pictures()
{
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            grey[y * W + x] = 126;
            step[y * W + x] = 127;
            ramp[y * W + x] = (unsigned char)(20 + 6 * x + 9 * y);
        }
    for (uint32_t i = 0; i < CW * CH; ++i) { cn[i] = 128; cr[i] = (unsigned char)(100 + 5 * i); }
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

int set(tm_itp *m, uint32_t slot, int side, const unsigned char *y, const unsigned char *u, const unsigned char *v)
{
    return tm_itp_set_frame(m, slot, side, y, u, v, W, CW, TM_MEM_HOST);
}
int set_pair(tm_itp *m, uint32_t slot, const unsigned char *ya, const unsigned char *yb, const unsigned char *cb)
{
    const int rc = set(m, slot, TM_SIDE_REF, ya, cn, cn);
    return rc ? rc : set(m, slot, TM_SIDE_DIS, yb, cb, cn);
}

void fail_next(long i, hipError_t err = hipErrorInvalidValue)
{
    fake_hip::State &s = fake_hip::state();
    s.fail_at = s.calls + i;
    s.fail_with = err;
    s.failed.clear();
}

void test_every_failure_position_of_create_and_set_frame()
{
    for (int want_map : {0, 1}) {
        fake_hip::reset();
        tm_itp *m = nullptr;
        REQUIRE(tm_itp_create(&m, W, H, TM_ITP_I420, 8, TM_ITP_PQ, 0, want_map, CAP) == TM_OK && m);
        const size_t counted = CAP * sizeof(TmCiedeCell) * 3 + 2 * 2 * CAP * sizeof(TmCiedeDesc) + (want_map ? CAP * W * H * sizeof(float) : 0);
        REQUIRE(tm_itp_mem_usage(m) == counted && tm_itp_mem_usage(nullptr) == 0);
        REQUIRE(set(m, 1, TM_SIDE_DIS, ramp, cr, cn) == TM_OK);
        const size_t with_surface = tm_itp_mem_usage(m);
        REQUIRE(with_surface > counted);
        REQUIRE(set(m, 1, TM_SIDE_DIS, ramp, cr, cn) == TM_OK && tm_itp_mem_usage(m) == with_surface); // the surface is kept
        const std::vector<std::string> calls = fake_hip::state().log;
        const long n_dev = want_map ? 4 : 3, n_create = 2 + n_dev + 2, n_first_set = 6; // set: hipSetDevice, hipMalloc, 3 x hipMemcpy2DAsync, hipStreamSynchronize
        REQUIRE(calls[0] == "hipGetDevice" && calls[1] == "hipStreamCreateWithFlags" && calls[2] == "hipMalloc" && calls[n_create - 1] == "hipHostMalloc");
        REQUIRE(calls[n_create] == "hipSetDevice" && calls[n_create + 1] == "hipMalloc" && calls[n_create + 2] == "hipMemcpy2DAsync" &&
                calls[n_create + n_first_set - 1] == "hipStreamSynchronize");
        REQUIRE((long)fake_hip::state().dev_allocs == n_dev + 1);
        tm_itp_destroy(m);
        tm_itp_destroy(nullptr);
        nothing_left();

        for (long k = 0; k < n_create + n_first_set; ++k)
            for (hipError_t err : {hipErrorOutOfMemory, hipErrorInvalidValue}) {
                fake_hip::reset(k, err);
                m = (tm_itp *)&m;
                int rc = tm_itp_create(&m, W, H, TM_ITP_I420, 8, TM_ITP_PQ, 0, want_map, CAP);
                if (k < n_create) {
                    REQUIRE(m == nullptr && rc == documented(calls[k], err));
                } else {
                    REQUIRE(rc == TM_OK && m);
                    rc = set(m, 0, TM_SIDE_REF, ramp, cr, cn);
                    REQUIRE(rc == documented(calls[k], err));
                    REQUIRE(set(m, 0, TM_SIDE_DIS, ramp, cn, cn) == TM_OK);
                    REQUIRE(tm_itp_compute_async(m, 1) == TM_ERR_STATE);                                         // the side does not count as set
                    REQUIRE(set(m, 0, TM_SIDE_REF, ramp, cr, cn) == TM_OK && tm_itp_compute_async(m, 1) == TM_OK); // the object goes on
                    tm_itp_destroy(m);                                                                           // with a compute pending
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
    tm_itp *m = nullptr;
    tm_itp_frame f[CAP];
    float map[H][W + 1];
    REQUIRE(tm_itp_create(&m, W, H, TM_ITP_I420, 8, TM_ITP_PQ, 0, 1, CAP) == TM_OK);
    REQUIRE(tm_itp_compute_async(m, 0) == TM_ERR_INVALID_ARG && tm_itp_compute_async(m, CAP + 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_compute_async(m, 1) == TM_ERR_STATE);                   // compute without set
    REQUIRE(tm_itp_get(m, 0, 1, f) == TM_ERR_STATE && tm_itp_get_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_STATE); // nothing computed yet
    REQUIRE(set(m, 0, TM_SIDE_REF, ramp, cr, cn) == TM_OK && tm_itp_compute_async(m, 1) == TM_ERR_STATE);              // one side only
    REQUIRE(set(m, 0, TM_SIDE_DIS, ramp, cr, cn) == TM_OK && tm_itp_compute_async(m, 2) == TM_ERR_STATE);              // slot 1 is not set
    REQUIRE(set_pair(m, 1, grey, step, cn) == TM_OK && set_pair(m, 2, ramp, ramp, cr) == TM_OK);

    // ---- a failure of operation i of the compute (0: hipSetDevice, 1: the descriptors, 2: the results)
    for (int i = 0; i < 3; ++i) {
        const long waits = s.waits;
        fail_next(i);
        REQUIRE(tm_itp_compute_async(m, 3) == TM_ERR_HIP && !s.failed.empty());
        REQUIRE(s.waits == waits + (i >= 2 ? 1 : 0));                      // after the first queued operation: waited for, once
        REQUIRE(i < 2 || s.log.back() == "hipStreamSynchronize");
        REQUIRE(!m->c.pending && m->c.n_last == 0);
        for (uint32_t k = 0; k < 6; ++k) REQUIRE(m->c.have[k]);
    }
    const int launches = g_launches;
    REQUIRE(tm_itp_compute_async(m, 3) == TM_OK && g_launches == launches + 1 && g_last_n == 3 && m->c.pending && m->c.n_last == 3);
    // ---- a second compute while one is in flight: refused before any HIP call, whatever the slots are
    m->c.have[0] = m->c.have[1] = 1;
    const long calls = s.calls;
    REQUIRE(tm_itp_compute_async(m, 1) == TM_ERR_STATE && s.calls == calls && m->c.pending);
    m->c.have[0] = m->c.have[1] = 0;
    // ---- get and get_map synchronise; both positions of the wait can fail, the compute stays pending and a later call delivers
    for (int i = 0; i < 2; ++i) {
        fail_next(i);
        REQUIRE(tm_itp_get(m, 0, 3, f) == TM_ERR_HIP && m->c.pending);
        fail_next(i);
        REQUIRE(tm_itp_get_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_HIP && m->c.pending);
    }
    REQUIRE(tm_itp_get(m, 3, 1, f) == TM_ERR_STATE && tm_itp_get(m, 1, 3, f) == TM_ERR_STATE && tm_itp_get_map(m, 3, &map[0][0], sizeof map[0]) == TM_ERR_STATE && m->c.pending);
    const long waits = s.waits;
    REQUIRE(tm_itp_get(m, 0, 3, f) == TM_OK && !m->c.pending && s.waits == waits + 1);
    REQUIRE(tm_itp_get(m, 1, 1, f + 1) == TM_OK && s.waits == waits + 1);
    // identical pictures: exactly 0; a flat luma step: every position the double function's value
    REQUIRE(f[0].de_sum == 0.0 && f[0].de_max == 0.0 && f[0].de_mean == 0.0 && f[0].pixels == W * H);
    double a[3], b[3];
    REQUIRE(tm_itp_ictcp(126, 128, 128, 8, TM_ITP_PQ, a) == TM_OK && tm_itp_ictcp(127, 128, 128, 8, TM_ITP_PQ, b) == TM_OK);
    const double de = tm_itp_de(a, b);
    REQUIRE(de > 2.0 && de < 5.0 && fabs(f[1].de_mean - de) < 4 * 6.7e-4 + 4 * 5.9e-4 * de && fabs(f[1].de_max - de) < 4 * 6.7e-4 + 4 * 5.9e-4 * de);
    REQUIRE(f[1].de_mean == f[1].de_sum / (W * H) && f[2].de_sum > 0.0 && f[2].de_max >= f[2].de_mean);
    // ---- get_map: the two positions of its copy (hipSetDevice, hipMemcpy2D), a caller's pitch, the values
    for (int i = 0; i < 2; ++i) {
        fail_next(i);
        REQUIRE(tm_itp_get_map(m, 1, &map[0][0], sizeof map[0]) == TM_ERR_HIP);
    }
    for (auto &r : map) for (float &v : r) v = -7.0f;
    REQUIRE(tm_itp_get_map(m, 1, &map[0][0], sizeof map[0]) == TM_OK);
    for (uint32_t y = 0; y < H; ++y) {
        REQUIRE(map[y][W] == -7.0f);                                       // nothing beyond a row
        for (uint32_t x = 0; x < W; ++x) REQUIRE((double)map[y][x] == f[1].de_max);
    }
    REQUIRE(tm_itp_get_map(m, 0, &map[0][0], sizeof map[0]) == TM_OK && map[1][2] == 0.0f);
    REQUIRE(tm_itp_get_map(m, 0, &map[0][0], 4 * W - 4) == TM_ERR_INVALID_ARG && tm_itp_get_map(m, 0, &map[0][0], 4 * W + 2) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_get_map(m, 0, nullptr, sizeof map[0]) == TM_ERR_INVALID_ARG && tm_itp_get_map(nullptr, 0, &map[0][0], sizeof map[0]) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_compute_async(m, 1) == TM_ERR_STATE);                   // the compute consumed its slots
    // ---- set_frame waits for a pending compute first ("sync before set"); a smaller compute narrows what get covers
    REQUIRE(set_pair(m, 0, ramp, ramp, cr) == TM_OK && tm_itp_compute_async(m, 1) == TM_OK && m->c.pending);
    const long w2 = s.waits;
    REQUIRE(set(m, 0, TM_SIDE_REF, grey, cn, cn) == TM_OK && !m->c.pending && s.waits == w2 + 2); // the pending compute, then the upload
    REQUIRE(tm_itp_get(m, 0, 1, f) == TM_OK && tm_itp_get(m, 1, 1, f) == TM_ERR_STATE && f[0].de_sum == f[2].de_sum && f[0].de_max == f[2].de_max);
    tm_itp_destroy(m);
    nothing_left();

    REQUIRE(tm_itp_create(&m, W, H, TM_ITP_I420, 8, TM_ITP_HLG, 0, 0, 1) == TM_OK);
    REQUIRE(set_pair(m, 0, ramp, ramp, cr) == TM_OK && tm_itp_compute_async(m, 1) == TM_OK);
    REQUIRE(tm_itp_get_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_STATE); // created without want_map
    REQUIRE(tm_itp_get(m, 0, 1, f + 1) == TM_OK && f[1].de_sum > 0.0 && f[1].de_sum != f[2].de_sum); // the other transfer
    tm_itp_destroy(m);
    nothing_left();
}

void test_argument_checks_and_host_functions()
{
    fake_hip::reset();
    tm_itp *m = (tm_itp *)&m;
    tm_itp_frame f;
    REQUIRE(tm_itp_create(nullptr, W, H, TM_ITP_I420, 8, 0, 0, 0, 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_create(&m, W, H, TM_ITP_I420, 8, 0, 0, 0, 0) == TM_ERR_INVALID_ARG && m == nullptr);
    REQUIRE(tm_itp_create(&m, W, H, TM_ITP_I420, 8, 0, 0, 0, 65536) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_create(&m, W, H, TM_ITP_I420, 8, 2, 0, 0, 1) == TM_ERR_INVALID_ARG && tm_itp_create(&m, W, H, TM_ITP_I420, 8, -1, 0, 0, 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_create(&m, W, H, TM_ITP_I420, 8, 0, 1, 0, 1) == TM_ERR_UNSUPPORTED);  // full range
    const uint32_t bad[][4] = {{1, 5, TM_ITP_I420, 8}, {5, 1, TM_ITP_I420, 8}, {32769, 8, TM_ITP_I420, 8}, {8, 32769, TM_ITP_I420, 8}, {7, 5, TM_ITP_NV12, 10},
                               {7, 5, TM_ITP_P016, 8}, {7, 5, TM_ITP_I420, 17}, {7, 5, TM_ITP_I420P10_PACKED, 12}, {7, 5, 4, 8}, {7, 5, TM_ITP_I420, 7}};
    for (const auto &b : bad) REQUIRE(tm_itp_create(&m, b[0], b[1], (int)b[2], b[3], 0, 0, 0, 1) == TM_ERR_UNSUPPORTED && m == nullptr);
    REQUIRE(fake_hip::state().calls == 0);                                 // refused before any device call
    REQUIRE(tm_itp_create(&m, W, H, TM_ITP_I420, 10, TM_ITP_PQ, 0, 0, 2) == TM_OK);
    static unsigned short y[W * H + 1], c[CW * CH + 1];
    const size_t py = 2 * W, pc = 2 * CW;
    REQUIRE(tm_itp_set_frame(nullptr, 0, 0, y, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_itp_set_frame(m, 2, 0, y, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_set_frame(m, 0, 2, y, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_set_frame(m, 0, 0, nullptr, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_itp_set_frame(m, 0, 0, y, nullptr, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_set_frame(m, 0, 0, y, c, nullptr, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);                 // three planes are needed
    REQUIRE(tm_itp_set_frame(m, 0, 0, y, c, c, py, pc, 7) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_set_frame(m, 0, 0, y, c, c, py - 2, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_itp_set_frame(m, 0, 0, y, c, c, py, pc - 2, TM_MEM_HOST) == TM_ERR_INVALID_ARG); // pitch below a row
    REQUIRE(tm_itp_set_frame(m, 0, 0, (const char *)y + 1, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);      // odd base of 16-bit samples
    REQUIRE(tm_itp_set_frame(m, 0, 0, y, c, c, py, pc + 1, TM_MEM_HOST) == TM_ERR_INVALID_ARG);                   // odd pitch
    REQUIRE(tm_itp_set_frame(m, 0, 0, y, c, c, py, pc, TM_MEM_DEVICE) == TM_OK && tm_itp_mem_usage(m) > 0);        // in place: no staging surface
    REQUIRE(fake_hip::state().dev_allocs == 3);
    REQUIRE(tm_itp_compute_async(nullptr, 1) == TM_ERR_INVALID_ARG && tm_itp_sync(nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_get(nullptr, 0, 1, &f) == TM_ERR_INVALID_ARG && tm_itp_get(m, 0, 1, nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_sync(m) == TM_OK);
    tm_itp_destroy(m);
    nothing_left();

    double o[3], g[3] = {0.75, 0.75, 0.75};
    REQUIRE(tm_itp_ictcp(64, 512, 512, 7, 0, o) == TM_ERR_UNSUPPORTED && tm_itp_ictcp(64, 512, 512, 17, 0, o) == TM_ERR_UNSUPPORTED);
    REQUIRE(tm_itp_ictcp(64, 512, 512, 10, 2, o) == TM_ERR_INVALID_ARG && tm_itp_ictcp(64, 512, 512, 10, 0, nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(std::isnan(tm_itp_de(nullptr, o)) && std::isnan(tm_itp_de(o, nullptr)));
    REQUIRE(tm_itp_hlg_display(nullptr, o) == TM_ERR_INVALID_ARG && tm_itp_hlg_display(g, nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_itp_hlg_display(g, o) == TM_OK && fabs(o[0] - 203.0) < 0.5 && o[0] == o[1] && o[1] == o[2]);
    REQUIRE(fabs(tm_itp_pq_inv_eotf(100.0) - 0.5081) < 5e-5 && fabs(tm_itp_pq_inv_eotf(1000.0) - 0.7518) < 5e-5 && tm_itp_pq_inv_eotf(10000.0) == 1.0);
    REQUIRE(tm_itp_pq_eotf(0.0) == 0.0 && tm_itp_pq_eotf(-1.0) == 0.0 && tm_itp_pq_eotf(1.0) == 10000.0 && tm_itp_pq_eotf(2.0) == 10000.0);
    REQUIRE(tm_itp_pq_inv_eotf(-5.0) == tm_itp_pq_inv_eotf(0.0) && tm_itp_pq_inv_eotf(20000.0) == 1.0);
}

} // namespace

int main()
{
    pictures();
    test_every_failure_position_of_create_and_set_frame();
    test_compute_get_map_and_state();
    test_argument_checks_and_host_functions();
    fake_hip::reset();
    printf("itp host ok\n");
    return 0;
}
