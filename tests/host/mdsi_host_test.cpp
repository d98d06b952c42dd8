// mdsi_host_test.cpp -- the host file of libturbometrics_mdsi.so (csrc/tm_mdsi.hip) against tests/host/fake_hip/hip/hip_runtime.h: no
// GPU, nothing loaded into Python.  Built and run by tests/test_mdsi_host_cpu.py with -fsanitize=address,undefined, which catches what
// the fake's own books do not.  The file is compiled as it is (TM_EMULATE: the kernel header in its host form); the one thing a host
// compiler cannot do, the four launches, is this file's tm_mdsi_host_test_launch: a plain loop over the 8-bit I420 pairs of the launch
// that follows DESIGN.md section 23 position by position with the kernel header's own functions, so that get and map are checked on
// values.
//   1  every position at which create (open, five device and two page-locked buffers) and a first host set_frame can fail: the
//      documented code, nothing live and nothing freed twice afterwards, and the object goes on after a failed set_frame
//   2  every position at which compute_async can fail: a failure after the first queued operation waits for the stream, nothing is
//      pending and the slots stay set
//   3  get and map: every position of their waits and copies; a failed wait leaves the compute pending and a later call delivers
//   4  the state rules: compute without set, a second compute while one is in flight (no HIP call is made), get synchronises, get
//      beyond the last compute, slots consumed, map without TM_MDSI_MAPS
//   5  the argument checks of every entry point and the host functions
#include <hip/hip_runtime.h>

// what tm_mdsi.hip calls beyond the fake's list
inline hipError_t hipMemcpy2D(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind)
{
    FAKE_HIP_CALL("hipMemcpy2D");
    for (size_t r = 0; r < height; ++r) memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
    return hipSuccess;
}

#define TM_EMULATE 1
#include "../../turbo-metrics_amd/csrc/tm_mdsi.hip"

#include <cstdio>
#include <vector>

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

// the four launches: TM_MDSI_I420 at 8 bits only; "device" memory is host memory here.  A plain loop over the positions with the kernel
// header's own tmm::box_sums / plane_of / gcs_of / z_of.  All of a slot's sums go to its first cell.
void tm_mdsi_host_test_launch(const TmMdsiGeom &g, unsigned n_slots, const TmCiedeDesc *desc, float *maps, TmMdsiCell *cells, TmMdsiCell *cells2,
                              TmMdsiRes *res)
{
    ++g_launches;
    g_last_n = n_slots;
    REQUIRE(g.b.fmt == TMX_F_U8 && g.b.bits == 8 && g.b.layout == TMC_I420 && maps && g.n == (unsigned long long)g.wd * g.hd);
    const int wd = (int)g.wd, hd = (int)g.hd;
    for (unsigned s = 0; s < n_slots; ++s) {
        std::vector<tmm::real> P(2 * 3 * (size_t)(wd + 2) * (hd + 2), (tmm::real)0.0); // [picture][plane][row + 1][column + 1], zeros around
        auto at = [&](int p, int q, int j, int i) -> tmm::real & { return P[(((size_t)p * 3 + q) * (hd + 2) + (j + 1)) * (wd + 2) + (i + 1)]; };
        for (int p = 0; p < 2; ++p)
            for (int j = 0; j < hd; ++j)
                for (int i = 0; i < wd; ++i) {
                    const tmm::Sums sm = tmm::box_sums<TMC_I420, TMX_F_U8>(g, desc[2 * s + p], i, j);
                    for (int q = 0; q < 3; ++q) at(p, q, j, i) = tmm::plane_of(g, q, sm);
                }
        TmMdsiRes out = {0.0, 0.0, 0.0, 0};
        float *m = maps + (size_t)s * g.n;
        for (int j = 0; j < hd; ++j)
            for (int i = 0; i < wd; ++i) {
                tmm::real gx[2], gy[2];
                for (int p = 0; p < 2; ++p) {
                    gx[p] = (((at(p, 0, j - 1, i + 1) - at(p, 0, j - 1, i - 1)) + (at(p, 0, j, i + 1) - at(p, 0, j, i - 1))) + (at(p, 0, j + 1, i + 1) - at(p, 0, j + 1, i - 1))) / (tmm::real)3.0;
                    gy[p] = (((at(p, 0, j + 1, i - 1) - at(p, 0, j - 1, i - 1)) + (at(p, 0, j + 1, i) - at(p, 0, j - 1, i))) + (at(p, 0, j + 1, i + 1) - at(p, 0, j - 1, i + 1))) / (tmm::real)3.0;
                }
                const float gcs = tmm::gcs_of(gx[0], gy[0], gx[1], gy[1], at(0, 1, j, i), at(1, 1, j, i), at(0, 2, j, i), at(1, 2, j, i));
                m[(size_t)j * wd + i] = gcs;
                const tmm::Z z = tmm::z_of(gcs);
                out.re += z.re; out.im += z.im; out.neg += gcs < 0.0f;
            }
        const double mur = out.re / (double)g.n, mui = out.im / (double)g.n;
        for (size_t k = 0; k < g.n; ++k) {
            const tmm::Z z = tmm::z_of(m[k]);
            out.dev += sqrt((z.re - mur) * (z.re - mur) + (z.im - mui) * (z.im - mui));
        }
        for (unsigned c = 0; c < g.cells; ++c) cells[(size_t)s * g.cells + c] = TmMdsiCell{0.0, 0.0, 0};
        for (unsigned c = 0; c < g.cells2; ++c) cells2[(size_t)s * g.cells2 + c] = TmMdsiCell{0.0, 0.0, 0};
        cells[(size_t)s * g.cells] = TmMdsiCell{out.re, out.im, out.neg};
        cells2[(size_t)s * g.cells2] = TmMdsiCell{out.dev, 0.0, 0};
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

int set(tm_mdsi *m, uint32_t slot, int side, const unsigned char *y, const unsigned char *u, const unsigned char *v)
{
    return tm_mdsi_set_frame(m, slot, side, y, u, v, W, CW, TM_MEM_HOST);
}
int set_pair(tm_mdsi *m, uint32_t slot, const unsigned char *ya, const unsigned char *yb, const unsigned char *cb)
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
    for (uint32_t flags : {0u, (uint32_t)TM_MDSI_MAPS}) {
        fake_hip::reset();
        tm_mdsi *m = nullptr;
        REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, TM_MDSI_BT709, 1, flags, CAP) == TM_OK && m);
        const size_t counted = CAP * sizeof(TmMdsiCell) * 2 + 2 * CAP * sizeof(TmMdsiRes) + 2 * 2 * CAP * sizeof(TmCiedeDesc) + CAP * W * H * sizeof(float); // one tile, one chunk
        REQUIRE(tm_mdsi_mem_usage(m) == counted && tm_mdsi_mem_usage(nullptr) == 0 && tm_mdsi_get_factor(m) == 1 && tm_mdsi_get_factor(nullptr) == 0);
        REQUIRE(set(m, 1, TM_SIDE_DIS, ramp, cr, cn) == TM_OK);
        const size_t with_surface = tm_mdsi_mem_usage(m);
        REQUIRE(with_surface > counted);
        REQUIRE(set(m, 1, TM_SIDE_DIS, ramp, cr, cn) == TM_OK && tm_mdsi_mem_usage(m) == with_surface); // the surface is kept
        const std::vector<std::string> calls = fake_hip::state().log;
        const long n_dev = 5, n_create = 2 + n_dev + 2, n_first_set = 6; // set: hipSetDevice, hipMalloc, 3 x hipMemcpy2DAsync, hipStreamSynchronize
        REQUIRE(calls[0] == "hipGetDevice" && calls[1] == "hipStreamCreateWithFlags" && calls[2] == "hipMalloc" && calls[n_create - 1] == "hipHostMalloc");
        REQUIRE(calls[n_create] == "hipSetDevice" && calls[n_create + 1] == "hipMalloc" && calls[n_create + 2] == "hipMemcpy2DAsync" &&
                calls[n_create + n_first_set - 1] == "hipStreamSynchronize");
        REQUIRE((long)fake_hip::state().dev_allocs == n_dev + 1);
        tm_mdsi_destroy(m);
        tm_mdsi_destroy(nullptr);
        nothing_left();

        for (long k = 0; k < n_create + n_first_set; ++k)
            for (hipError_t err : {hipErrorOutOfMemory, hipErrorInvalidValue}) {
                fake_hip::reset(k, err);
                m = (tm_mdsi *)&m;
                int rc = tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, TM_MDSI_BT709, 1, flags, CAP);
                if (k < n_create) {
                    REQUIRE(m == nullptr && rc == documented(calls[k], err));
                } else {
                    REQUIRE(rc == TM_OK && m);
                    rc = set(m, 0, TM_SIDE_REF, ramp, cr, cn);
                    REQUIRE(rc == documented(calls[k], err));
                    REQUIRE(set(m, 0, TM_SIDE_DIS, ramp, cn, cn) == TM_OK);
                    REQUIRE(tm_mdsi_compute_async(m, 1) == TM_ERR_STATE);                                         // the side does not count as set
                    REQUIRE(set(m, 0, TM_SIDE_REF, ramp, cr, cn) == TM_OK && tm_mdsi_compute_async(m, 1) == TM_OK); // the object goes on
                    tm_mdsi_destroy(m);                                                                           // with a compute pending
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
    tm_mdsi *m = nullptr;
    tm_mdsi_frame f[CAP];
    float map[H][W + 1];
    REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, TM_MDSI_BT709, 1, TM_MDSI_MAPS, CAP) == TM_OK);
    REQUIRE(tm_mdsi_compute_async(m, 0) == TM_ERR_INVALID_ARG && tm_mdsi_compute_async(m, CAP + 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_compute_async(m, 1) == TM_ERR_STATE);                   // compute without set
    REQUIRE(tm_mdsi_get(m, 0, 1, f) == TM_ERR_STATE && tm_mdsi_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_STATE); // nothing computed yet
    REQUIRE(set(m, 0, TM_SIDE_REF, ramp, cr, cn) == TM_OK && tm_mdsi_compute_async(m, 1) == TM_ERR_STATE);              // one side only
    REQUIRE(set(m, 0, TM_SIDE_DIS, ramp, cr, cn) == TM_OK && tm_mdsi_compute_async(m, 2) == TM_ERR_STATE);              // slot 1 is not set
    REQUIRE(set_pair(m, 1, grey, step, cn) == TM_OK && set_pair(m, 2, ramp, ramp, cr) == TM_OK);

    // ---- a failure of operation i of the compute (0: hipSetDevice, 1: the descriptors, 2: the results)
    for (int i = 0; i < 3; ++i) {
        const long waits = s.waits;
        fail_next(i);
        REQUIRE(tm_mdsi_compute_async(m, 3) == TM_ERR_HIP && !s.failed.empty());
        REQUIRE(s.waits == waits + (i >= 2 ? 1 : 0));                      // after the first queued operation: waited for, once
        REQUIRE(i < 2 || s.log.back() == "hipStreamSynchronize");
        REQUIRE(!m->c.pending && m->c.n_last == 0);
        for (uint32_t k = 0; k < 6; ++k) REQUIRE(m->c.have[k]);
    }
    const int launches = g_launches;
    REQUIRE(tm_mdsi_compute_async(m, 3) == TM_OK && g_launches == launches + 1 && g_last_n == 3 && m->c.pending && m->c.n_last == 3);
    // ---- a second compute while one is in flight: refused before any HIP call, whatever the slots are
    m->c.have[0] = m->c.have[1] = 1;
    const long calls = s.calls;
    REQUIRE(tm_mdsi_compute_async(m, 1) == TM_ERR_STATE && s.calls == calls && m->c.pending);
    m->c.have[0] = m->c.have[1] = 0;
    // ---- get and get_map synchronise; both positions of the wait can fail, the compute stays pending and a later call delivers
    for (int i = 0; i < 2; ++i) {
        fail_next(i);
        REQUIRE(tm_mdsi_get(m, 0, 3, f) == TM_ERR_HIP && m->c.pending);
        fail_next(i);
        REQUIRE(tm_mdsi_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_HIP && m->c.pending);
    }
    REQUIRE(tm_mdsi_get(m, 3, 1, f) == TM_ERR_STATE && tm_mdsi_get(m, 1, 3, f) == TM_ERR_STATE && tm_mdsi_map(m, 3, &map[0][0], sizeof map[0]) == TM_ERR_STATE && m->c.pending);
    const long waits = s.waits;
    REQUIRE(tm_mdsi_get(m, 0, 3, f) == TM_OK && !m->c.pending && s.waits == waits + 1);
    REQUIRE(tm_mdsi_get(m, 1, 1, f + 1) == TM_OK && s.waits == waits + 1);
    // identical pictures: exactly 0 and a map of ones; a flat luma step: flat interior, damage only where the zero border meets the step
    REQUIRE(f[0].dev == 0.0 && f[0].sum_im == 0.0 && f[0].sum_re == (double)(W * H) && f[0].n == W * H && f[0].negatives == 0 && f[0].factor == 1);
    REQUIRE(tm_mdsi_score(f[0].dev, f[0].n) == 0.0);
    REQUIRE(f[1].dev > 0.0 && f[1].sum_im == 0.0 && f[1].negatives == 0 && f[2].dev > 0.0); // slot 2 differs in Cb only
    const double mdsi1 = tm_mdsi_score(f[1].dev, f[1].n);
    REQUIRE(mdsi1 > 0.0 && mdsi1 < 0.2);                                   // one luma code on a flat picture
    // ---- get_map: the two positions of its copy (hipSetDevice, hipMemcpy2D), a caller's pitch, the values
    for (int i = 0; i < 2; ++i) {
        fail_next(i);
        REQUIRE(tm_mdsi_map(m, 1, &map[0][0], sizeof map[0]) == TM_ERR_HIP);
    }
    for (auto &r : map) for (float &v : r) v = -7.0f;
    REQUIRE(tm_mdsi_map(m, 1, &map[0][0], sizeof map[0]) == TM_OK);
    for (uint32_t y = 0; y < H; ++y) {
        REQUIRE(map[y][W] == -7.0f);                                       // nothing beyond a row
        for (uint32_t x = 0; x < W; ++x) REQUIRE(map[y][x] > 0.99f && map[y][x] <= 1.0f);
    }
    REQUIRE(map[2][3] > 0.9999f && map[2][3] < 1.0f);                     // the flat interior: no gradient; H and M carry 1 % and 9 % of the luma step
    REQUIRE(tm_mdsi_map(m, 0, &map[0][0], sizeof map[0]) == TM_OK && map[1][2] == 1.0f);
    REQUIRE(tm_mdsi_map(m, 0, &map[0][0], 4 * W - 4) == TM_ERR_INVALID_ARG && tm_mdsi_map(m, 0, &map[0][0], 4 * W + 2) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_map(m, 0, nullptr, sizeof map[0]) == TM_ERR_INVALID_ARG && tm_mdsi_map(nullptr, 0, &map[0][0], sizeof map[0]) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_compute_async(m, 1) == TM_ERR_STATE);                   // the compute consumed its slots
    // ---- set_frame waits for a pending compute first ("sync before set"); a smaller compute narrows what get covers
    REQUIRE(set_pair(m, 0, ramp, ramp, cr) == TM_OK && tm_mdsi_compute_async(m, 1) == TM_OK && m->c.pending);
    const long w2 = s.waits;
    REQUIRE(set(m, 0, TM_SIDE_REF, grey, cn, cn) == TM_OK && !m->c.pending && s.waits == w2 + 2); // the pending compute, then the upload
    REQUIRE(tm_mdsi_get(m, 0, 1, f) == TM_OK && tm_mdsi_get(m, 1, 1, f) == TM_ERR_STATE && f[0].dev > 0.0 && f[0].n == W * H);
    tm_mdsi_destroy(m);
    nothing_left();

    REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, TM_MDSI_BT601, 2, 0, 1) == TM_OK);
    REQUIRE(set_pair(m, 0, ramp, grey, cr) == TM_OK && tm_mdsi_compute_async(m, 1) == TM_OK);
    REQUIRE(tm_mdsi_map(m, 0, &map[0][0], sizeof map[0]) == TM_ERR_STATE); // created without TM_MDSI_MAPS
    REQUIRE(tm_mdsi_get(m, 0, 1, f + 1) == TM_OK && f[1].dev > 0.0 && f[1].factor == 2 && f[1].n == 4 * 3); // the forced factor
    tm_mdsi_destroy(m);
    nothing_left();
}

void test_argument_checks_and_host_functions()
{
    fake_hip::reset();
    tm_mdsi *m = (tm_mdsi *)&m;
    tm_mdsi_frame f;
    REQUIRE(tm_mdsi_create(nullptr, W, H, TM_MDSI_I420, 8, 0, 0, 0, 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, 0, 0, 0, 0) == TM_ERR_INVALID_ARG && m == nullptr);
    REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, 0, 0, 0, 65536) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, 3, 0, 0, 1) == TM_ERR_INVALID_ARG && tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, -1, 0, 0, 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, 0, 129, 0, 1) == TM_ERR_INVALID_ARG && tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, 0, 0, 2, 1) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 8, 0, 5, 0, 1) == TM_ERR_UNSUPPORTED && m == nullptr);  // 7 x 5 at f = 5: 2 x 1 positions, fewer than 4
    const uint32_t bad[][4] = {{1, 5, TM_MDSI_I420, 8}, {5, 1, TM_MDSI_I420, 8}, {32769, 8, TM_MDSI_I420, 8}, {8, 32769, TM_MDSI_I420, 8}, {7, 5, TM_MDSI_NV12, 10},
                               {7, 5, TM_MDSI_P016, 8}, {7, 5, TM_MDSI_I420, 17}, {7, 5, TM_MDSI_I420P10_PACKED, 12}, {7, 5, 4, 8}, {7, 5, TM_MDSI_I420, 7}};
    for (const auto &b : bad) REQUIRE(tm_mdsi_create(&m, b[0], b[1], (int)b[2], b[3], 0, 0, 0, 1) == TM_ERR_UNSUPPORTED && m == nullptr);
    REQUIRE(fake_hip::state().calls == 0);                                 // refused before any device call
    REQUIRE(tm_mdsi_create(&m, W, H, TM_MDSI_I420, 10, TM_MDSI_BY_HEIGHT, 0, 0, 2) == TM_OK);
    static unsigned short y[W * H + 1], c[CW * CH + 1];
    const size_t py = 2 * W, pc = 2 * CW;
    REQUIRE(tm_mdsi_set_frame(nullptr, 0, 0, y, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_mdsi_set_frame(m, 2, 0, y, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_set_frame(m, 0, 2, y, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_set_frame(m, 0, 0, nullptr, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_mdsi_set_frame(m, 0, 0, y, nullptr, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_set_frame(m, 0, 0, y, c, nullptr, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);                 // three planes are needed
    REQUIRE(tm_mdsi_set_frame(m, 0, 0, y, c, c, py, pc, 7) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_set_frame(m, 0, 0, y, c, c, py - 2, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG && tm_mdsi_set_frame(m, 0, 0, y, c, c, py, pc - 2, TM_MEM_HOST) == TM_ERR_INVALID_ARG); // pitch below a row
    REQUIRE(tm_mdsi_set_frame(m, 0, 0, (const char *)y + 1, c, c, py, pc, TM_MEM_HOST) == TM_ERR_INVALID_ARG);      // odd base of 16-bit samples
    REQUIRE(tm_mdsi_set_frame(m, 0, 0, y, c, c, py, pc + 1, TM_MEM_HOST) == TM_ERR_INVALID_ARG);                   // odd pitch
    REQUIRE(tm_mdsi_set_frame(m, 0, 0, y, c, c, py, pc, TM_MEM_DEVICE) == TM_OK && tm_mdsi_mem_usage(m) > 0);        // in place: no staging surface
    REQUIRE(fake_hip::state().dev_allocs == 5);
    REQUIRE(tm_mdsi_compute_async(nullptr, 1) == TM_ERR_INVALID_ARG && tm_mdsi_sync(nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_get(nullptr, 0, 1, &f) == TM_ERR_INVALID_ARG && tm_mdsi_get(m, 0, 1, nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_sync(m) == TM_OK);
    tm_mdsi_destroy(m);
    nothing_left();

    double o[3];
    REQUIRE(tm_mdsi_lhm(16, 128, 128, TM_MDSI_BT709, 7, o) == TM_ERR_UNSUPPORTED && tm_mdsi_lhm(16, 128, 128, TM_MDSI_BT709, 17, o) == TM_ERR_UNSUPPORTED);
    REQUIRE(tm_mdsi_lhm(16, 128, 128, TM_MDSI_BY_HEIGHT, 8, o) == TM_ERR_INVALID_ARG && tm_mdsi_lhm(16, 128, 128, -1, 8, o) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_lhm(16, 128, 128, TM_MDSI_BT709, 8, nullptr) == TM_ERR_INVALID_ARG);
    REQUIRE(tm_mdsi_lhm(16, 128, 128, TM_MDSI_BT601, 8, o) == TM_OK && o[0] == 0.0 && o[1] == 0.0 && o[2] == 0.0); // black
    REQUIRE(tm_mdsi_lhm(940, 512, 512, TM_MDSI_BT709, 10, o) == TM_OK && fabs(o[0] - 0.9999 * 255.0) < 1e-9 && fabs(o[1] + 0.01 * 255.0) < 1e-9 && fabs(o[2] + 0.09 * 255.0) < 1e-9);
    REQUIRE(tm_mdsi_factor(640, 641) == 3 && tm_mdsi_factor(639, 2000) == 2 && tm_mdsi_factor(384, 384) == 2 && tm_mdsi_factor(383, 383) == 1 &&
            tm_mdsi_factor(2, 2) == 1 && tm_mdsi_factor(896, 895) == 3 && tm_mdsi_factor(896, 896) == 4 && tm_mdsi_factor(32768, 32768) == 128);
    REQUIRE(std::isnan(tm_mdsi_score(1.0, 0)) && tm_mdsi_score(0.0, 4) == 0.0 && tm_mdsi_score(-1e-30, 4) == 0.0 && fabs(tm_mdsi_score(16.0 * 4, 4) - 2.0) < 1e-15);
}

} // namespace

int main()
{
    pictures();
    test_every_failure_position_of_create_and_set_frame();
    test_compute_get_map_and_state();
    test_argument_checks_and_host_functions();
    fake_hip::reset();
    printf("mdsi host ok\n");
    return 0;
}
