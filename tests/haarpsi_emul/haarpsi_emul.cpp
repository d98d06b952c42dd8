// tests/haarpsi_emul/haarpsi_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_haarpsi_kernels.h on the
// CPU.  A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a
// grid run one after the other, and `__shared__` objects are statics that keep what the workgroup before left in them, as LDS does.
// Drives computes the way the library does -- the cells, the maps and the results are allocated ONCE, filled with garbage, and reused by
// every compute, never cleared by the host -- so that indexing, edge, slot and stale-cell bugs are found against tests/haarpsi_ref.py
// without a GPU.  The integer arithmetic, the conversions and every f32 operation (the exponential included: fmaf, conversions and
// multiplications only) are the kernel's own.
#define TM_EMULATE 1
#include "hip_emul.h"
#include <pthread.h>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

thread_local uint3_ threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

static pthread_barrier_t g_bar; // the 256 lanes of the running workgroup
void tm_emul_syncthreads() { pthread_barrier_wait(&g_bar); }
void tm_emul_wave_barrier() { pthread_barrier_wait(&g_bar); }
void tm_emul_yield() { sched_yield(); }

#include "../../turbo-metrics_amd/csrc/tm_haarpsi_kernels.h"

namespace {

// 256 pool threads, one workgroup at a time
struct Pool {
    pthread_barrier_t start, done;
    volatile unsigned jx = 0, jy = 0, gx = 1, gy = 1;
    volatile int quit = 0;
    std::function<void()> body;
    std::vector<std::thread> th;
    Pool()
    {
        pthread_barrier_init(&g_bar, nullptr, TMP_THREADS);
        pthread_barrier_init(&start, nullptr, TMP_THREADS + 1);
        pthread_barrier_init(&done, nullptr, TMP_THREADS + 1);
        for (int t = 0; t < TMP_THREADS; ++t)
            th.emplace_back([this, t] {
                threadIdx = {(unsigned)t, 0, 0};
                blockDim = dim3(TMP_THREADS);
                for (;;) {
                    pthread_barrier_wait(&start);
                    if (quit) break;
                    blockIdx = {jx, jy, 0};
                    gridDim = dim3(gx, gy);
                    body();
                    pthread_barrier_wait(&done);
                }
            });
    }
    void launch(unsigned nx, unsigned ny, std::function<void()> f)
    {
        body = std::move(f);
        gx = nx; gy = ny;
        for (unsigned y = 0; y < ny; ++y)
            for (unsigned x = 0; x < nx; ++x) {
                jx = x; jy = y;
                pthread_barrier_wait(&start);
                pthread_barrier_wait(&done);
            }
    }
    ~Pool()
    {
        quit = 1;
        pthread_barrier_wait(&start);
        for (auto &t : th) t.join();
        pthread_barrier_destroy(&start);
        pthread_barrier_destroy(&done);
        pthread_barrier_destroy(&g_bar);
    }
};

} // namespace

extern "C" {
unsigned he_desc_size() { return (unsigned)sizeof(TmHaarpsiDesc); }
// decimated positions per tile edge: the tests build their sizes from them
unsigned he_tile_w() { return TMP_TW; }
unsigned he_tile_h() { return TMP_TH; }

// out[0 .. 5] = w2, h2, workgroups (= cells) per slot, C_1, C_2, whether maps are kept.  0, or -1 (refused)
int he_geom(unsigned w, unsigned h, int layout, unsigned bits, int maps, unsigned long long *out)
{
    TmHaarpsiGeom g;
    if (tmp_make_geom(&g, w, h, layout, bits, maps)) return -1;
    out[0] = g.w2; out[1] = g.h2; out[2] = g.cells; out[3] = g.c[0]; out[4] = g.c[1]; out[5] = (unsigned long long)g.maps;
    return 0;
}

// the kernel's f32 pieces of a position and orientation
float he_e_of(int hr, int hd, unsigned long long c) { return tmp::e_of(hr, hd, c); }
float he_exp_pos(float z) { return tmp::exp_pos(z); }
float he_q_of(float s) { return tmp::q_of(s); }
float he_alpha() { return TMP_A; }

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] descriptors as its slots
// 0 .. batches[c]-1.  Per pair, in the order of the descriptors: out_q[i] = Q, out_ws[i] = WS; with out_maps, pair i's map goes to
// out_maps + i * w2 * h2.  force_vec: -1 = the library's rule (bases and pitches 16-byte aligned), 0 = the sample-by-sample path
// everywhere.  0, or -1 (refused)
int he_run(unsigned w, unsigned h, int layout, unsigned bits, unsigned cap, int ncomputes, const int *batches, TmHaarpsiDesc *desc, int force_vec,
           double *out_q, unsigned long long *out_ws, float *out_maps)
{
    TmHaarpsiGeom g;
    if (tmp_make_geom(&g, w, h, layout, bits, out_maps != nullptr)) return -1;
    const size_t npos = (size_t)g.w2 * g.h2;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<TmHaarpsiCell> cells((size_t)cap * g.cells), res(cap);
    std::vector<float> maps(g.maps ? cap * npos : 0);
    memset(cells.data(), 0xEE, cells.size() * sizeof(TmHaarpsiCell));
    memset(res.data(), 0xEE, cap * sizeof(TmHaarpsiCell));
    if (g.maps) memset(maps.data(), 0xEE, maps.size() * sizeof(float));
    Pool pool;
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -2;
        TmHaarpsiDesc *dd = desc + f0;
        for (unsigned i = 0; i < n; ++i) {
            TmHaarpsiDesc &d = dd[i];
            d.vec = force_vec < 0 ? (((uintptr_t)d.p[0] | (uintptr_t)d.p[1] | d.pitch[0] | d.pitch[1]) & 15) == 0 : force_vec;
        }
#define HE_LAUNCH(F) pool.launch(g.cells, n, [&] { k_haarpsi<F>(g, dd, g.maps ? maps.data() : nullptr, cells.data()); })
        TMP_DISPATCH(g, HE_LAUNCH);
#undef HE_LAUNCH
        pool.launch(n, 1, [&] { k_haarpsi_finish(g, cells.data(), res.data()); });
        for (unsigned i = 0; i < n; ++i) {
            out_q[f0 + i] = res[i].q; out_ws[f0 + i] = res[i].ws;
            if (g.maps) memcpy(out_maps + (f0 + i) * npos, maps.data() + i * npos, npos * sizeof(float));
        }
        f0 += n;
    }
    return 0;
}
}
