// tests/ciede_emul/ciede_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_ciede_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a grid
// run one after the other, and `__shared__` objects are statics that keep what the workgroup before left in them, as LDS does.  Drives
// computes the way the library does -- the cells, the maps and the results are allocated ONCE, filled with garbage, and reused by every
// compute, never cleared by the host -- so that indexing, edge, slot and stale-cell bugs are found against tests/ciede_ref.py without a
// GPU.  Every f32 operation is the kernel's own; powf, cbrtf, atan2f, expf, sinf and cosf are the host libm's.
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

#include "../../turbo-metrics_amd/csrc/tm_ciede_kernels.h"

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
        pthread_barrier_init(&g_bar, nullptr, TMC_THREADS);
        pthread_barrier_init(&start, nullptr, TMC_THREADS + 1);
        pthread_barrier_init(&done, nullptr, TMC_THREADS + 1);
        for (int t = 0; t < TMC_THREADS; ++t)
            th.emplace_back([this, t] {
                threadIdx = {(unsigned)t, 0, 0};
                blockDim = dim3(TMC_THREADS);
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
unsigned ce_desc_size() { return (unsigned)sizeof(TmCiedeDesc); }
// luma positions per tile edge: the tests build their sizes from them
unsigned ce_tile_w() { return TMC_TW; }
unsigned ce_tile_h() { return TMC_TH; }

// workgroups (= cells) per slot.  0, or -1 (refused)
int ce_geom(unsigned w, unsigned h, int layout, unsigned bits, unsigned long long *out)
{
    TmCiedeGeom g;
    if (tmc_make_geom(&g, w, h, layout, bits)) return -1;
    out[0] = g.cells;
    return 0;
}

// the device's dE00 of two Lab triples
float ce_de00(const float *lab1, const float *lab2, float kl, float kc, float kh)
{
    const tmc::Lab p = {lab1[0], lab1[1], lab1[2]}, q = {lab2[0], lab2[1], lab2[2]};
    return tmc::de00(p, q, kl, kc, kh);
}

// the device's Lab of one sample triple, through the kernel's own normalisation.  0, or -1 (refused)
int ce_lab(unsigned y, unsigned u, unsigned v, int matrix, unsigned bits, float *out)
{
    TmCiedeGeom g;
    if (tmc_make_geom(&g, 2, 2, bits == 8 ? TMC_I420 : TMC_I420, bits) || tmc_set_params(&g, matrix, 1, 1, 1)) return -1;
    const float un = (float)((int)u - g.coff) / g.cdiv, vn = (float)((int)v - g.coff) / g.cdiv, yn = (float)((int)y - g.yoff) / g.ydiv;
    const tmc::Lab p = tmc::lab_of(yn, g.c[0] * vn, g.c[1] * un, g.c[2] * vn, g.c[3] * un);
    out[0] = p.L; out[1] = p.a; out[2] = p.b;
    return 0;
}

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] pairs (two descriptors each:
// reference, distorted) as its slots 0 .. batches[c]-1.  Per pair, in the order of the descriptors: out_res[2 i] = the sum,
// out_res[2 i + 1] = the maximum; maps (or null): [pair][h][w].  force_vec: -1 = the library's rule (bases and pitches 16-byte
// aligned), 0 = the sample-by-sample path everywhere.  0, or -1 (refused)
int ce_run(unsigned w, unsigned h, int layout, unsigned bits, int matrix, double kl, double kc, double kh, unsigned cap, int ncomputes,
           const int *batches, TmCiedeDesc *desc, int force_vec, double *out_res, float *maps)
{
    TmCiedeGeom g;
    if (tmc_make_geom(&g, w, h, layout, bits) || tmc_set_params(&g, matrix, kl, kc, kh)) return -1;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<TmCiedeCell> cells((size_t)cap * g.cells), res(cap);
    std::vector<float> dmaps(maps ? (size_t)cap * w * h : 0);
    memset(cells.data(), 0xEE, cells.size() * sizeof(TmCiedeCell));
    memset(res.data(), 0xEE, cap * sizeof(TmCiedeCell));
    if (maps) memset(dmaps.data(), 0xEE, dmaps.size() * sizeof(float));
    Pool pool;
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -2;
        TmCiedeDesc *dd = desc + 2 * f0;
        for (unsigned i = 0; i < 2 * n; ++i) {
            TmCiedeDesc &d = dd[i];
            d.vec = force_vec < 0 ? (((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2) & 15) == 0 : force_vec;
        }
        float *dm = maps ? dmaps.data() : nullptr;
#define CE_LAUNCH(L, F) pool.launch(g.cells, n, [&] { k_ciede<L, F>(g, dd, dm, cells.data()); })
        TMC_DISPATCH(g, CE_LAUNCH);
#undef CE_LAUNCH
        pool.launch(n, 1, [&] { k_ciede_finish(g, cells.data(), res.data()); });
        for (unsigned i = 0; i < n; ++i) {
            out_res[2 * (f0 + i)] = res[i].sum; out_res[2 * (f0 + i) + 1] = (double)res[i].max;
            if (maps) memcpy(maps + (f0 + i) * (size_t)w * h, dmaps.data() + (size_t)i * w * h, (size_t)w * h * sizeof(float));
        }
        f0 += n;
    }
    return 0;
}
}
