// tests/adm_emul/adm_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_adm_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a
// grid run one after the other, the launches in the library's order (scales 0 .. 3, then the finish).  The restored, additive and
// threshold planes of every scale, which the product never writes, and the a bands are taken through TM_ADM_PLANE_HOOK and
// TM_ADM_THR_HOOK, so that indexing, mirror, halo and ordering bugs are found against tests/adm_ref.py without a GPU.
#define TM_EMULATE 1
#include "hip_emul.h"
#include <pthread.h>
#include <cstdlib>
#include <thread>
#include <vector>

thread_local uint3_ threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

static pthread_barrier_t g_bar; // the 256 lanes of the running workgroup
void tm_emul_syncthreads() { pthread_barrier_wait(&g_bar); }
void tm_emul_wave_barrier() { pthread_barrier_wait(&g_bar); }
void tm_emul_yield() { sched_yield(); }

bool tm_adm_block_sum6(double (&a)[6])
{
    static double buf[6][256];
    const unsigned t = threadIdx.x;
    for (int k = 0; k < 6; ++k) buf[k][t] = a[k];
    tm_emul_syncthreads();
    if (t == 0) {
        for (int k = 0; k < 6; ++k) {
            double x = 0.0;
            for (int i = 0; i < 256; ++i) x += buf[k][i];
            a[k] = x;
        }
    }
    tm_emul_syncthreads();
    return t == 0;
}

// where the planes of the running emulation go: [scale] -> float [9][bh_s][bw_s] of slot 0: r(h, v, d), a(h, v, d), thr, a_ref, a_dis
static float *g_planes[4];
static int g_pw[4], g_ph[4];
#define TM_ADM_PLANE_HOOK(scale, slot, x, y, r, a, a_ref, a_dis)                                        \
    do {                                                                                                \
        if (g_planes[scale] && (slot) == 0) {                                                           \
            const size_t n_ = (size_t)g_pw[scale] * g_ph[scale], i_ = (size_t)(y) * g_pw[scale] + (x);   \
            for (int b_ = 0; b_ < 3; ++b_) {                                                            \
                g_planes[scale][b_ * n_ + i_] = (r)[b_];                                                \
                g_planes[scale][(3 + b_) * n_ + i_] = (a)[b_];                                          \
            }                                                                                           \
            g_planes[scale][7 * n_ + i_] = (a_ref);                                                     \
            g_planes[scale][8 * n_ + i_] = (a_dis);                                                     \
        }                                                                                               \
    } while (0)
#define TM_ADM_THR_HOOK(scale, slot, x, y, thr)                                                         \
    do {                                                                                                \
        if (g_planes[scale] && (slot) == 0)                                                             \
            g_planes[scale][6 * (size_t)g_pw[scale] * g_ph[scale] + (size_t)(y) * g_pw[scale] + (x)] = (thr); \
    } while (0)

#include "../../turbo-metrics_amd/csrc/tm_adm_kernels.h"

namespace {
struct Launch {
    TmAdmGeom g;
    const TmAdmDesc *desc;
    float *pl;
    double *cell, *res;
    int stage; // 0 .. 3: k_adm of that scale; 4: k_adm_finish
};

void kernel(const Launch &L)
{
    switch (L.stage) {
    case 0:
        switch (L.g.fmt) {
        case TMX_F_U8: k_adm<TMX_F_U8, 0>(L.g, L.desc, L.pl, L.cell); break;
        case TMX_F_U16_MSB: k_adm<TMX_F_U16_MSB, 0>(L.g, L.desc, L.pl, L.cell); break;
        case TMX_F_U16_LOW: k_adm<TMX_F_U16_LOW, 0>(L.g, L.desc, L.pl, L.cell); break;
        default: k_adm<TMX_F_P10, 0>(L.g, L.desc, L.pl, L.cell); break;
        }
        break;
    case 1: k_adm<TMX_F_HIST, 1>(L.g, L.desc, L.pl, L.cell); break;
    case 2: k_adm<TMX_F_HIST, 2>(L.g, L.desc, L.pl, L.cell); break;
    case 3: k_adm<TMX_F_HIST, 3>(L.g, L.desc, L.pl, L.cell); break;
    default: k_adm_finish(L.g, L.cell, L.res); break;
    }
}

// the library's launches over one slot, block 256: 256 pool threads, one workgroup at a time
void run(Launch L)
{
    pthread_barrier_t start, done;
    pthread_barrier_init(&g_bar, nullptr, TMA_THREADS);
    pthread_barrier_init(&start, nullptr, TMA_THREADS + 1);
    pthread_barrier_init(&done, nullptr, TMA_THREADS + 1);
    volatile int job = 0, quit = 0;
    std::vector<std::thread> pool;
    for (int t = 0; t < TMA_THREADS; ++t)
        pool.emplace_back([&, t] {
            threadIdx = {(unsigned)t, 0, 0};
            blockDim = dim3(TMA_THREADS);
            for (;;) {
                pthread_barrier_wait(&start);
                if (quit) break;
                blockIdx = {(unsigned)job, 0, 0};
                kernel(L);
                pthread_barrier_wait(&done);
            }
        });
    for (int stage = 0; stage <= 4; ++stage) {
        L.stage = stage;
        const int grid = stage < 4 ? L.g.tiles[stage] : TMA_SCALES;
        for (int x = 0; x < grid; ++x) {
            job = x;
            pthread_barrier_wait(&start);
            pthread_barrier_wait(&done);
        }
    }
    quit = 1;
    pthread_barrier_wait(&start);
    for (auto &t : pool) t.join();
    pthread_barrier_destroy(&start);
    pthread_barrier_destroy(&done);
    pthread_barrier_destroy(&g_bar);
}
} // namespace

extern "C" {
unsigned ae_desc_size() { return (unsigned)sizeof(TmAdmDesc); }
// the tile of k_adm (band pixels of a scale): tests/geom_sweep.py builds its sizes from it
void ae_tile(int *out) { out[0] = TMA_TX; out[1] = TMA_TY; }

int ae_mirror(int p, int n) { return tma::mirror(p, n); }

void ae_filters(float *lo, float *hi)
{
    for (int k = 0; k < 4; ++k) { lo[k] = tma::lo(k); hi[k] = tma::hi(k); }
}

// the geometry of a pair: ws, hs, bws, bhs [4]; border [4][4] = left, top, right, bottom; rf [4][3]; 0, or -1 (unsupported)
int ae_geom(unsigned w, unsigned h, int layout, unsigned bits, int *ws, int *hs, int *bws, int *bhs, int *border, float *rf, float *cos2)
{
    TmAdmGeom g;
    if (tma_make_geom(&g, w, h, layout, bits)) return -1;
    for (int s = 0; s < 4; ++s) {
        ws[s] = g.w[s]; hs[s] = g.h[s]; bws[s] = g.bw[s]; bhs[s] = g.bh[s];
        border[4 * s] = g.left[s]; border[4 * s + 1] = g.top[s]; border[4 * s + 2] = g.right[s]; border[4 * s + 3] = g.bottom[s];
        for (int b = 0; b < 3; ++b) rf[3 * s + b] = g.rf[s][b];
    }
    *cos2 = g.cos2;
    return 0;
}

// one pair: sums[scale] = {N[h, v, d], Dn[h, v, d]}; planes[scale] (optional): float [9][bh_s][bw_s].  0, or -1 (unsupported)
int ae_pair(unsigned w, unsigned h, int layout, unsigned bits, TmAdmDesc *desc, double *sums, float **planes)
{
    TmAdmGeom g;
    if (tma_make_geom(&g, w, h, layout, bits)) return -1;
    for (int p = 0; p < 2; ++p) desc->vec[p] = (((uintptr_t)desc->p[p] | desc->pitch[p]) & 15) == 0;
    for (int s = 0; s < 4; ++s) {
        g_planes[s] = planes ? planes[s] : nullptr;
        g_pw[s] = g.bw[s];
        g_ph[s] = g.bh[s];
    }
    std::vector<float> pl((size_t)g.pslot + 8, -12345.0f); // undefined on the device: never read before it is written
    float *base = (float *)(((uintptr_t)pl.data() + 15) & ~(uintptr_t)15);
    std::vector<double> cell((size_t)g.cells * 6, -1.0), res(TMA_SCALES * 6, -1.0);
    run(Launch{g, desc, base, cell.data(), res.data(), 0});
    memcpy(sums, res.data(), sizeof(double) * TMA_SCALES * 6);
    for (int s = 0; s < 4; ++s) g_planes[s] = nullptr;
    return 0;
}
}
