// tests/vif_emul/vif_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_vif_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a
// grid run one after the other, the launches in the library's order (scales 0 .. 3, then the finish).  The three integer planes
// of every scale, which the product never writes, are taken through TM_VIF_PLANE_HOOK, so that indexing, mirror, halo, rounding and
// decimation bugs are found against tests/vif_ref.py without a GPU.
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

bool tm_vif_block_sum2(double &a, double &b)
{
    static double buf[2][256];
    const unsigned t = threadIdx.x;
    buf[0][t] = a;
    buf[1][t] = b;
    tm_emul_syncthreads();
    if (t == 0) {
        double x = 0.0, y = 0.0;
        for (int i = 0; i < 256; ++i) { x += buf[0][i]; y += buf[1][i]; }
        a = x;
        b = y;
    }
    tm_emul_syncthreads();
    return t == 0;
}

// where the planes of the running emulation go: [scale] -> int32 [3][h_s][w_s] of slot 0
static int *g_planes[4];
static int g_pw[4], g_ph[4];
#define TM_VIF_PLANE_HOOK(scale, slot, x, y, s1, s2, s12)                                  \
    do {                                                                                  \
        if (g_planes[scale] && (slot) == 0) {                                             \
            const size_t n_ = (size_t)g_pw[scale] * g_ph[scale], i_ = (size_t)(y) * g_pw[scale] + (x); \
            g_planes[scale][i_] = (s1);                                                   \
            g_planes[scale][n_ + i_] = (s2);                                              \
            g_planes[scale][2 * n_ + i_] = (s12);                                         \
        }                                                                                 \
    } while (0)

#include "../../turbo-metrics_amd/csrc/tm_vif_kernels.h"

namespace {
struct Launch {
    TmVifGeom g;
    const TmVifDesc *desc;
    unsigned short *pl;
    double *cell, *res;
    int stage; // 0 .. 3: k_vif of that scale; 4: k_vif_finish
};

void kernel(const Launch &L)
{
    switch (L.stage) {
    case 0:
        switch (L.g.fmt) {
        case TMX_F_U8: k_vif<TMX_F_U8, 0>(L.g, L.desc, L.pl, L.cell); break;
        case TMX_F_U16_MSB: k_vif<TMX_F_U16_MSB, 0>(L.g, L.desc, L.pl, L.cell); break;
        case TMX_F_U16_LOW: k_vif<TMX_F_U16_LOW, 0>(L.g, L.desc, L.pl, L.cell); break;
        default: k_vif<TMX_F_P10, 0>(L.g, L.desc, L.pl, L.cell); break;
        }
        break;
    case 1: k_vif<TMX_F_HIST, 1>(L.g, L.desc, L.pl, L.cell); break;
    case 2: k_vif<TMX_F_HIST, 2>(L.g, L.desc, L.pl, L.cell); break;
    case 3: k_vif<TMX_F_HIST, 3>(L.g, L.desc, L.pl, L.cell); break;
    default: k_vif_finish(L.g, L.cell, L.res); break;
    }
}

// the library's launches over one slot, block 256: 256 pool threads, one workgroup at a time
void run(Launch L)
{
    pthread_barrier_t start, done;
    pthread_barrier_init(&g_bar, nullptr, TMV_THREADS);
    pthread_barrier_init(&start, nullptr, TMV_THREADS + 1);
    pthread_barrier_init(&done, nullptr, TMV_THREADS + 1);
    volatile int job = 0, quit = 0;
    std::vector<std::thread> pool;
    for (int t = 0; t < TMV_THREADS; ++t)
        pool.emplace_back([&, t] {
            threadIdx = {(unsigned)t, 0, 0};
            blockDim = dim3(TMV_THREADS);
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
        const int grid = stage < 4 ? L.g.tiles[stage] : TMV_SCALES;
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
unsigned ve_desc_size() { return (unsigned)sizeof(TmVifDesc); }
// the tile of k_vif (pixels of a scale): tests/geom_sweep.py builds its sizes from it
void ve_tile(int *out) { out[0] = TMV_TW; out[1] = TMV_TH; }

// taps of filter s into out[17]; returns their number
int ve_filter(int s, unsigned *out)
{
    const int n = tmv::ntaps(s);
    for (int k = 0; k < n; ++k) out[k] = tmv::coef(s, k);
    return n;
}

int ve_mirror(int i, int n) { return tmv::mirror(i, n); }

// w[4], h[4] of the scales; 0, or -1 (unsupported geometry)
int ve_sizes(unsigned w, unsigned h, int layout, unsigned bits, int *ws, int *hs)
{
    TmVifGeom g;
    if (tmv_make_geom(&g, w, h, layout, bits)) return -1;
    for (int s = 0; s < 4; ++s) { ws[s] = g.w[s]; hs[s] = g.h[s]; }
    return 0;
}

// one pair: numden[scale] = {num, den}; planes[scale] (optional): int32 [3][h_s][w_s].  0, or -1 (unsupported geometry)
int ve_pair(unsigned w, unsigned h, int layout, unsigned bits, TmVifDesc *desc, double *numden, int **planes)
{
    TmVifGeom g;
    if (tmv_make_geom(&g, w, h, layout, bits)) return -1;
    for (int p = 0; p < 2; ++p) desc->vec[p] = (((uintptr_t)desc->p[p] | desc->pitch[p]) & 15) == 0;
    for (int s = 0; s < 4; ++s) {
        g_planes[s] = planes ? planes[s] : nullptr;
        g_pw[s] = g.w[s];
        g_ph[s] = g.h[s];
    }
    std::vector<unsigned short> pl((size_t)g.pslot + 8, 0xABCD); // undefined on the device: never read before it is written
    unsigned short *base = (unsigned short *)(((uintptr_t)pl.data() + 15) & ~(uintptr_t)15);
    std::vector<double> cell((size_t)g.cells * 2, -1.0), res(TMV_SCALES * 2, -1.0);
    run(Launch{g, desc, base, cell.data(), res.data(), 0});
    memcpy(numden, res.data(), sizeof(double) * TMV_SCALES * 2);
    for (int s = 0; s < 4; ++s) g_planes[s] = nullptr;
    return 0;
}
}
