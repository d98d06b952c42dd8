// turbo_metrics.cpp -- see turbo_metrics.hpp.  Host orchestration only: frame selection, batching over the engine's
// slots, ping-pong pipelining of two engines; every number comes out of libturbometrics_hip.so.
#include "turbo_metrics.hpp"
#include "../../include/turbo_metrics_xpsnr.h"
#include "../../include/turbo_metrics_motion.h"
#include "../../include/turbo_metrics_scene.h"
#include "../../include/turbo_metrics_siti.h"
#include "../../include/turbo_metrics_cambi.h"
#include "../../include/turbo_metrics_flip.h"
#include "../../include/turbo_metrics_yuv.h"
#include "../../include/turbo_metrics_hvs.h"
#include "../../include/turbo_metrics_gmsd.h"
#include "../../include/turbo_metrics_haarpsi.h"
#include "../../include/turbo_metrics_itp.h"
#include "../../include/turbo_metrics_mdsi.h"
#include "../../include/turbo_metrics_ciede.h"
#include "frame_sources.hpp" // write_pfm_gray
#include "../../include/turbo_metrics_vif.h"
#include "../../include/turbo_metrics_adm.h"
#include <dlfcn.h>
#include <array>
#include <cmath>
#include <deque>
#include <chrono>
#include <fstream>
#include <sched.h>
#include <string>

#include <condition_variable>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>
#include <unistd.h>

namespace tm_host {

TmError::TmError(int c, const std::string &where)
    : std::runtime_error(where + ": " + tm_strerror(c) + (c == TM_ERR_HIP ? std::string(" [") + tm_last_hip_error() + "]" : std::string())),
      code(c)
{
}

static void chk(int code, const char *where)
{
    if (code != TM_OK) throw TmError(code, where);
}

// The calling thread (and every thread it starts afterwards: the sources' readers, the ring helper, the fetch helper) is bound to the CPUs
// of the NUMA node next to the device.  Frames are copied from the page cache into page-locked memory that the runtime places on that
// node and are then read by the device's copy engines through that socket: from the other socket the same CLI run delivers 4.3-4.9 k
// pairs/s of 1080p instead of 6.6-7.4 k, and left to the scheduler it lands in between and differs from box to box
// (tools/numa_probe.sh, profiles/r04y_numa_probe.log).  TM_NUMA_BIND=0 leaves the affinity alone; nothing happens when the node is
// unknown or the process may not run on any of its CPUs.
static void bind_to_device_node(int device)
{
    const char *env = getenv("TM_NUMA_BIND");
    if (env && atoi(env) == 0) return;
    const int node = tm_device_numa_node(device);
    if (node < 0) return;
    std::ifstream f("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist");
    std::string list;
    if (!(f >> list)) return;
    // The mask the PROCESS was started with, taken once before the first bind: with --devices N the main thread is bound to device 0's
    // node before the shard threads start, they inherit that narrowed mask, and a device on the other socket would intersect to nothing
    // and stay on device 0's CPUs.
    static cpu_set_t original;
    static std::once_flag once;
    static bool have_original = false;
    std::call_once(once, [] { have_original = sched_getaffinity(getpid(), sizeof original, &original) == 0; });
    if (!have_original) return;
    cpu_set_t now = original, want;
    CPU_ZERO(&want);
    int n = 0;
    for (size_t i = 0; i < list.size();) { // "0-63,128-191"
        char *end = nullptr;
        const long lo = strtol(list.c_str() + i, &end, 10);
        long hi = lo;
        if (end && *end == '-') hi = strtol(end + 1, &end, 10);
        if (!end || lo < 0 || hi < lo) return;
        for (long c = lo; c <= hi && c < CPU_SETSIZE; ++c)
            if (CPU_ISSET((int)c, &now)) { CPU_SET((int)c, &want); ++n; }
        i = (size_t)(end - list.c_str());
        if (i < list.size() && list[i] == ',') ++i; else break;
    }
    if (n > 0 && n < CPU_COUNT(&now)) (void)sched_setaffinity(0, sizeof want, &want);
}

void init_hip(int device)
{
    chk(tm_init(device), "tm_init");
    bind_to_device_node(device);
}

// ---- colour metadata ---------------------------------------------------------------------------------------------
ColorCharacteristics ColorCharacteristics::from_codes(int cp, int mc, int tc)
{
    ColorCharacteristics c;
    switch (cp) {
    case 1: c.cp = ColourPrimaries::BT709; break;
    case 2: c.cp = ColourPrimaries::Unspecified; break;
    case 5: c.cp = ColourPrimaries::BT601_625; break;
    case 6: c.cp = ColourPrimaries::BT601_525; break;
    case 0: case 3: c.cp = ColourPrimaries::Invalid; break;
    default: c.cp = ColourPrimaries::Unsupported; break;
    }
    switch (mc) {
    case 1: c.mc = MatrixCoefficients::BT709; break;
    case 2: c.mc = MatrixCoefficients::Unspecified; break;
    case 5: c.mc = MatrixCoefficients::BT601_625; break;
    case 6: c.mc = MatrixCoefficients::BT601_525; break;
    case 3: c.mc = MatrixCoefficients::Invalid; break;
    default: c.mc = MatrixCoefficients::Unsupported; break; // 0 = identity, 4 = FCC, ...
    }
    switch (tc) {
    case 1: case 6: c.tc = TransferCharacteristic::BT709; break;
    case 2: c.tc = TransferCharacteristic::Unspecified; break;
    case 0: case 3: c.tc = TransferCharacteristic::Invalid; break;
    default: c.tc = TransferCharacteristic::Unsupported; break;
    }
    return c;
}

ColorCharacteristics ColorCharacteristics::or_(const ColorCharacteristics &o) const
{
    ColorCharacteristics r = *this;
    if (cp == ColourPrimaries::Unspecified || cp == ColourPrimaries::Invalid) r.cp = o.cp;
    if (mc == MatrixCoefficients::Unspecified || mc == MatrixCoefficients::Invalid) r.mc = o.mc;
    if (tc == TransferCharacteristic::Unspecified || tc == TransferCharacteristic::Invalid) r.tc = o.tc;
    return r;
}

ColorCharacteristics color_characteristics_fallback(uint32_t height)
{
    ColorCharacteristics c;
    c.tc = TransferCharacteristic::BT709;
    if (height <= 525) { c.cp = ColourPrimaries::BT601_525; c.mc = MatrixCoefficients::BT601_525; }
    else if (height <= 625) { c.cp = ColourPrimaries::BT601_625; c.mc = MatrixCoefficients::BT601_625; }
    else { c.cp = ColourPrimaries::BT709; c.mc = MatrixCoefficients::BT709; }
    return c;
}

int get_color_matrix(const ColorCharacteristics &c)
{
    if (c.cp == ColourPrimaries::BT709 && c.mc == MatrixCoefficients::BT709) return TM_MATRIX_BT709;
    if (c.cp == ColourPrimaries::BT601_525 && c.mc == MatrixCoefficients::BT601_525) return TM_MATRIX_BT601_525;
    if (c.cp == ColourPrimaries::BT601_625 && c.mc == MatrixCoefficients::BT601_625) return TM_MATRIX_BT601_625;
    throw std::runtime_error(std::string("not implemented: colour primaries ") + to_string(c.cp) + " with matrix coefficients " +
                             to_string(c.mc) + " (todo!() in the reference, turbo-metrics/src/color.rs:85)");
}

int get_transfer(const ColorCharacteristics &c)
{
    if (c.tc == TransferCharacteristic::BT709) return TM_TRANSFER_BT709;
    throw std::runtime_error(std::string("not implemented: transfer characteristic ") + to_string(c.tc) +
                             " (todo!() in the reference, turbo-metrics/src/color.rs:92)");
}

const char *to_string(ColourPrimaries v)
{
    switch (v) {
    case ColourPrimaries::Invalid: return "Invalid";
    case ColourPrimaries::Unspecified: return "Unspecified";
    case ColourPrimaries::Unsupported: return "Unsupported";
    case ColourPrimaries::BT709: return "BT709";
    case ColourPrimaries::BT601_525: return "BT601_525";
    default: return "BT601_625";
    }
}
const char *to_string(MatrixCoefficients v)
{
    switch (v) {
    case MatrixCoefficients::Invalid: return "Invalid";
    case MatrixCoefficients::Unspecified: return "Unspecified";
    case MatrixCoefficients::Unsupported: return "Unsupported";
    case MatrixCoefficients::BT709: return "BT709";
    case MatrixCoefficients::BT601_525: return "BT601_525";
    default: return "BT601_625";
    }
}
const char *to_string(TransferCharacteristic v)
{
    switch (v) {
    case TransferCharacteristic::Invalid: return "Invalid";
    case TransferCharacteristic::Unspecified: return "Unspecified";
    case TransferCharacteristic::Unsupported: return "Unsupported";
    default: return "BT709";
    }
}
const char *to_string(ColorRange v) { return v == ColorRange::Full ? "Full" : "Limited"; }

// ---- XPSNR ---------------------------------------------------------------------------------------------------------
// libturbometrics_xpsnr.so, loaded at run time (a CLI run without -m xpsnr never loads it; the host archive has no link dependency on
// it).  Pairs are handed over as TM_MEM_HOST copies -- done before set_frame returns, so the sources' rings of page-locked surfaces and
// the engine's upload fences are untouched -- and computed batch by batch in stream order; results wait in `ready` until the engine's
// scores of the same pairs are drained.
struct XpsnrRun {
    void *lib = nullptr;
    int (*create)(tm_xpsnr **, uint32_t, uint32_t, int, uint32_t, uint32_t, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_xpsnr *) = nullptr;
    int (*set_frame)(tm_xpsnr *, uint32_t, int, const void *, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_xpsnr *, uint32_t) = nullptr;
    int (*sync)(tm_xpsnr *) = nullptr;
    int (*get)(tm_xpsnr *, uint32_t, uint32_t, tm_xpsnr_frame *) = nullptr;
    double (*sequence)(double, double, uint64_t, uint32_t, uint32_t, uint32_t) = nullptr;
    tm_xpsnr *x = nullptr;
    uint32_t w, h, batch, fps_num = 25, fps_den = 1; // ffmpeg's rawvideo default of 25 fps when nothing else is known
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    std::deque<std::array<double, 3>> ready;
    double sum_sqrt[3] = {0, 0, 0}, sum_x[3] = {0, 0, 0};
    uint64_t frames = 0;

    XpsnrRun(uint32_t w_, uint32_t h_, uint32_t batch_) : w(w_), h(h_), batch(batch_)
    {
        const char *path = getenv("TM_XPSNR_LIB");
        lib = dlopen(path ? path : "libturbometrics_xpsnr.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m xpsnr needs libturbometrics_xpsnr.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_xpsnr_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_xpsnr_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_xpsnr_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_xpsnr_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_xpsnr_sync");
        get = (decltype(get))dlsym(lib, "tm_xpsnr_get");
        sequence = (decltype(sequence))dlsym(lib, "tm_xpsnr_sequence");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !sequence)
            throw std::runtime_error("libturbometrics_xpsnr.so does not export include/turbo_metrics_xpsnr.h");
    }
    ~XpsnrRun()
    {
        if (x) destroy(x);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &layout, uint32_t &bits)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: layout = TM_XPSNR_NV12; bits = 8; return;
        case HwFrame::NvDecP016: layout = TM_XPSNR_P016; bits = 10; return;
        case HwFrame::Planar420: layout = TM_XPSNR_I420; bits = (uint32_t)f.bits; return;
        case HwFrame::Planar420P10: layout = TM_XPSNR_I420P10_PACKED; bits = 10; return;
        default: throw std::runtime_error("xpsnr needs 4:2:0 YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    void push(const HwFrame &r, const HwFrame &d)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd) throw std::runtime_error("xpsnr needs reference and distorted in the same YUV layout and bit depth");
        if (!x) {
            layout = lr; bits = br;
            chk(create(&x, w, h, layout, bits, fps_num, fps_den, batch), "tm_xpsnr_create");
        } else if (lr != layout || br != bits) {
            throw std::runtime_error("xpsnr: the YUV layout changed inside the stream");
        }
        const bool bi = layout == TM_XPSNR_NV12 || layout == TM_XPSNR_P016;
        int side = TM_SIDE_REF;
        for (const HwFrame *f : {&r, &d}) {
            chk(set_frame(x, filled, side, f->data, bi ? f->uv : f->u, bi ? nullptr : f->v, f->pitch, bi ? f->pitch : f->pitch_uv,
                          f->device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_xpsnr_set_frame");
            side = TM_SIDE_DIS;
        }
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(x, filled), "tm_xpsnr_compute_async");
        chk(sync(x), "tm_xpsnr_sync");
        std::vector<tm_xpsnr_frame> out(filled);
        chk(get(x, 0, filled, out.data()), "tm_xpsnr_get");
        for (const tm_xpsnr_frame &f : out) {
            for (int c = 0; c < 3; ++c) { sum_sqrt[c] += sqrt((double)f.wsse[c]); sum_x[c] += f.xpsnr[c]; }
            ready.push_back({f.xpsnr[0], f.xpsnr[1], f.xpsnr[2]});
            ++frames;
        }
        filled = 0;
    }
    std::array<double, 3> pop()
    {
        if (ready.empty()) throw std::logic_error("xpsnr: a pair's result is missing");
        const std::array<double, 3> v = ready.front();
        ready.pop_front();
        return v;
    }
    double sequence_score(int c) const
    {
        const uint32_t pw = c ? (w + 1) / 2 : w, ph = c ? (h + 1) / 2 : h;
        return sequence(sum_sqrt[c], sum_x[c], frames, pw, ph, bits);
    }
};

// ---- motion --------------------------------------------------------------------------------------------------------
// libturbometrics_motion.so, loaded at run time like the XPSNR library (a CLI run without --motion never loads it).  The REFERENCE
// picture of every kept pair is handed over as a TM_MEM_HOST copy and computed batch by batch in stream order; a picture's motion
// waits in `ready` until the engine's scores of the same pair are drained.
struct MotionRun {
    void *lib = nullptr;
    int (*create)(tm_motion **, uint32_t, uint32_t, int, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_motion *) = nullptr;
    int (*set_frame)(tm_motion *, uint32_t, const void *, size_t, int) = nullptr;
    int (*compute_async)(tm_motion *, uint32_t) = nullptr;
    int (*sync)(tm_motion *) = nullptr;
    int (*get)(tm_motion *, uint32_t, uint32_t, tm_motion_frame *) = nullptr;
    double (*motion2)(double, double) = nullptr;
    tm_motion *m = nullptr;
    uint32_t w, h, batch;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    std::deque<double> ready;

    MotionRun(uint32_t w_, uint32_t h_, uint32_t batch_) : w(w_), h(h_), batch(batch_)
    {
        const char *path = getenv("TM_MOTION_LIB");
        lib = dlopen(path ? path : "libturbometrics_motion.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("--motion needs libturbometrics_motion.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_motion_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_motion_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_motion_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_motion_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_motion_sync");
        get = (decltype(get))dlsym(lib, "tm_motion_get");
        motion2 = (decltype(motion2))dlsym(lib, "tm_motion2");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !motion2)
            throw std::runtime_error("libturbometrics_motion.so does not export include/turbo_metrics_motion.h");
    }
    ~MotionRun()
    {
        if (m) destroy(m);
        if (lib) dlclose(lib);
    }
    void push(const HwFrame &r)
    {
        int l;
        uint32_t b;
        switch (r.kind) {
        case HwFrame::NvDecNV12: l = TM_MOTION_Y8; b = 8; break;
        case HwFrame::NvDecP016: l = TM_MOTION_Y16_MSB; b = 10; break;
        case HwFrame::Planar420: b = (uint32_t)r.bits; l = b == 8 ? TM_MOTION_Y8 : TM_MOTION_Y16_LOW; break;
        case HwFrame::Planar420P10: l = TM_MOTION_Y10_PACKED; b = 10; break;
        default: throw std::runtime_error("motion needs YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
        if (!m) {
            layout = l; bits = b;
            chk(create(&m, w, h, layout, bits, batch), "tm_motion_create");
        } else if (l != layout || b != bits) {
            throw std::runtime_error("motion: the YUV layout changed inside the stream");
        }
        chk(set_frame(m, filled, r.data, r.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_motion_set_frame");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(m, filled), "tm_motion_compute_async");
        chk(sync(m), "tm_motion_sync");
        std::vector<tm_motion_frame> out(filled);
        chk(get(m, 0, filled, out.data()), "tm_motion_get");
        for (const tm_motion_frame &f : out) ready.push_back(f.motion);
        filled = 0;
    }
    double pop()
    {
        if (ready.empty()) throw std::logic_error("motion: a picture's result is missing");
        const double v = ready.front();
        ready.pop_front();
        return v;
    }
};

// ---- SI / TI ---------------------------------------------------------------------------------------------------------
// libturbometrics_siti.so, loaded at run time like the motion library (a CLI run without --siti never loads it).  The REFERENCE luma of
// every kept pair is handed over as a TM_MEM_HOST copy and computed batch by batch in stream order; the library keeps the previous
// picture.  SI and TI at the chosen gain are the library's host functions of the exact sums: nothing here restates the definition.
struct SitiRun {
    struct Value { double si, ti; bool ti_valid; };
    void *lib = nullptr;
    int (*create)(tm_siti **, uint32_t, uint32_t, int, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_siti *) = nullptr;
    int (*set_frame)(tm_siti *, uint32_t, const void *, size_t, int) = nullptr;
    int (*compute_async)(tm_siti *, uint32_t) = nullptr;
    int (*sync)(tm_siti *) = nullptr;
    int (*get)(tm_siti *, uint32_t, uint32_t, tm_siti_frame *) = nullptr;
    double (*si_of)(uint64_t, uint64_t, uint64_t, double) = nullptr;
    double (*ti_of)(int64_t, uint64_t, uint64_t, uint32_t, double) = nullptr;
    tm_siti *m = nullptr;
    uint32_t w, h, batch;
    double gain;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    std::deque<Value> ready;

    SitiRun(uint32_t w_, uint32_t h_, uint32_t batch_, double gain_) : w(w_), h(h_), batch(batch_), gain(gain_)
    {
        const char *path = getenv("TM_SITI_LIB");
        lib = dlopen(path ? path : "libturbometrics_siti.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("--siti needs libturbometrics_siti.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_siti_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_siti_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_siti_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_siti_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_siti_sync");
        get = (decltype(get))dlsym(lib, "tm_siti_get");
        si_of = (decltype(si_of))dlsym(lib, "tm_siti_si");
        ti_of = (decltype(ti_of))dlsym(lib, "tm_siti_ti");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !si_of || !ti_of)
            throw std::runtime_error("libturbometrics_siti.so does not export include/turbo_metrics_siti.h");
    }
    ~SitiRun()
    {
        if (m) destroy(m);
        if (lib) dlclose(lib);
    }
    void push(const HwFrame &r)
    {
        int l;
        uint32_t b;
        switch (r.kind) {
        case HwFrame::NvDecNV12: l = TM_SITI_Y8; b = 8; break;
        case HwFrame::NvDecP016: l = TM_SITI_Y16_MSB; b = 10; break;
        case HwFrame::Planar420: b = (uint32_t)r.bits; l = b == 8 ? TM_SITI_Y8 : TM_SITI_Y16_LOW; break;
        case HwFrame::Planar420P10: l = TM_SITI_Y10_PACKED; b = 10; break;
        default: throw std::runtime_error("siti needs YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
        if (!m) {
            layout = l; bits = b;
            chk(create(&m, w, h, layout, bits, batch), "tm_siti_create");
        } else if (l != layout || b != bits) {
            throw std::runtime_error("siti: the YUV layout changed inside the stream");
        }
        chk(set_frame(m, filled, r.data, r.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_siti_set_frame");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(m, filled), "tm_siti_compute_async");
        chk(sync(m), "tm_siti_sync");
        std::vector<tm_siti_frame> out(filled);
        chk(get(m, 0, filled, out.data()), "tm_siti_get");
        const uint64_t n = (uint64_t)w * h, n_si = (uint64_t)(w - 2) * (h - 2);
        for (const tm_siti_frame &f : out)
            ready.push_back({si_of(f.s1, f.s2, n_si, gain), f.ti_valid ? ti_of(f.t1, f.t2, n, bits, gain) : 0.0, f.ti_valid != 0});
        filled = 0;
    }
    Value pop()
    {
        if (ready.empty()) throw std::logic_error("siti: a picture's result is missing");
        const Value v = ready.front();
        ready.pop_front();
        return v;
    }
};

// ---- scene cuts ------------------------------------------------------------------------------------------------------
// libturbometrics_scene.so, loaded at run time like the motion library (a CLI run without --scenes never loads it).  The REFERENCE
// luma of every kept pair is handed over as a TM_MEM_HOST copy and its histogram computed batch by batch in stream order; the
// previous kept picture's histogram stays here, on the host, across batches.  The verdict is the library's host functions: nothing
// here restates the definition.  A picture's {score, cut} waits in `ready` until the engine's scores of the same pair are drained.
// No device history: --every is fine (the score is then that against the previous KEPT picture).
struct SceneRun {
    void *lib = nullptr;
    int (*create)(tm_scene **, uint32_t, uint32_t, int, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_scene *) = nullptr;
    int (*set_frame)(tm_scene *, uint32_t, const void *, size_t, int) = nullptr;
    int (*compute_async)(tm_scene *, uint32_t) = nullptr;
    int (*sync)(tm_scene *) = nullptr;
    int (*get)(tm_scene *, uint32_t, uint32_t, tm_scene_frame *) = nullptr;
    int (*distance)(const uint32_t *, const uint32_t *, int, uint64_t *) = nullptr;
    double (*score)(uint64_t, uint32_t, uint32_t) = nullptr;
    int (*is_cut)(double, double) = nullptr;
    tm_scene *s = nullptr;
    uint32_t w, h, batch;
    int bins;
    double threshold;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    bool have_prev = false;
    tm_scene_frame prev;
    std::vector<tm_scene_frame> out;
    std::deque<std::pair<double, bool>> ready;

    SceneRun(uint32_t w_, uint32_t h_, uint32_t batch_, uint32_t bins_, double threshold_)
        : w(w_), h(h_), batch(batch_), bins((int)bins_), threshold(threshold_)
    {
        const char *path = getenv("TM_SCENE_LIB");
        lib = dlopen(path ? path : "libturbometrics_scene.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("--scenes needs libturbometrics_scene.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_scene_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_scene_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_scene_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_scene_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_scene_sync");
        get = (decltype(get))dlsym(lib, "tm_scene_get");
        distance = (decltype(distance))dlsym(lib, "tm_scene_distance");
        score = (decltype(score))dlsym(lib, "tm_scene_score");
        is_cut = (decltype(is_cut))dlsym(lib, "tm_scene_is_cut");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !distance || !score || !is_cut)
            throw std::runtime_error("libturbometrics_scene.so does not export include/turbo_metrics_scene.h");
    }
    ~SceneRun()
    {
        if (s) destroy(s);
        if (lib) dlclose(lib);
    }
    void push(const HwFrame &r)
    {
        int l;
        uint32_t b;
        switch (r.kind) {
        case HwFrame::NvDecNV12: l = TM_SCENE_Y8; b = 8; break;
        case HwFrame::NvDecP016: l = TM_SCENE_Y16_MSB; b = 10; break;
        case HwFrame::Planar420: b = (uint32_t)r.bits; l = b == 8 ? TM_SCENE_Y8 : TM_SCENE_Y16_LOW; break;
        case HwFrame::Planar420P10: l = TM_SCENE_Y10_PACKED; b = 10; break;
        default: throw std::runtime_error("scenes needs YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
        if (!s) {
            layout = l; bits = b;
            chk(create(&s, w, h, layout, bits, batch), "tm_scene_create");
        } else if (l != layout || b != bits) {
            throw std::runtime_error("scenes: the YUV layout changed inside the stream");
        }
        chk(set_frame(s, filled, r.data, r.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_scene_set_frame");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(s, filled), "tm_scene_compute_async");
        chk(sync(s), "tm_scene_sync");
        out.resize(filled);
        chk(get(s, 0, filled, out.data()), "tm_scene_get");
        for (const tm_scene_frame &f : out) {
            double sc = 0.0; // the first picture of a sequence has score 0 and is never a cut
            bool cut = false;
            if (have_prev) {
                uint64_t d = 0;
                chk(distance(prev.hist, f.hist, bins, &d), "tm_scene_distance");
                sc = score(d, w, h);
                cut = is_cut(sc, threshold) != 0;
            }
            ready.emplace_back(sc, cut);
            prev = f;
            have_prev = true;
        }
        filled = 0;
    }
    std::pair<double, bool> pop()
    {
        if (ready.empty()) throw std::logic_error("scenes: a picture's result is missing");
        const std::pair<double, bool> v = ready.front();
        ready.pop_front();
        return v;
    }
};

// ---- CAMBI ---------------------------------------------------------------------------------------------------------
// libturbometrics_cambi.so, loaded at run time like the scene library (a CLI run without -m cambi never loads it).  The luma of ONE
// stream of every kept pair is handed over as a TM_MEM_HOST copy and computed batch by batch in stream order; a picture's six scores
// (five scales, cambi) wait in `ready` until the engine's scores of the same pair are drained.  The scores are the library's host
// function: nothing here restates the definition.  No history: --every is fine.
struct CambiRun {
    void *lib = nullptr;
    int (*create)(tm_cambi **, uint32_t, uint32_t, int, uint32_t, uint32_t, double, double, uint32_t) = nullptr;
    void (*destroy)(tm_cambi *) = nullptr;
    int (*set_frame)(tm_cambi *, uint32_t, const void *, size_t, int) = nullptr;
    int (*compute_async)(tm_cambi *, uint32_t) = nullptr;
    int (*sync)(tm_cambi *) = nullptr;
    int (*get)(tm_cambi *, uint32_t, uint32_t, tm_cambi_frame *) = nullptr;
    int (*scores)(const tm_cambi_frame *, uint32_t, double *) = nullptr;
    uint32_t (*window_of)(uint32_t, uint32_t) = nullptr;
    tm_cambi *s = nullptr;
    uint32_t w, h, batch, window;
    double topk;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    std::vector<tm_cambi_frame> out;
    std::deque<std::array<double, 6>> ready;

    CambiRun(uint32_t w_, uint32_t h_, uint32_t batch_, uint32_t window_, double topk_) : w(w_), h(h_), batch(batch_), window(window_), topk(topk_)
    {
        const char *path = getenv("TM_CAMBI_LIB");
        lib = dlopen(path ? path : "libturbometrics_cambi.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m cambi needs libturbometrics_cambi.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_cambi_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_cambi_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_cambi_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_cambi_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_cambi_sync");
        get = (decltype(get))dlsym(lib, "tm_cambi_get");
        scores = (decltype(scores))dlsym(lib, "tm_cambi_scores");
        window_of = (decltype(window_of))dlsym(lib, "tm_cambi_window");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !scores || !window_of)
            throw std::runtime_error("libturbometrics_cambi.so does not export include/turbo_metrics_cambi.h");
    }
    ~CambiRun()
    {
        if (s) destroy(s);
        if (lib) dlclose(lib);
    }
    void push(const HwFrame &r)
    {
        int l;
        uint32_t b;
        switch (r.kind) {
        case HwFrame::NvDecNV12: l = TM_CAMBI_Y8; b = 8; break;
        case HwFrame::NvDecP016: l = TM_CAMBI_Y16_MSB; b = 10; break;
        case HwFrame::Planar420: b = (uint32_t)r.bits; l = b == 8 ? TM_CAMBI_Y8 : TM_CAMBI_Y16_LOW; break;
        case HwFrame::Planar420P10: l = TM_CAMBI_Y10_PACKED; b = 10; break;
        default: throw std::runtime_error("cambi needs YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
        if (!s) {
            layout = l; bits = b;
            const int rc = create(&s, w, h, layout, bits, window, topk, TM_CAMBI_DEFAULT_TVI_THRESHOLD, batch);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("cambi takes pictures of at least 32 x 32 and at most 2^31 samples, at 8 to 16 bits in a layout that carries them, a window of 0 or 3 .. 127 and a topk in (0, 1]");
            chk(rc, "tm_cambi_create");
        } else if (l != layout || b != bits) {
            throw std::runtime_error("cambi: the YUV layout changed inside the stream");
        }
        chk(set_frame(s, filled, r.data, r.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_cambi_set_frame");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(s, filled), "tm_cambi_compute_async");
        chk(sync(s), "tm_cambi_sync");
        out.resize(filled);
        chk(get(s, 0, filled, out.data()), "tm_cambi_get");
        const uint32_t win = window_of(w, window);
        for (const tm_cambi_frame &f : out) {
            std::array<double, 6> v;
            chk(scores(&f, win, v.data()), "tm_cambi_scores");
            ready.push_back(v);
        }
        filled = 0;
    }
    std::array<double, 6> pop()
    {
        if (ready.empty()) throw std::logic_error("cambi: a picture's result is missing");
        const std::array<double, 6> v = ready.front();
        ready.pop_front();
        return v;
    }
};

// ---- FLIP ----------------------------------------------------------------------------------------------------------
// libturbometrics_flip.so, loaded at run time like the CAMBI library (a CLI run without -m flip never loads it).  Every kept pair of
// 8-bit RGB pictures is handed over as TM_MEM_HOST copies and computed batch by batch in stream order; a pair's mean, min and max wait
// in `ready` until the engine's scores of the same pair are drained.  --flip-map: every pair's FLIP map goes to PREFIX%06d.pfm, numbered
// in the order the pairs are computed.  No history: --every is fine.
struct FlipRun {
    void *lib = nullptr;
    int (*create)(tm_flip **, uint32_t, uint32_t, int, double, uint32_t) = nullptr;
    void (*destroy)(tm_flip *) = nullptr;
    int (*set_pair)(tm_flip *, uint32_t, const void *, size_t, const void *, size_t, int) = nullptr;
    int (*compute_async)(tm_flip *, uint32_t) = nullptr;
    int (*sync)(tm_flip *) = nullptr;
    int (*get)(tm_flip *, uint32_t, uint32_t, tm_flip_frame *) = nullptr;
    int (*get_map)(tm_flip *, uint32_t, int, float *, size_t) = nullptr;
    tm_flip *s = nullptr;
    uint32_t w, h, batch, filled = 0;
    double ppd;
    std::string map_prefix;
    size_t written = 0;
    std::vector<tm_flip_frame> out;
    std::vector<float> map;
    std::deque<std::array<double, 3>> ready;

    FlipRun(uint32_t w_, uint32_t h_, uint32_t batch_, double ppd_, std::string prefix) : w(w_), h(h_), batch(batch_), ppd(ppd_), map_prefix(std::move(prefix))
    {
        const char *path = getenv("TM_FLIP_LIB");
        lib = dlopen(path ? path : "libturbometrics_flip.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m flip needs libturbometrics_flip.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_flip_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_flip_destroy");
        set_pair = (decltype(set_pair))dlsym(lib, "tm_flip_set_pair");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_flip_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_flip_sync");
        get = (decltype(get))dlsym(lib, "tm_flip_get");
        get_map = (decltype(get_map))dlsym(lib, "tm_flip_get_map");
        if (!create || !destroy || !set_pair || !compute_async || !sync || !get || !get_map)
            throw std::runtime_error("libturbometrics_flip.so does not export include/turbo_metrics_flip.h");
    }
    ~FlipRun()
    {
        if (s) destroy(s);
        if (lib) dlclose(lib);
    }
    void push(const HwFrame &r, const HwFrame &d)
    {
        if (r.kind != HwFrame::Npp8 || d.kind != HwFrame::Npp8)
            throw std::runtime_error("flip needs 8-bit RGB images (PNG, PPM) on both sides, not YUV or deeper pictures");
        if (!s) {
            const int rc = create(&s, w, h, TM_FLIP_RGB8, ppd, batch);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("flip takes pictures of at most 2^31 samples and a --flip-ppd of 8 to 74.04 (a filter radius of at most 10)");
            chk(rc, "tm_flip_create");
        }
        if (r.device != d.device) throw std::runtime_error("flip: one picture of a pair is in device memory and the other is not");
        chk(set_pair(s, filled, r.data, r.pitch, d.data, d.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_flip_set_pair");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(s, filled), "tm_flip_compute_async");
        chk(sync(s), "tm_flip_sync");
        out.resize(filled);
        chk(get(s, 0, filled, out.data()), "tm_flip_get");
        for (uint32_t i = 0; i < filled; ++i) {
            ready.push_back({out[i].mean, out[i].min, out[i].max});
            if (map_prefix.empty()) continue;
            map.resize((size_t)w * h);
            chk(get_map(s, i, TM_FLIP_MAP, map.data(), (size_t)w * sizeof(float)), "tm_flip_get_map");
            char num[32];
            snprintf(num, sizeof num, "%06zu.pfm", written++);
            write_pfm_gray(map_prefix + num, w, h, map.data());
        }
        filled = 0;
    }
    std::array<double, 3> pop()
    {
        if (ready.empty()) throw std::logic_error("flip: a pair's result is missing");
        const std::array<double, 3> v = ready.front();
        ready.pop_front();
        return v;
    }
};

// ---- plane-wise YUV PSNR / SSIM --------------------------------------------------------------------------------------
// libturbometrics_yuv.so, loaded at run time like the XPSNR library (a CLI run without -m psnr-yuv / -m ssim-yuv never loads it).  Pairs are
// handed over as -m xpsnr hands them over and computed batch by batch in stream order; a pair's eight values (kYuvNames) wait in `ready`
// until the engine's scores of the same pair are drained.  The sequence values: PSNR from the summed SSE over the summed sample counts,
// SSIM as the mean over the frames.  --ssim-yuv-map: every pair's luma map goes to PREFIX%06d.pfm, numbered in the order the pairs are
// computed.  No history: --every is fine.
const char *const kYuvNames[8] = {"psnr_y", "psnr_u", "psnr_v", "psnr_avg", "ssim_y", "ssim_u", "ssim_v", "ssim_all"};

struct YuvRun {
    void *lib = nullptr;
    int (*create)(tm_yuv **, uint32_t, uint32_t, int, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_yuv *) = nullptr;
    int (*set_frame)(tm_yuv *, uint32_t, int, const void *, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_yuv *, uint32_t) = nullptr;
    int (*sync)(tm_yuv *) = nullptr;
    int (*get)(tm_yuv *, uint32_t, uint32_t, tm_yuv_frame *) = nullptr;
    int (*get_map)(tm_yuv *, uint32_t, int, float *, size_t) = nullptr;
    double (*psnr)(uint64_t, uint64_t, uint32_t, double) = nullptr;
    double (*ssim_all)(const double *, uint32_t, uint32_t) = nullptr;
    int (*map_size)(uint32_t, uint32_t, int, uint32_t *, uint32_t *) = nullptr;
    tm_yuv *x = nullptr;
    uint32_t w, h, batch;
    bool use_cap;
    std::string map_prefix;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    size_t written = 0;
    std::vector<float> map;
    std::deque<std::array<double, 8>> ready;
    uint64_t sum_sse[3] = {0, 0, 0}, frames = 0;
    double sum_ssim[4] = {0, 0, 0, 0};

    YuvRun(uint32_t w_, uint32_t h_, uint32_t batch_, bool cap, std::string prefix) : w(w_), h(h_), batch(batch_), use_cap(cap), map_prefix(std::move(prefix))
    {
        const char *path = getenv("TM_YUV_LIB");
        lib = dlopen(path ? path : "libturbometrics_yuv.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m psnr-yuv / ssim-yuv need libturbometrics_yuv.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_yuv_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_yuv_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_yuv_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_yuv_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_yuv_sync");
        get = (decltype(get))dlsym(lib, "tm_yuv_get");
        get_map = (decltype(get_map))dlsym(lib, "tm_yuv_get_ssim_map");
        psnr = (decltype(psnr))dlsym(lib, "tm_yuv_psnr");
        ssim_all = (decltype(ssim_all))dlsym(lib, "tm_yuv_ssim_all");
        map_size = (decltype(map_size))dlsym(lib, "tm_yuv_map_size");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !get_map || !psnr || !ssim_all || !map_size)
            throw std::runtime_error("libturbometrics_yuv.so does not export include/turbo_metrics_yuv.h");
    }
    ~YuvRun()
    {
        if (x) destroy(x);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &layout, uint32_t &bits)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: layout = TM_YUV_NV12; bits = 8; return;
        case HwFrame::NvDecP016: layout = TM_YUV_P016; bits = 10; return;
        case HwFrame::Planar420: layout = TM_YUV_I420; bits = (uint32_t)f.bits; return;
        case HwFrame::Planar420P10: layout = TM_YUV_I420P10_PACKED; bits = 10; return;
        default: throw std::runtime_error("psnr-yuv / ssim-yuv need 4:2:0 YUV input");
        }
    }
    uint64_t samples(int c) const { return c ? (uint64_t)((w + 1) / 2) * ((h + 1) / 2) : (uint64_t)w * h; }
    double cap() const { return use_cap ? 6.0 * bits + 12.0 : 0.0; }
    void push(const HwFrame &r, const HwFrame &d)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd) throw std::runtime_error("psnr-yuv / ssim-yuv need reference and distorted in the same YUV layout and bit depth");
        if (!x) {
            layout = lr; bits = br;
            const int rc = create(&x, w, h, layout, bits, batch);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("psnr-yuv / ssim-yuv take pictures of 16 x 16 to 32768 x 32768 samples");
            chk(rc, "tm_yuv_create");
        } else if (lr != layout || br != bits) {
            throw std::runtime_error("psnr-yuv / ssim-yuv: the YUV layout changed inside the stream");
        }
        const bool bi = layout == TM_YUV_NV12 || layout == TM_YUV_P016;
        int side = TM_SIDE_REF;
        for (const HwFrame *f : {&r, &d}) {
            chk(set_frame(x, filled, side, f->data, bi ? f->uv : f->u, bi ? nullptr : f->v, f->pitch, bi ? f->pitch : f->pitch_uv,
                          f->device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_yuv_set_frame");
            side = TM_SIDE_DIS;
        }
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(x, filled), "tm_yuv_compute_async");
        chk(sync(x), "tm_yuv_sync");
        std::vector<tm_yuv_frame> out(filled);
        chk(get(x, 0, filled, out.data()), "tm_yuv_get");
        for (uint32_t i = 0; i < filled; ++i) {
            const tm_yuv_frame &f = out[i];
            std::array<double, 8> v;
            for (int c = 0; c < 3; ++c) {
                v[c] = psnr(f.sse[c], samples(c), bits, cap());
                v[4 + c] = f.ssim[c];
                sum_sse[c] += f.sse[c];
            }
            v[3] = psnr(f.sse[0] + f.sse[1] + f.sse[2], samples(0) + 2 * samples(1), bits, cap());
            v[7] = ssim_all(f.ssim, w, h);
            for (int k = 0; k < 4; ++k) sum_ssim[k] += v[4 + k];
            ready.push_back(v);
            ++frames;
            if (map_prefix.empty()) continue;
            uint32_t mw = 0, mh = 0;
            chk(map_size(w, h, 0, &mw, &mh), "tm_yuv_map_size");
            map.resize((size_t)mw * mh);
            chk(get_map(x, i, 0, map.data(), (size_t)mw * sizeof(float)), "tm_yuv_get_ssim_map");
            char num[32];
            snprintf(num, sizeof num, "%06zu.pfm", written++);
            write_pfm_gray(map_prefix + num, mw, mh, map.data());
        }
        filled = 0;
    }
    std::array<double, 8> pop()
    {
        if (ready.empty()) throw std::logic_error("psnr-yuv / ssim-yuv: a pair's result is missing");
        const std::array<double, 8> v = ready.front();
        ready.pop_front();
        return v;
    }
    // the sequence value of column k (kYuvNames)
    double sequence_score(int k) const
    {
        if (k < 3) return psnr(sum_sse[k], samples(k) * frames, bits, cap());
        if (k == 3) return psnr(sum_sse[0] + sum_sse[1] + sum_sse[2], (samples(0) + 2 * samples(1)) * frames, bits, cap());
        return sum_ssim[k - 4] / (double)frames;
    }
};

// ---- PSNR-HVS / PSNR-HVS-M ---------------------------------------------------------------------------------------------
// libturbometrics_hvs.so, loaded at run time like the VIF library (a CLI run without -m psnr-hvs / -m psnr-hvs-m never loads it).  The lumas
// of every kept pair are handed over as -m vif hands them over and computed batch by batch in stream order; a pair's two values
// (kHvsNames) wait in `ready` until the engine's scores of the same pair are drained.  The sequence values: the PSNR of the summed S
// over the summed number of blocks.  No history: --every is fine.
const char *const kHvsNames[2] = {"psnr_hvs", "psnr_hvs_m"};

struct HvsRun {
    void *lib = nullptr;
    int (*create)(tm_hvs **, uint32_t, uint32_t, int, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_hvs *) = nullptr;
    int (*set_pair)(tm_hvs *, uint32_t, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_hvs *, uint32_t) = nullptr;
    int (*sync)(tm_hvs *) = nullptr;
    int (*get)(tm_hvs *, uint32_t, uint32_t, tm_hvs_frame *) = nullptr;
    double (*psnr)(double, uint64_t, uint32_t) = nullptr;
    tm_hvs *v = nullptr;
    uint32_t w, h, batch;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    std::deque<std::array<double, 2>> ready;
    double sum_s[2] = {0.0, 0.0};
    uint64_t sum_blocks = 0;

    HvsRun(uint32_t w_, uint32_t h_, uint32_t batch_) : w(w_), h(h_), batch(batch_)
    {
        const char *path = getenv("TM_HVS_LIB");
        lib = dlopen(path ? path : "libturbometrics_hvs.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m psnr-hvs / psnr-hvs-m need libturbometrics_hvs.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_hvs_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_hvs_destroy");
        set_pair = (decltype(set_pair))dlsym(lib, "tm_hvs_set_pair");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_hvs_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_hvs_sync");
        get = (decltype(get))dlsym(lib, "tm_hvs_get");
        psnr = (decltype(psnr))dlsym(lib, "tm_hvs_psnr");
        if (!create || !destroy || !set_pair || !compute_async || !sync || !get || !psnr) {
            dlclose(lib); // the destructor does not run for an object whose constructor throws
            throw std::runtime_error("libturbometrics_hvs.so does not export include/turbo_metrics_hvs.h");
        }
    }
    ~HvsRun()
    {
        if (v) destroy(v);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &l, uint32_t &b)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: l = TM_HVS_Y8; b = 8; return;
        case HwFrame::NvDecP016: l = TM_HVS_Y16_MSB; b = 10; return;
        case HwFrame::Planar420: b = (uint32_t)f.bits; l = b == 8 ? TM_HVS_Y8 : TM_HVS_Y16_LOW; return;
        case HwFrame::Planar420P10: l = TM_HVS_Y10_PACKED; b = 10; return;
        default: throw std::runtime_error("psnr-hvs / psnr-hvs-m need YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    void push(const HwFrame &r, const HwFrame &d)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd || r.device != d.device) throw std::runtime_error("psnr-hvs / psnr-hvs-m need reference and distorted in the same YUV layout and bit depth");
        if (!v) {
            layout = lr; bits = br;
            const int rc = create(&v, w, h, layout, bits, batch);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("psnr-hvs / psnr-hvs-m take pictures of 8 x 8 to 32768 x 32768 samples");
            chk(rc, "tm_hvs_create");
        } else if (lr != layout || br != bits) {
            throw std::runtime_error("psnr-hvs / psnr-hvs-m: the YUV layout changed inside the stream");
        }
        chk(set_pair(v, filled, r.data, d.data, r.pitch, d.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_hvs_set_pair");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(v, filled), "tm_hvs_compute_async");
        chk(sync(v), "tm_hvs_sync");
        std::vector<tm_hvs_frame> out(filled);
        chk(get(v, 0, filled, out.data()), "tm_hvs_get");
        for (const tm_hvs_frame &f : out) {
            ready.push_back({psnr(f.s_hvs, f.blocks, bits), psnr(f.s_hvsm, f.blocks, bits)});
            sum_s[0] += f.s_hvs; sum_s[1] += f.s_hvsm;
            sum_blocks += f.blocks;
        }
        filled = 0;
    }
    std::array<double, 2> pop()
    {
        if (ready.empty()) throw std::logic_error("psnr-hvs / psnr-hvs-m: a pair's result is missing");
        const std::array<double, 2> s = ready.front();
        ready.pop_front();
        return s;
    }
    // the sequence value of column k (kHvsNames)
    double sequence_score(int k) const { return psnr(sum_s[k], sum_blocks, bits); }
};

// ---- GMSD ----------------------------------------------------------------------------------------------------------------
// libturbometrics_gmsd.so, loaded at run time like the PSNR-HVS library (a CLI run without -m gmsd never loads it).  The lumas of every kept
// pair are handed over as -m psnr-hvs hands them over and computed batch by batch in stream order; a pair's two values (kGmsdNames: gmsd and
// gmsm, the mean GMS) wait in `ready` until the engine's scores of the same pair are drained.  The sequence values: the library's host
// functions of the summed E1, E2 and N -- pooled over all positions of all pairs.  --gmsd-map: every pair's GMS map goes to PREFIX%06d.pfm,
// numbered in the order the pairs are computed.  No history: --every is fine.
const char *const kGmsdNames[2] = {"gmsd", "gmsm"};

struct GmsdRun {
    void *lib = nullptr;
    int (*create)(tm_gmsd **, uint32_t, uint32_t, int, uint32_t, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_gmsd *) = nullptr;
    int (*set_pair)(tm_gmsd *, uint32_t, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_gmsd *, uint32_t) = nullptr;
    int (*sync)(tm_gmsd *) = nullptr;
    int (*get)(tm_gmsd *, uint32_t, uint32_t, tm_gmsd_frame *) = nullptr;
    int (*get_map)(tm_gmsd *, uint32_t, float *, size_t) = nullptr;
    double (*score)(double, double, uint64_t, int) = nullptr;
    double (*mean)(double, uint64_t) = nullptr;
    tm_gmsd *v = nullptr;
    uint32_t w, h, batch;
    bool population;
    std::string map_prefix;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    size_t written = 0;
    std::vector<float> map;
    std::deque<std::array<double, 2>> ready;
    double sum_e1 = 0.0, sum_e2 = 0.0;
    uint64_t sum_n = 0;

    GmsdRun(uint32_t w_, uint32_t h_, uint32_t batch_, bool population_, std::string prefix)
        : w(w_), h(h_), batch(batch_), population(population_), map_prefix(std::move(prefix))
    {
        const char *path = getenv("TM_GMSD_LIB");
        lib = dlopen(path ? path : "libturbometrics_gmsd.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m gmsd needs libturbometrics_gmsd.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_gmsd_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_gmsd_destroy");
        set_pair = (decltype(set_pair))dlsym(lib, "tm_gmsd_set_pair");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_gmsd_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_gmsd_sync");
        get = (decltype(get))dlsym(lib, "tm_gmsd_get");
        get_map = (decltype(get_map))dlsym(lib, "tm_gmsd_map");
        score = (decltype(score))dlsym(lib, "tm_gmsd_score");
        mean = (decltype(mean))dlsym(lib, "tm_gmsd_mean");
        if (!create || !destroy || !set_pair || !compute_async || !sync || !get || !get_map || !score || !mean) {
            dlclose(lib); // the destructor does not run for an object whose constructor throws
            throw std::runtime_error("libturbometrics_gmsd.so does not export include/turbo_metrics_gmsd.h");
        }
    }
    ~GmsdRun()
    {
        if (v) destroy(v);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &l, uint32_t &b)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: l = TM_GMSD_Y8; b = 8; return;
        case HwFrame::NvDecP016: l = TM_GMSD_Y16_MSB; b = 10; return;
        case HwFrame::Planar420: b = (uint32_t)f.bits; l = b == 8 ? TM_GMSD_Y8 : TM_GMSD_Y16_LOW; return;
        case HwFrame::Planar420P10: l = TM_GMSD_Y10_PACKED; b = 10; return;
        default: throw std::runtime_error("gmsd needs YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    void push(const HwFrame &r, const HwFrame &d)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd || r.device != d.device) throw std::runtime_error("gmsd needs reference and distorted in the same YUV layout and bit depth");
        if (!v) {
            layout = lr; bits = br;
            const int rc = create(&v, w, h, layout, bits, batch, map_prefix.empty() ? 0u : (uint32_t)TM_GMSD_MAPS);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("gmsd takes pictures of 4 x 4 to 32768 x 32768 samples");
            chk(rc, "tm_gmsd_create");
        } else if (lr != layout || br != bits) {
            throw std::runtime_error("gmsd: the YUV layout changed inside the stream");
        }
        chk(set_pair(v, filled, r.data, d.data, r.pitch, d.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_gmsd_set_pair");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(v, filled), "tm_gmsd_compute_async");
        chk(sync(v), "tm_gmsd_sync");
        std::vector<tm_gmsd_frame> out(filled);
        chk(get(v, 0, filled, out.data()), "tm_gmsd_get");
        const uint32_t w2 = (w + 1) / 2, h2 = (h + 1) / 2;
        for (uint32_t i = 0; i < filled; ++i) {
            const tm_gmsd_frame &f = out[i];
            ready.push_back({score(f.e1, f.e2, f.n, population), mean(f.e1, f.n)});
            sum_e1 += f.e1; sum_e2 += f.e2;
            sum_n += f.n;
            if (map_prefix.empty()) continue;
            map.resize((size_t)w2 * h2);
            chk(get_map(v, i, map.data(), (size_t)w2 * sizeof(float)), "tm_gmsd_map");
            char num[32];
            snprintf(num, sizeof num, "%06zu.pfm", written++);
            write_pfm_gray(map_prefix + num, w2, h2, map.data());
        }
        filled = 0;
    }
    std::array<double, 2> pop()
    {
        if (ready.empty()) throw std::logic_error("gmsd: a pair's result is missing");
        const std::array<double, 2> s = ready.front();
        ready.pop_front();
        return s;
    }
    // the sequence value of column k (kGmsdNames)
    double sequence_score(int k) const { return k ? mean(sum_e1, sum_n) : score(sum_e1, sum_e2, sum_n, population); }
};

// ---- HaarPSI -------------------------------------------------------------------------------------------------------------
// libturbometrics_haarpsi.so, loaded at run time like the GMSD library (a CLI run without -m haarpsi never loads it).  The lumas of every
// kept pair are handed over as -m gmsd hands them over and computed batch by batch in stream order; a pair's value waits in `ready` until
// the engine's scores of the same pair are drained.  The sequence value: the library's host function of the summed Q and WS.
// --haarpsi-map: every pair's local similarity map goes to PREFIX%06d.pfm, numbered in the order the pairs are computed.  No history:
// --every is fine.
struct HaarpsiRun {
    void *lib = nullptr;
    int (*create)(tm_haarpsi **, uint32_t, uint32_t, int, uint32_t, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_haarpsi *) = nullptr;
    int (*set_pair)(tm_haarpsi *, uint32_t, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_haarpsi *, uint32_t) = nullptr;
    int (*sync)(tm_haarpsi *) = nullptr;
    int (*get)(tm_haarpsi *, uint32_t, uint32_t, tm_haarpsi_frame *) = nullptr;
    int (*get_map)(tm_haarpsi *, uint32_t, float *, size_t) = nullptr;
    double (*score)(double, uint64_t) = nullptr;
    tm_haarpsi *v = nullptr;
    uint32_t w, h, batch;
    std::string map_prefix;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    size_t written = 0;
    std::vector<float> map;
    std::deque<double> ready;
    double sum_q = 0.0;
    uint64_t sum_ws = 0;

    HaarpsiRun(uint32_t w_, uint32_t h_, uint32_t batch_, std::string prefix) : w(w_), h(h_), batch(batch_), map_prefix(std::move(prefix))
    {
        const char *path = getenv("TM_HAARPSI_LIB");
        lib = dlopen(path ? path : "libturbometrics_haarpsi.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m haarpsi needs libturbometrics_haarpsi.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_haarpsi_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_haarpsi_destroy");
        set_pair = (decltype(set_pair))dlsym(lib, "tm_haarpsi_set_pair");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_haarpsi_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_haarpsi_sync");
        get = (decltype(get))dlsym(lib, "tm_haarpsi_get");
        get_map = (decltype(get_map))dlsym(lib, "tm_haarpsi_map");
        score = (decltype(score))dlsym(lib, "tm_haarpsi_score");
        if (!create || !destroy || !set_pair || !compute_async || !sync || !get || !get_map || !score) {
            dlclose(lib); // the destructor does not run for an object whose constructor throws
            throw std::runtime_error("libturbometrics_haarpsi.so does not export include/turbo_metrics_haarpsi.h");
        }
    }
    ~HaarpsiRun()
    {
        if (v) destroy(v);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &l, uint32_t &b)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: l = TM_HAARPSI_Y8; b = 8; return;
        case HwFrame::NvDecP016: l = TM_HAARPSI_Y16_MSB; b = 10; return;
        case HwFrame::Planar420: b = (uint32_t)f.bits; l = b == 8 ? TM_HAARPSI_Y8 : TM_HAARPSI_Y16_LOW; return;
        case HwFrame::Planar420P10: l = TM_HAARPSI_Y10_PACKED; b = 10; return;
        default: throw std::runtime_error("haarpsi needs YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    void push(const HwFrame &r, const HwFrame &d)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd || r.device != d.device) throw std::runtime_error("haarpsi needs reference and distorted in the same YUV layout and bit depth");
        if (!v) {
            layout = lr; bits = br;
            const int rc = create(&v, w, h, layout, bits, batch, map_prefix.empty() ? 0u : (uint32_t)TM_HAARPSI_MAPS);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("haarpsi takes pictures of 4 x 4 to 32768 x 32768 samples");
            chk(rc, "tm_haarpsi_create");
        } else if (lr != layout || br != bits) {
            throw std::runtime_error("haarpsi: the YUV layout changed inside the stream");
        }
        chk(set_pair(v, filled, r.data, d.data, r.pitch, d.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_haarpsi_set_pair");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(v, filled), "tm_haarpsi_compute_async");
        chk(sync(v), "tm_haarpsi_sync");
        std::vector<tm_haarpsi_frame> out(filled);
        chk(get(v, 0, filled, out.data()), "tm_haarpsi_get");
        const uint32_t w2 = (w + 1) / 2, h2 = (h + 1) / 2;
        for (uint32_t i = 0; i < filled; ++i) {
            const tm_haarpsi_frame &f = out[i];
            ready.push_back(score(f.q, f.ws));
            sum_q += f.q;
            sum_ws += f.ws;
            if (map_prefix.empty()) continue;
            map.resize((size_t)w2 * h2);
            chk(get_map(v, i, map.data(), (size_t)w2 * sizeof(float)), "tm_haarpsi_map");
            char num[32];
            snprintf(num, sizeof num, "%06zu.pfm", written++);
            write_pfm_gray(map_prefix + num, w2, h2, map.data());
        }
        filled = 0;
    }
    double pop()
    {
        if (ready.empty()) throw std::logic_error("haarpsi: a pair's result is missing");
        const double s = ready.front();
        ready.pop_front();
        return s;
    }
    double sequence_score() const { return score(sum_q, sum_ws); }
};

// ---- dE ITP ----------------------------------------------------------------------------------------------------------------
// libturbometrics_itp.so, loaded at run time like the CIEDE2000 library (a CLI run without -m deitp never loads it).  Pairs are handed over
// as -m ciede2000 hands them over and computed batch by batch in stream order; a pair's two values (kItpNames: the mean and the largest
// dE ITP) wait in `ready` until the engine's scores of the same pair are drained.  The matrix is always BT.2020 non-constant luminance: the
// streams' matrix coefficients are not consulted; the transfer is --itp-transfer's.  The sequence values: the summed dE ITP over the summed
// positions, and the largest maximum.  --itp-map: every pair's dE ITP map goes to PREFIX%06d.pfm, numbered in the order the pairs are
// computed.  No history: --every is fine.
const char *const kItpNames[2] = {"deitp", "deitp_max"};

struct ItpRun {
    void *lib = nullptr;
    int (*create)(tm_itp **, uint32_t, uint32_t, int, uint32_t, int, int, int, uint32_t) = nullptr;
    void (*destroy)(tm_itp *) = nullptr;
    int (*set_frame)(tm_itp *, uint32_t, int, const void *, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_itp *, uint32_t) = nullptr;
    int (*sync)(tm_itp *) = nullptr;
    int (*get)(tm_itp *, uint32_t, uint32_t, tm_itp_frame *) = nullptr;
    int (*get_map)(tm_itp *, uint32_t, float *, size_t) = nullptr;
    tm_itp *x = nullptr;
    uint32_t w, h, batch;
    bool hlg;
    std::string map_prefix;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    size_t written = 0;
    std::vector<float> map;
    std::deque<std::array<double, 2>> ready;
    double sum_de = 0.0, max_de = 0.0;
    uint64_t sum_px = 0;

    ItpRun(uint32_t w_, uint32_t h_, uint32_t batch_, bool hlg_, std::string prefix) : w(w_), h(h_), batch(batch_), hlg(hlg_), map_prefix(std::move(prefix))
    {
        const char *path = getenv("TM_ITP_LIB");
        lib = dlopen(path ? path : "libturbometrics_itp.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m deitp needs libturbometrics_itp.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_itp_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_itp_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_itp_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_itp_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_itp_sync");
        get = (decltype(get))dlsym(lib, "tm_itp_get");
        get_map = (decltype(get_map))dlsym(lib, "tm_itp_get_map");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !get_map) {
            dlclose(lib); // the destructor does not run for an object whose constructor throws
            throw std::runtime_error("libturbometrics_itp.so does not export include/turbo_metrics_itp.h");
        }
    }
    ~ItpRun()
    {
        if (x) destroy(x);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &layout, uint32_t &bits)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: layout = TM_ITP_NV12; bits = 8; return;
        case HwFrame::NvDecP016: layout = TM_ITP_P016; bits = 10; return;
        case HwFrame::Planar420: layout = TM_ITP_I420; bits = (uint32_t)f.bits; return;
        case HwFrame::Planar420P10: layout = TM_ITP_I420P10_PACKED; bits = 10; return;
        default: throw std::runtime_error("deitp needs 4:2:0 YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    using ColorInfo = TurboMetrics::ColorInfo;
    void push(const HwFrame &r, const HwFrame &d, const ColorInfo &cr, const ColorInfo &cd)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd) throw std::runtime_error("deitp needs reference and distorted in the same YUV layout and bit depth");
        if (cr.second == ColorRange::Full || cd.second == ColorRange::Full) throw std::runtime_error("deitp takes limited-range YUV only");
        if (!x) {
            layout = lr; bits = br;
            const int rc = create(&x, w, h, layout, bits, hlg ? TM_ITP_HLG : TM_ITP_PQ, 0, map_prefix.empty() ? 0 : 1, batch);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("deitp takes pictures of 2 x 2 to 32768 x 32768 samples");
            chk(rc, "tm_itp_create");
        } else if (lr != layout || br != bits) {
            throw std::runtime_error("deitp: the YUV layout changed inside the stream");
        }
        const bool bi = layout == TM_ITP_NV12 || layout == TM_ITP_P016;
        int side = TM_SIDE_REF;
        for (const HwFrame *f : {&r, &d}) {
            chk(set_frame(x, filled, side, f->data, bi ? f->uv : f->u, bi ? nullptr : f->v, f->pitch, bi ? f->pitch : f->pitch_uv,
                          f->device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_itp_set_frame");
            side = TM_SIDE_DIS;
        }
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(x, filled), "tm_itp_compute_async");
        chk(sync(x), "tm_itp_sync");
        std::vector<tm_itp_frame> out(filled);
        chk(get(x, 0, filled, out.data()), "tm_itp_get");
        for (uint32_t i = 0; i < filled; ++i) {
            const tm_itp_frame &f = out[i];
            ready.push_back({f.de_mean, f.de_max});
            sum_de += f.de_sum;
            sum_px += f.pixels;
            max_de = std::max(max_de, f.de_max);
            if (map_prefix.empty()) continue;
            map.resize((size_t)w * h);
            chk(get_map(x, i, map.data(), (size_t)w * sizeof(float)), "tm_itp_get_map");
            char num[32];
            snprintf(num, sizeof num, "%06zu.pfm", written++);
            write_pfm_gray(map_prefix + num, w, h, map.data());
        }
        filled = 0;
    }
    std::array<double, 2> pop()
    {
        if (ready.empty()) throw std::logic_error("deitp: a pair's result is missing");
        const std::array<double, 2> v = ready.front();
        ready.pop_front();
        return v;
    }
    // the sequence value of column k (kItpNames)
    double sequence_score(int k) const { return k ? max_de : sum_de / (double)sum_px; }
};

// ---- MDSI ----------------------------------------------------------------------------------------------------------------
// libturbometrics_mdsi.so, loaded at run time like the CIEDE2000 library (a CLI run without -m mdsi never loads it).  Pairs are handed over
// as -m ciede2000 hands them over, with its rule for the matrix (the streams' matrix coefficients: BT.709 or BT.601, limited range), and
// computed batch by batch in stream order; a pair's value waits in `ready` until the engine's scores of the same pair are drained.  MDSI
// does not pool across pictures: the sequence value is the mean of the pairs' values.  --mdsi-map: every pair's GCS map goes to
// PREFIX%06d.pfm, numbered in the order the pairs are computed.  No history: --every is fine.
struct MdsiRun {
    void *lib = nullptr;
    int (*create)(tm_mdsi **, uint32_t, uint32_t, int, uint32_t, int, uint32_t, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_mdsi *) = nullptr;
    int (*set_frame)(tm_mdsi *, uint32_t, int, const void *, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_mdsi *, uint32_t) = nullptr;
    int (*sync)(tm_mdsi *) = nullptr;
    int (*get)(tm_mdsi *, uint32_t, uint32_t, tm_mdsi_frame *) = nullptr;
    int (*get_map)(tm_mdsi *, uint32_t, float *, size_t) = nullptr;
    double (*score)(double, uint64_t) = nullptr;
    tm_mdsi *x = nullptr;
    uint32_t w, h, batch, factor;
    std::string map_prefix;
    int layout = -1, matrix = -1;
    uint32_t bits = 8, filled = 0;
    size_t written = 0;
    std::vector<float> map;
    std::deque<double> ready;
    double sum = 0.0;
    uint64_t pairs = 0;

    MdsiRun(uint32_t w_, uint32_t h_, uint32_t batch_, uint32_t factor_, std::string prefix) : w(w_), h(h_), batch(batch_), factor(factor_), map_prefix(std::move(prefix))
    {
        const char *path = getenv("TM_MDSI_LIB");
        lib = dlopen(path ? path : "libturbometrics_mdsi.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m mdsi needs libturbometrics_mdsi.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_mdsi_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_mdsi_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_mdsi_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_mdsi_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_mdsi_sync");
        get = (decltype(get))dlsym(lib, "tm_mdsi_get");
        get_map = (decltype(get_map))dlsym(lib, "tm_mdsi_map");
        score = (decltype(score))dlsym(lib, "tm_mdsi_score");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !get_map || !score) {
            dlclose(lib); // the destructor does not run for an object whose constructor throws
            throw std::runtime_error("libturbometrics_mdsi.so does not export include/turbo_metrics_mdsi.h");
        }
    }
    ~MdsiRun()
    {
        if (x) destroy(x);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &layout, uint32_t &bits)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: layout = TM_MDSI_NV12; bits = 8; return;
        case HwFrame::NvDecP016: layout = TM_MDSI_P016; bits = 10; return;
        case HwFrame::Planar420: layout = TM_MDSI_I420; bits = (uint32_t)f.bits; return;
        case HwFrame::Planar420P10: layout = TM_MDSI_I420P10_PACKED; bits = 10; return;
        default: throw std::runtime_error("mdsi needs 4:2:0 YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    // the library's matrix for a stream's colour metadata
    using ColorInfo = TurboMetrics::ColorInfo;
    int matrix_of(const ColorInfo &c) const
    {
        if (c.second == ColorRange::Full) throw std::runtime_error("mdsi takes limited-range YUV only");
        switch (c.first.mc) {
        case MatrixCoefficients::BT709: return TM_MDSI_BT709;
        case MatrixCoefficients::BT601_525: case MatrixCoefficients::BT601_625: return TM_MDSI_BT601;
        default: throw std::runtime_error(std::string("mdsi: not implemented: matrix coefficients ") + to_string(c.first.mc));
        }
    }
    void push(const HwFrame &r, const HwFrame &d, const ColorInfo &cr, const ColorInfo &cd)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd) throw std::runtime_error("mdsi needs reference and distorted in the same YUV layout and bit depth");
        const int mr = matrix_of(cr), md = matrix_of(cd);
        if (mr != md) throw std::runtime_error("mdsi needs reference and distorted with the same matrix coefficients");
        if (!x) {
            layout = lr; bits = br; matrix = mr;
            const int rc = create(&x, w, h, layout, bits, matrix, factor, map_prefix.empty() ? 0u : (uint32_t)TM_MDSI_MAPS, batch);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("mdsi takes pictures of 2 x 2 to 32768 x 32768 samples with at least four positions after the decimation by its factor");
            chk(rc, "tm_mdsi_create");
        } else if (lr != layout || br != bits || mr != matrix) {
            throw std::runtime_error("mdsi: the YUV layout or the matrix changed inside the stream");
        }
        const bool bi = layout == TM_MDSI_NV12 || layout == TM_MDSI_P016;
        int side = TM_SIDE_REF;
        for (const HwFrame *f : {&r, &d}) {
            chk(set_frame(x, filled, side, f->data, bi ? f->uv : f->u, bi ? nullptr : f->v, f->pitch, bi ? f->pitch : f->pitch_uv,
                          f->device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_mdsi_set_frame");
            side = TM_SIDE_DIS;
        }
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(x, filled), "tm_mdsi_compute_async");
        chk(sync(x), "tm_mdsi_sync");
        std::vector<tm_mdsi_frame> out(filled);
        chk(get(x, 0, filled, out.data()), "tm_mdsi_get");
        for (uint32_t i = 0; i < filled; ++i) {
            const tm_mdsi_frame &f = out[i];
            const double v = score(f.dev, f.n);
            ready.push_back(v);
            sum += v;
            ++pairs;
            if (map_prefix.empty()) continue;
            const uint32_t wd = (w + f.factor - 1) / f.factor, hd = (h + f.factor - 1) / f.factor; // the library's own factor
            map.resize((size_t)wd * hd);
            chk(get_map(x, i, map.data(), (size_t)wd * sizeof(float)), "tm_mdsi_map");
            char num[32];
            snprintf(num, sizeof num, "%06zu.pfm", written++);
            write_pfm_gray(map_prefix + num, wd, hd, map.data());
        }
        filled = 0;
    }
    double pop()
    {
        if (ready.empty()) throw std::logic_error("mdsi: a pair's result is missing");
        const double v = ready.front();
        ready.pop_front();
        return v;
    }
    // MDSI does not pool across pictures: the mean of the pairs' values
    double sequence_score() const { return pairs ? sum / (double)pairs : std::nan(""); }
};

// ---- CIEDE2000 ---------------------------------------------------------------------------------------------------------
// libturbometrics_ciede.so, loaded at run time like the YUV library (a CLI run without -m ciede2000 never loads it).  Pairs are handed over
// as -m psnr-yuv hands them over and computed batch by batch in stream order; a pair's two values (kCiedeNames: the score and the mean dE00)
// wait in `ready` until the engine's scores of the same pair are drained.  The matrix comes from the streams' colour metadata (BT.709 or
// BT.601; both streams the same), or is libvmaf's with --ciede-libvmaf, which also sets kL, kC, kH = 0.65, 1, 4.  The sequence values: from
// the summed dE00 over the summed positions.  --ciede-map: every pair's dE00 map goes to PREFIX%06d.pfm, numbered in the order the pairs are
// computed.  No history: --every is fine.
const char *const kCiedeNames[2] = {"ciede2000", "ciede2000_de"};

struct CiedeRun {
    void *lib = nullptr;
    int (*create)(tm_ciede **, uint32_t, uint32_t, int, uint32_t, int, double, double, double, int, int, uint32_t) = nullptr;
    void (*destroy)(tm_ciede *) = nullptr;
    int (*set_frame)(tm_ciede *, uint32_t, int, const void *, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_ciede *, uint32_t) = nullptr;
    int (*sync)(tm_ciede *) = nullptr;
    int (*get)(tm_ciede *, uint32_t, uint32_t, tm_ciede_frame *) = nullptr;
    int (*get_map)(tm_ciede *, uint32_t, float *, size_t) = nullptr;
    double (*score)(double, uint64_t) = nullptr;
    tm_ciede *x = nullptr;
    uint32_t w, h, batch;
    bool libvmaf;
    std::string map_prefix;
    int layout = -1, matrix = -1;
    uint32_t bits = 8, filled = 0;
    size_t written = 0;
    std::vector<float> map;
    std::deque<std::array<double, 2>> ready;
    double sum_de = 0.0;
    uint64_t sum_px = 0;

    CiedeRun(uint32_t w_, uint32_t h_, uint32_t batch_, bool libvmaf_, std::string prefix) : w(w_), h(h_), batch(batch_), libvmaf(libvmaf_), map_prefix(std::move(prefix))
    {
        const char *path = getenv("TM_CIEDE_LIB");
        lib = dlopen(path ? path : "libturbometrics_ciede.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m ciede2000 needs libturbometrics_ciede.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_ciede_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_ciede_destroy");
        set_frame = (decltype(set_frame))dlsym(lib, "tm_ciede_set_frame");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_ciede_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_ciede_sync");
        get = (decltype(get))dlsym(lib, "tm_ciede_get");
        get_map = (decltype(get_map))dlsym(lib, "tm_ciede_get_map");
        score = (decltype(score))dlsym(lib, "tm_ciede_score");
        if (!create || !destroy || !set_frame || !compute_async || !sync || !get || !get_map || !score) {
            dlclose(lib); // the destructor does not run for an object whose constructor throws
            throw std::runtime_error("libturbometrics_ciede.so does not export include/turbo_metrics_ciede.h");
        }
    }
    ~CiedeRun()
    {
        if (x) destroy(x);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &layout, uint32_t &bits)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: layout = TM_CIEDE_NV12; bits = 8; return;
        case HwFrame::NvDecP016: layout = TM_CIEDE_P016; bits = 10; return;
        case HwFrame::Planar420: layout = TM_CIEDE_I420; bits = (uint32_t)f.bits; return;
        case HwFrame::Planar420P10: layout = TM_CIEDE_I420P10_PACKED; bits = 10; return;
        default: throw std::runtime_error("ciede2000 needs 4:2:0 YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    // the library's matrix for a stream's colour metadata
    using ColorInfo = TurboMetrics::ColorInfo;
    int matrix_of(const ColorInfo &c) const
    {
        if (c.second == ColorRange::Full) throw std::runtime_error("ciede2000 takes limited-range YUV only");
        if (libvmaf) return TM_CIEDE_LIBVMAF;
        switch (c.first.mc) {
        case MatrixCoefficients::BT709: return TM_CIEDE_BT709;
        case MatrixCoefficients::BT601_525: case MatrixCoefficients::BT601_625: return TM_CIEDE_BT601;
        default: throw std::runtime_error(std::string("ciede2000: not implemented: matrix coefficients ") + to_string(c.first.mc));
        }
    }
    void push(const HwFrame &r, const HwFrame &d, const ColorInfo &cr, const ColorInfo &cd)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd) throw std::runtime_error("ciede2000 needs reference and distorted in the same YUV layout and bit depth");
        const int mr = matrix_of(cr), md = matrix_of(cd);
        if (mr != md) throw std::runtime_error("ciede2000 needs reference and distorted with the same matrix coefficients");
        if (!x) {
            layout = lr; bits = br; matrix = mr;
            const int rc = create(&x, w, h, layout, bits, matrix, libvmaf ? 0.65 : 1.0, 1.0, libvmaf ? 4.0 : 1.0, 0, map_prefix.empty() ? 0 : 1, batch);
            if (rc == TM_ERR_UNSUPPORTED) throw std::runtime_error("ciede2000 takes pictures of 2 x 2 to 32768 x 32768 samples");
            chk(rc, "tm_ciede_create");
        } else if (lr != layout || br != bits || mr != matrix) {
            throw std::runtime_error("ciede2000: the YUV layout or the matrix changed inside the stream");
        }
        const bool bi = layout == TM_CIEDE_NV12 || layout == TM_CIEDE_P016;
        int side = TM_SIDE_REF;
        for (const HwFrame *f : {&r, &d}) {
            chk(set_frame(x, filled, side, f->data, bi ? f->uv : f->u, bi ? nullptr : f->v, f->pitch, bi ? f->pitch : f->pitch_uv,
                          f->device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_ciede_set_frame");
            side = TM_SIDE_DIS;
        }
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(x, filled), "tm_ciede_compute_async");
        chk(sync(x), "tm_ciede_sync");
        std::vector<tm_ciede_frame> out(filled);
        chk(get(x, 0, filled, out.data()), "tm_ciede_get");
        for (uint32_t i = 0; i < filled; ++i) {
            const tm_ciede_frame &f = out[i];
            ready.push_back({f.score, f.de_mean});
            sum_de += f.de_sum;
            sum_px += f.pixels;
            if (map_prefix.empty()) continue;
            map.resize((size_t)w * h);
            chk(get_map(x, i, map.data(), (size_t)w * sizeof(float)), "tm_ciede_get_map");
            char num[32];
            snprintf(num, sizeof num, "%06zu.pfm", written++);
            write_pfm_gray(map_prefix + num, w, h, map.data());
        }
        filled = 0;
    }
    std::array<double, 2> pop()
    {
        if (ready.empty()) throw std::logic_error("ciede2000: a pair's result is missing");
        const std::array<double, 2> v = ready.front();
        ready.pop_front();
        return v;
    }
    // the sequence value of column k (kCiedeNames)
    double sequence_score(int k) const { return k ? sum_de / (double)sum_px : score(sum_de, sum_px); }
};

// ---- VIF -----------------------------------------------------------------------------------------------------------
// libturbometrics_vif.so, loaded at run time like the XPSNR and motion libraries (a CLI run without -m vif never loads it).  The lumas
// of every kept pair are handed over as TM_MEM_HOST copies and computed batch by batch in stream order; a pair's five scores wait in
// `ready` until the engine's scores of the same pair are drained.  No history: --every is fine.
struct VifRun {
    void *lib = nullptr;
    int (*create)(tm_vif **, uint32_t, uint32_t, int, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_vif *) = nullptr;
    int (*set_pair)(tm_vif *, uint32_t, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_vif *, uint32_t) = nullptr;
    int (*sync)(tm_vif *) = nullptr;
    int (*get)(tm_vif *, uint32_t, uint32_t, tm_vif_frame *) = nullptr;
    void (*scores)(const tm_vif_frame *, double *) = nullptr;
    tm_vif *v = nullptr;
    uint32_t w, h, batch;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    std::deque<std::array<double, 5>> ready;

    VifRun(uint32_t w_, uint32_t h_, uint32_t batch_) : w(w_), h(h_), batch(batch_)
    {
        const char *path = getenv("TM_VIF_LIB");
        lib = dlopen(path ? path : "libturbometrics_vif.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m vif needs libturbometrics_vif.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_vif_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_vif_destroy");
        set_pair = (decltype(set_pair))dlsym(lib, "tm_vif_set_pair");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_vif_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_vif_sync");
        get = (decltype(get))dlsym(lib, "tm_vif_get");
        scores = (decltype(scores))dlsym(lib, "tm_vif_scores");
        if (!create || !destroy || !set_pair || !compute_async || !sync || !get || !scores)
            throw std::runtime_error("libturbometrics_vif.so does not export include/turbo_metrics_vif.h");
    }
    ~VifRun()
    {
        if (v) destroy(v);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &l, uint32_t &b)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: l = TM_VIF_Y8; b = 8; return;
        case HwFrame::NvDecP016: l = TM_VIF_Y16_MSB; b = 10; return;
        case HwFrame::Planar420: b = (uint32_t)f.bits; l = b == 8 ? TM_VIF_Y8 : TM_VIF_Y16_LOW; return;
        case HwFrame::Planar420P10: l = TM_VIF_Y10_PACKED; b = 10; return;
        default: throw std::runtime_error("vif needs YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    void push(const HwFrame &r, const HwFrame &d)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd || r.device != d.device) throw std::runtime_error("vif needs reference and distorted in the same YUV layout and bit depth");
        if (!v) {
            layout = lr; bits = br;
            chk(create(&v, w, h, layout, bits, batch), "tm_vif_create");
        } else if (lr != layout || br != bits) {
            throw std::runtime_error("vif: the YUV layout changed inside the stream");
        }
        chk(set_pair(v, filled, r.data, d.data, r.pitch, d.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_vif_set_pair");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(v, filled), "tm_vif_compute_async");
        chk(sync(v), "tm_vif_sync");
        std::vector<tm_vif_frame> out(filled);
        chk(get(v, 0, filled, out.data()), "tm_vif_get");
        for (const tm_vif_frame &f : out) {
            std::array<double, 5> s;
            scores(&f, s.data());
            ready.push_back(s);
        }
        filled = 0;
    }
    std::array<double, 5> pop()
    {
        if (ready.empty()) throw std::logic_error("vif: a pair's result is missing");
        const std::array<double, 5> s = ready.front();
        ready.pop_front();
        return s;
    }
};

// ---- ADM -----------------------------------------------------------------------------------------------------------
// libturbometrics_adm.so, loaded at run time like the XPSNR, motion and VIF libraries (a CLI run without -m adm never loads it).  The
// lumas of every kept pair are handed over as TM_MEM_HOST copies and computed batch by batch in stream order; a pair's five scores
// (adm_scale0 .. adm_scale3, adm2) wait in `ready` until the engine's scores of the same pair are drained.  No history: --every is fine.
struct AdmRun {
    void *lib = nullptr;
    int (*create)(tm_adm **, uint32_t, uint32_t, int, uint32_t, uint32_t) = nullptr;
    void (*destroy)(tm_adm *) = nullptr;
    int (*set_pair)(tm_adm *, uint32_t, const void *, const void *, size_t, size_t, int) = nullptr;
    int (*compute_async)(tm_adm *, uint32_t) = nullptr;
    int (*sync)(tm_adm *) = nullptr;
    int (*get)(tm_adm *, uint32_t, uint32_t, tm_adm_frame *) = nullptr;
    void (*scores)(const tm_adm_frame *, uint32_t, uint32_t, double *) = nullptr;
    tm_adm *v = nullptr;
    uint32_t w, h, batch;
    int layout = -1;
    uint32_t bits = 8, filled = 0;
    std::deque<std::array<double, 5>> ready;

    AdmRun(uint32_t w_, uint32_t h_, uint32_t batch_) : w(w_), h(h_), batch(batch_)
    {
        const char *path = getenv("TM_ADM_LIB");
        lib = dlopen(path ? path : "libturbometrics_adm.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) throw std::runtime_error(std::string("-m adm needs libturbometrics_adm.so: ") + dlerror());
        create = (decltype(create))dlsym(lib, "tm_adm_create");
        destroy = (decltype(destroy))dlsym(lib, "tm_adm_destroy");
        set_pair = (decltype(set_pair))dlsym(lib, "tm_adm_set_pair");
        compute_async = (decltype(compute_async))dlsym(lib, "tm_adm_compute_async");
        sync = (decltype(sync))dlsym(lib, "tm_adm_sync");
        get = (decltype(get))dlsym(lib, "tm_adm_get");
        scores = (decltype(scores))dlsym(lib, "tm_adm_scores");
        if (!create || !destroy || !set_pair || !compute_async || !sync || !get || !scores)
            throw std::runtime_error("libturbometrics_adm.so does not export include/turbo_metrics_adm.h");
    }
    ~AdmRun()
    {
        if (v) destroy(v);
        if (lib) dlclose(lib);
    }
    static void layout_of(const HwFrame &f, int &l, uint32_t &b)
    {
        switch (f.kind) {
        case HwFrame::NvDecNV12: l = TM_ADM_Y8; b = 8; return;
        case HwFrame::NvDecP016: l = TM_ADM_Y16_MSB; b = 10; return;
        case HwFrame::Planar420: b = (uint32_t)f.bits; l = b == 8 ? TM_ADM_Y8 : TM_ADM_Y16_LOW; return;
        case HwFrame::Planar420P10: l = TM_ADM_Y10_PACKED; b = 10; return;
        default: throw std::runtime_error("adm needs YUV input (Y4M, raw planar YUV or decoded video), not RGB images");
        }
    }
    void push(const HwFrame &r, const HwFrame &d)
    {
        int lr, ld;
        uint32_t br, bd;
        layout_of(r, lr, br);
        layout_of(d, ld, bd);
        if (lr != ld || br != bd || r.device != d.device) throw std::runtime_error("adm needs reference and distorted in the same YUV layout and bit depth");
        if (!v) {
            layout = lr; bits = br;
            chk(create(&v, w, h, layout, bits, batch), "tm_adm_create");
        } else if (lr != layout || br != bits) {
            throw std::runtime_error("adm: the YUV layout changed inside the stream");
        }
        chk(set_pair(v, filled, r.data, d.data, r.pitch, d.pitch, r.device ? TM_MEM_DEVICE : TM_MEM_HOST), "tm_adm_set_pair");
        ++filled;
    }
    void flush()
    {
        if (!filled) return;
        chk(compute_async(v, filled), "tm_adm_compute_async");
        chk(sync(v), "tm_adm_sync");
        std::vector<tm_adm_frame> out(filled);
        chk(get(v, 0, filled, out.data()), "tm_adm_get");
        for (const tm_adm_frame &f : out) {
            std::array<double, 5> s;
            scores(&f, w, h, s.data());
            ready.push_back(s);
        }
        filled = 0;
    }
    std::array<double, 5> pop()
    {
        if (ready.empty()) throw std::logic_error("adm: a pair's result is missing");
        const std::array<double, 5> s = ready.front();
        ready.pop_front();
        return s;
    }
};

void TurboMetrics::set_xpsnr_fps(uint32_t num, uint32_t den)
{
    if (!xp_) throw std::runtime_error("xpsnr was not selected");
    if (num == 0 || den == 0) throw TmError(TM_ERR_INVALID_ARG, "set_xpsnr_fps");
    xp_->fps_num = num;
    xp_->fps_den = den;
}

// ---- engine --------------------------------------------------------------------------------------------------------
TurboMetrics::TurboMetrics(uint32_t width, uint32_t height, const Metrics &metrics, uint32_t batch, bool pipeline)
    : w_(width), h_(height), batch_(batch ? batch : 1), metrics_(metrics)
{
    if (metrics_.xpsnr) xp_ = std::make_unique<XpsnrRun>(w_, h_, batch_);
    if (metrics_.motion) mo_ = std::make_unique<MotionRun>(w_, h_, batch_);
    if (metrics_.siti) si_ = std::make_unique<SitiRun>(w_, h_, batch_, metrics_.siti_gain);
    if (metrics_.vif) vf_ = std::make_unique<VifRun>(w_, h_, batch_);
    if (metrics_.adm) ad_ = std::make_unique<AdmRun>(w_, h_, batch_);
    if (metrics_.scenes) sc_ = std::make_unique<SceneRun>(w_, h_, batch_, metrics_.scene_bins, metrics_.scene_threshold);
    if (metrics_.cambi) cb_ = std::make_unique<CambiRun>(w_, h_, batch_, metrics_.cambi_window, metrics_.cambi_topk);
    if (metrics_.cambi && metrics_.cambi_ref) cbr_ = std::make_unique<CambiRun>(w_, h_, batch_, metrics_.cambi_window, metrics_.cambi_topk);
    if (metrics_.flip) fl_ = std::make_unique<FlipRun>(w_, h_, batch_, metrics_.flip_ppd, metrics_.flip_map);
    if (metrics_.psnr_yuv || metrics_.ssim_yuv) yv_ = std::make_unique<YuvRun>(w_, h_, batch_, metrics_.psnr_yuv_cap, metrics_.ssim_yuv_map);
    if (metrics_.psnr_hvs || metrics_.psnr_hvs_m) hv_ = std::make_unique<HvsRun>(w_, h_, batch_);
    if (metrics_.ciede) ci_ = std::make_unique<CiedeRun>(w_, h_, batch_, metrics_.ciede_libvmaf, metrics_.ciede_map);
    if (metrics_.gmsd) gm_ = std::make_unique<GmsdRun>(w_, h_, batch_, metrics_.gmsd_population, metrics_.gmsd_map);
    if (metrics_.haarpsi) hp_ = std::make_unique<HaarpsiRun>(w_, h_, batch_, metrics_.haarpsi_map);
    if (metrics_.deitp) it_ = std::make_unique<ItpRun>(w_, h_, batch_, metrics_.itp_hlg, metrics_.itp_map);
    if (metrics_.mdsi) md_ = std::make_unique<MdsiRun>(w_, h_, batch_, metrics_.mdsi_factor, metrics_.mdsi_map);
    if (metrics_.mask() == 0 && (metrics_.xpsnr || metrics_.motion || metrics_.vif || metrics_.adm || metrics_.scenes || metrics_.cambi || metrics_.flip || yv_ || hv_ || ci_ || si_ || gm_ || hp_ || it_ || md_)) return; // -m xpsnr, -m vif, -m adm, --motion or --scenes alone: no SSIMULACRA2 / PSNR engine at all
    chk(tm_engine_create(&eng_[0], w_, h_, metrics_.mask(), batch_), "tm_engine_create");
    if (pipeline) {
        const int rc = tm_engine_create(&eng_[1], w_, h_, metrics_.mask(), batch_);
        if (rc != TM_OK) {
            tm_engine_destroy(eng_[0]);
            eng_[0] = nullptr;
            throw TmError(rc, "tm_engine_create (second engine of the pipeline)");
        }
    }
    // compute_all hands pictures over one by one, as they arrive, with a fence per pair: for that pattern a picture of a planar file is
    // fastest as one linear copy (the library's default suits callers that queue whole batches; tm_engine.hip, set_frame_planar)
    for (tm_engine *e : eng_)
        if (e) (void)tm_engine_set_linear_upload(e, 1);
}

TurboMetrics::~TurboMetrics()
{
    for (tm_engine *e : eng_)
        if (e) tm_engine_destroy(e);
}

size_t TurboMetrics::mem_usage() const
{
    size_t total = 0;
    for (tm_engine *e : eng_)
        if (e) total += tm_engine_mem_usage(e);
    return total;
}

// tm_engine_debug_set_param is a function of the LABORATORY build (include/turbo_metrics_hip_debug.h): the ship library this file links
// does not export it.  A measurement run puts the laboratory build in front (LD_PRELOAD=turbo-metrics_amd/lab/libturbometrics_hip_lab.so,
// tools/cli_ab.sh); the CLI's --tune says so otherwise.
using debug_set_param_fn = int (*)(tm_engine *, int, long long);
static debug_set_param_fn lab_set_param()
{
    static const debug_set_param_fn fn = (debug_set_param_fn)dlsym(RTLD_DEFAULT, "tm_engine_debug_set_param");
    return fn;
}

void TurboMetrics::debug_set_param(int param, long long value)
{
    if (!lab_set_param()) throw std::runtime_error("tuning values belong to the laboratory build: run with LD_PRELOAD=<...>/turbo-metrics_amd/lab/libturbometrics_hip_lab.so");
    retire_deferred(); // a setting never changes under a pair in flight: its scores are collected first
    debug_params_.emplace_back(param, value);
    for (tm_engine *e : eng_)
        if (e) chk(lab_set_param()(e, param, value), "tm_engine_debug_set_param");
}

void TurboMetrics::set_full_sums(bool on)
{
    retire_deferred(); // tm_engine_set_full_sums drops the engine's results: a pair in flight keeps its scores for collect()
    full_sums_ = on; // (an engine created later -- compute_one_deferred's second one -- starts with it)
    for (tm_engine *e : eng_)
        if (e) chk(tm_engine_set_full_sums(e, on ? 1 : 0), "tm_engine_set_full_sums");
}

// == convert_frame_to_linearrgb (color.rs:96-116): kernel selection by frame kind and colour metadata
void TurboMetrics::set_frame(tm_engine *e, uint32_t slot, int side, const HwFrame &f, const ColorInfo &c)
{
    const int mem = f.device ? TM_MEM_DEVICE : (f.pinned ? TM_MEM_HOST_PINNED : TM_MEM_HOST);
    switch (f.kind) {
    case HwFrame::NvDecNV12:
    case HwFrame::NvDecP016: {
        const int matrix = get_color_matrix(c.first), transfer = get_transfer(c.first);
        const int full = c.second == ColorRange::Full ? 1 : 0;
        if (f.kind == HwFrame::NvDecNV12)
            chk(tm_engine_set_frame_nv12(e, slot, side, f.data, f.uv, f.pitch, matrix, transfer, full, mem), "tm_engine_set_frame_nv12");
        else
            chk(tm_engine_set_frame_p016(e, slot, side, f.data, f.uv, f.pitch, matrix, transfer, full, mem), "tm_engine_set_frame_p016");
        break;
    }
    case HwFrame::Planar420: {
        const int matrix = get_color_matrix(c.first), transfer = get_transfer(c.first);
        const int full = c.second == ColorRange::Full ? 1 : 0;
        chk(tm_engine_set_frame_i420(e, slot, side, f.data, f.u, f.v, f.pitch, f.pitch_uv, f.bits, matrix, transfer, full, mem), "tm_engine_set_frame_i420");
        break;
    }
    case HwFrame::Planar420P10: {
        const int matrix = get_color_matrix(c.first), transfer = get_transfer(c.first);
        const int full = c.second == ColorRange::Full ? 1 : 0;
        chk(tm_engine_set_frame_i420p10(e, slot, side, f.data, f.u, f.v, f.pitch, f.pitch_uv, matrix, transfer, full, mem), "tm_engine_set_frame_i420p10");
        break;
    }
    case HwFrame::Npp8: chk(tm_engine_set_frame_rgb8(e, slot, side, f.data, f.pitch, mem), "tm_engine_set_frame_rgb8"); break;
    case HwFrame::Npp16: chk(tm_engine_set_frame_rgb16(e, slot, side, f.data, f.pitch, mem), "tm_engine_set_frame_rgb16"); break;
    case HwFrame::Npp32: chk(tm_engine_set_frame_rgbf32(e, slot, side, f.data, f.pitch, mem), "tm_engine_set_frame_rgbf32"); break;
    }
}

FrameScores TurboMetrics::scores_of(tm_engine *e, uint32_t slot)
{
    tm_frame_scores s;
    chk(tm_engine_get_scores(e, slot, &s), "tm_engine_get_scores");
    FrameScores r;
    if (s.valid & TM_METRIC_PSNR) r.psnr = s.psnr;
    if (s.valid & TM_METRIC_SSIM) r.ssim = s.ssim;
    if (s.valid & TM_METRIC_MSSSIM) r.msssim = s.msssim;
    if (s.valid & TM_METRIC_SSIMULACRA2) r.ssimulacra2 = s.ssimulacra2;
    return r;
}

void TurboMetrics::create_deferred_engine(size_t i)
{
    if (eng_[i]) return;
    chk(tm_engine_create(&eng_[i], w_, h_, metrics_.mask(), 1), "tm_engine_create (further engine of compute_one_deferred)");
    (void)tm_engine_set_linear_upload(eng_[i], 1);
    if (full_sums_) chk(tm_engine_set_full_sums(eng_[i], 1), "tm_engine_set_full_sums");
    for (const auto &kv : debug_params_) (void)lab_set_param()(eng_[i], kv.first, kv.second); // (only ever non-empty with the laboratory build loaded)
}

void TurboMetrics::set_deferred_depth(uint32_t depth, bool create_now)
{
    if (depth < 2 || depth > MAX_DEFERRED_DEPTH) throw TmError(TM_ERR_INVALID_ARG, "set_deferred_depth: 2 ... 8 pairs in flight");
    retire_deferred();
    for (size_t i = std::max<size_t>(2, depth); i < eng_.size(); ++i)
        if (eng_[i]) tm_engine_destroy(eng_[i]);
    eng_.resize(std::max<size_t>(2, depth), nullptr);
    def_pending_.assign(depth, 0);
    def_depth_ = depth;
    if (create_now) {
        if (batch_ != 1) throw TmError(TM_ERR_INVALID_ARG, "compute_one_deferred: create the TurboMetrics object with batch = 1");
        for (size_t i = 1; i < depth; ++i) create_deferred_engine(i);
    }
}

void TurboMetrics::retire_deferred()
{
    for (size_t i = 0; i < def_pending_.size(); ++i)
        if (def_pending_[i]) {
            chk(tm_engine_sync(eng_[i]), "tm_engine_sync");
            def_done_.emplace_back(def_pending_[i], scores_of(eng_[i], 0));
            def_pending_[i] = 0;
        }
}

FrameScores TurboMetrics::compute_one(const HwFrame &fref, const ColorInfo &cref, const HwFrame &fdis, const ColorInfo &cdis)
{
    retire_deferred(); // (slot 0 of this engine may hold a deferred pair)
    set_frame(eng_[0], 0, TM_SIDE_REF, fref, cref);
    set_frame(eng_[0], 0, TM_SIDE_DIS, fdis, cdis);
    chk(tm_engine_compute_async(eng_[0], 1), "tm_engine_compute_async");
    chk(tm_engine_sync(eng_[0]), "tm_engine_sync");
    return scores_of(eng_[0], 0);
}

uint64_t TurboMetrics::compute_one_deferred(const HwFrame &fref, const ColorInfo &cref, const HwFrame &fdis, const ColorInfo &cdis)
{
    // the one-pair-per-call path, as in the Python mirror: on a batched object the lazily created second engine would cost a whole
    // batch of device memory for one-pair launches
    if (batch_ != 1) throw TmError(TM_ERR_INVALID_ARG, "compute_one_deferred: create the TurboMetrics object with batch = 1");
    const uint64_t ticket = def_next_++;
    const size_t i = (size_t)(ticket % def_depth_);
    create_deferred_engine(i); // (the engines the launches take turns on are created when their turn first comes, unless set_deferred_depth made them)
    if (def_pending_[i]) { // `depth` pairs are in flight already: the oldest one (on this engine) is finished first
        chk(tm_engine_sync(eng_[i]), "tm_engine_sync");
        def_done_.emplace_back(def_pending_[i], scores_of(eng_[i], 0));
        def_pending_[i] = 0;
    }
    set_frame(eng_[i], 0, TM_SIDE_REF, fref, cref);
    set_frame(eng_[i], 0, TM_SIDE_DIS, fdis, cdis);
    chk(tm_engine_compute_async(eng_[i], 1), "tm_engine_compute_async");
    def_pending_[i] = ticket;
    return ticket;
}

FrameScores TurboMetrics::collect(uint64_t ticket)
{
    for (size_t i = 0; i < def_pending_.size(); ++i)
        if (ticket && def_pending_[i] == ticket) {
            def_pending_[i] = 0;
            chk(tm_engine_sync(eng_[i]), "tm_engine_sync");
            return scores_of(eng_[i], 0);
        }
    for (size_t k = 0; k < def_done_.size(); ++k)
        if (def_done_[k].first == ticket) {
            FrameScores r = def_done_[k].second;
            def_done_.erase(def_done_.begin() + (long)k);
            return r;
        }
    throw TmError(TM_ERR_INVALID_ARG, "collect: no such ticket (never issued, or collected already)");
}

MetricsResults aggregate_scores(const std::vector<FrameScores> &frames, const Metrics &metrics)
{
    std::optional<std::vector<double>> a, b, c, d;
    if (metrics.psnr) a.emplace();
    if (metrics.ssim) b.emplace();
    if (metrics.msssim) c.emplace();
    if (metrics.ssimulacra2) d.emplace();
    for (const FrameScores &r : frames) {
        if (a && r.psnr) a->push_back(*r.psnr);
        if (b && r.ssim) b->push_back(*r.ssim);
        if (c && r.msssim) c->push_back(*r.msssim);
        if (d && r.ssimulacra2) d->push_back(*r.ssimulacra2);
    }
    MetricsResults res;
    res.frame_count = frames.size();
    if (frames.empty() && (a || b || c || d))
        throw NoFramesSelected();
    if (a) res.psnr = MetricAggregate::from(std::move(*a));
    if (b) res.ssim = MetricAggregate::from(std::move(*b));
    if (c) res.msssim = MetricAggregate::from(std::move(*c));
    if (d) res.ssimulacra2 = MetricAggregate::from(std::move(*d));
    return res;
}

// A page-locked frame is pulled into an engine-owned device surface by an asynchronous DMA; its bytes are free again when THAT
// copy is done (tm_engine_upload_fence / tm_engine_upload_done), not when its batch has been computed: a frame has to survive
// only UPLOADS_IN_FLIGHT further next_frame calls, whatever the batch size -- the sources' rings of page-locked surfaces stay
// small (round 3: 2 * batch + 1 surfaces per stream; page-locking them, at ~3 GB/s, was most of a short 4K run and the reason
// why --batch 16 was slower than --batch 8)
// (Up to 16 pairs in flight with a fence per 4 was measured too -- TurboMetrics::set_upload_tuning, `--tune 100=16 --tune 101=4`: the loop
// then waits for the readers instead of the uploads and ends within the run-to-run spread of the default, 7.06 k vs 6.69 k pairs/s on one
// box, 5.87 k vs 6.04 k on another; profiles/r04y_cli_ab2.log, r04y_cli_ab3.log -- the small ring kept.)
// (Round 6: the engine sends page-locked pictures that lie back to back in the source's ring up as ONE DMA, up to 14 MB of them, and every fence
// flushes what it holds back: pictures of up to 1080p 8-bit get a fence per 4 pairs with 8 pairs in flight -- 7.84-7.92 k -> 8.08-8.21 k pairs/s,
// profiles/r06o_cli_fence_ab.log --; larger ones are a DMA each and keep the small ring.)
static size_t UPLOADS_IN_FLIGHT = 4; // pairs whose uploads may be in flight behind the one being read (the sources' lookahead)
static size_t FENCE_EVERY = 1;       // pairs per fence
static bool UPLOAD_TUNING_SET = false;
void TurboMetrics::set_upload_tuning(size_t in_flight, size_t fence_every)
{
    FENCE_EVERY = std::max<size_t>(1, fence_every);
    UPLOADS_IN_FLIGHT = std::max(std::max<size_t>(in_flight ? 1 : 4, in_flight), FENCE_EVERY);
    UPLOAD_TUNING_SET = true;
}

void TurboMetrics::prepare_sources(FrameSource &frames_ref, FrameSource &frames_dis, const Options &opts, size_t min_lookahead)
{
    if (!UPLOAD_TUNING_SET) {
        const bool small = (size_t)frames_ref.width() * frames_ref.height() <= (size_t)1920 * 1088 * 2; // pictures of which several fit one DMA
        UPLOADS_IN_FLIGHT = small ? 8 : 4;
        FENCE_EVERY = small ? 4 : 1;
    }
    for (FrameSource *s : {&frames_ref, &frames_dis}) {
        s->set_lookahead(std::max(UPLOADS_IN_FLIGHT, min_lookahead));
        s->set_readahead(opts.every <= 1); // dropped pictures are consumed without being read: no reading ahead then
        s->prepare();
    }
}

MetricsResults TurboMetrics::compute_all(FrameSource &frames_ref, FrameSource &frames_dis, const Options &opts,
                                         const std::function<void(const FrameScores &)> &on_frame, uint32_t *decode_count_out)
{
    if (frames_ref.width() != frames_dis.width() || frames_ref.height() != frames_dis.height())
        throw std::runtime_error("Reference and distorted are not the same size"); // assert_eq! at lib.rs:368-372
    const ColorInfo cref = frames_ref.color_characteristics(), cdis = frames_dis.color_characteristics();
    retire_deferred(); // (the engines' slots may hold deferred pairs)

    std::optional<std::vector<double>> s_psnr, s_ssim, s_msssim, s_ssimu;
    if (metrics_.psnr) s_psnr.emplace();
    if (metrics_.ssim) s_ssim.emplace();
    if (metrics_.msssim) s_msssim.emplace();
    if (metrics_.ssimulacra2) s_ssimu.emplace();

    uint32_t decode_count = opts.decode_start;
    size_t compute_count = 0;
    timing_ = LoopTiming{};
    const auto tick = [] { return std::chrono::steady_clock::now(); };
    const auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    prepare_sources(frames_ref, frames_dis, opts); // (no-ops when the caller has done it already)
    struct Fence { tm_engine *e = nullptr; uint64_t token = 0; };
    std::vector<Fence> fences(UPLOADS_IN_FLIGHT + FENCE_EVERY + 2); // [pair % size]: the fence that covers the pair's uploads
    size_t first_unfenced = 0;                                      // pairs [first_unfenced, kept) have no fence yet (fewer than FENCE_EVERY, all on eng_[cur])
    size_t kept = 0; // pairs handed to an engine so far
    frames_ref.skip_frames(opts.skip_ref + opts.skip + opts.decode_start);
    frames_dis.skip_frames(opts.skip_dis + opts.skip + opts.decode_start);

    // A batch in flight on engine `cur` while the next one is being read and uploaded into the other engine.
    uint32_t filled[2] = {0, 0};
    bool in_flight[2] = {false, false};
    int cur = 0;
    std::optional<std::vector<double>> s_xp[3];
    if (xp_)
        for (auto &v : s_xp) v.emplace();
    // --motion: motion2 of a pair needs the next pair's motion, so a pair's row is held until the next one is drained (or the stream ends)
    std::optional<std::vector<double>> s_mo, s_mo2;
    if (mo_) { s_mo.emplace(); s_mo2.emplace(); }
    std::optional<std::vector<double>> s_vf[5];
    if (vf_)
        for (auto &v : s_vf) v.emplace();
    std::optional<std::vector<double>> s_ad[5]; // adm_scale0 .. adm_scale3, adm2
    if (ad_)
        for (auto &v : s_ad) v.emplace();
    std::optional<std::vector<double>> s_sc; // --scenes: the scores, and the frames at which a scene starts
    std::vector<size_t> scene_starts;
    if (sc_) s_sc.emplace();
    std::optional<std::vector<double>> s_cb[6], s_cbr[6]; // cambi_scale0 .. cambi_scale4, cambi; the reference stream's
    if (cb_)
        for (auto &v : s_cb) v.emplace();
    if (cbr_)
        for (auto &v : s_cbr) v.emplace();
    std::optional<std::vector<double>> s_fl[3]; // flip, flip_min, flip_max
    if (fl_)
        for (auto &v : s_fl) v.emplace();
    std::optional<std::vector<double>> s_yv[8]; // kYuvNames: [0 .. 3] with psnr-yuv, [4 .. 7] with ssim-yuv
    for (int k = 0; k < 8; ++k)
        if (k < 4 ? metrics_.psnr_yuv : metrics_.ssim_yuv) s_yv[k].emplace();
    std::optional<std::vector<double>> s_hv[2]; // kHvsNames
    if (metrics_.psnr_hvs) s_hv[0].emplace();
    if (metrics_.psnr_hvs_m) s_hv[1].emplace();
    std::optional<std::vector<double>> s_ci[2]; // kCiedeNames
    if (metrics_.ciede) { s_ci[0].emplace(); s_ci[1].emplace(); }
    std::optional<std::vector<double>> s_si, s_ti; // --siti: every frame's si and ti (the first picture's ti: 0)
    std::vector<double> ti_valid;                  // ... and the ti values its statistics are of: the first picture has none
    if (si_) { s_si.emplace(); s_ti.emplace(); }
    std::optional<std::vector<double>> s_gm[2]; // kGmsdNames
    if (gm_) { s_gm[0].emplace(); s_gm[1].emplace(); }
    std::optional<std::vector<double>> s_hp;
    if (hp_) s_hp.emplace();
    std::optional<std::vector<double>> s_it[2]; // kItpNames
    if (it_) { s_it[0].emplace(); s_it[1].emplace(); }
    std::optional<std::vector<double>> s_md;
    if (md_) s_md.emplace();
    std::optional<FrameScores> held;
    auto emit = [&](const FrameScores &r) {
        if (on_frame) on_frame(r);
        if (s_psnr && r.psnr) s_psnr->push_back(*r.psnr);
        if (s_ssim && r.ssim) s_ssim->push_back(*r.ssim);
        if (s_msssim && r.msssim) s_msssim->push_back(*r.msssim);
        if (s_ssimu && r.ssimulacra2) s_ssimu->push_back(*r.ssimulacra2);
        if (s_mo) { s_mo->push_back(*r.motion); s_mo2->push_back(*r.motion2); }
        if (s_sc) {
            s_sc->push_back(*r.scene_score);
            if (compute_count == 0 || *r.scene_cut) scene_starts.push_back(compute_count);
        }
        if (s_si) {
            s_si->push_back(*r.si);
            s_ti->push_back(*r.ti);
            if (r.ti_valid) ti_valid.push_back(*r.ti);
        }
        ++compute_count;
    };
    auto drain = [&](int i) {
        if (!in_flight[i]) return;
        if (eng_[i]) chk(tm_engine_sync(eng_[i]), "tm_engine_sync");
        for (uint32_t slot = 0; slot < filled[i]; ++slot) {
            FrameScores r = eng_[i] ? scores_of(eng_[i], slot) : FrameScores{};
            if (xp_) { // (its batch was computed when the engine's was submitted: in stream order, ready)
                const std::array<double, 3> v = xp_->pop();
                r.xpsnr_y = v[0]; r.xpsnr_u = v[1]; r.xpsnr_v = v[2];
                for (int c = 0; c < 3; ++c) s_xp[c]->push_back(v[c]);
            }
            if (vf_) {
                const std::array<double, 5> v = vf_->pop();
                for (int k = 0; k < 4; ++k) r.vif_scale[k] = v[k];
                r.vif = v[4];
                for (int k = 0; k < 5; ++k) s_vf[k]->push_back(v[k]);
            }
            if (ad_) {
                const std::array<double, 5> v = ad_->pop();
                for (int k = 0; k < 4; ++k) r.adm_scale[k] = v[k];
                r.adm2 = v[4];
                for (int k = 0; k < 5; ++k) s_ad[k]->push_back(v[k]);
            }
            if (sc_) {
                const std::pair<double, bool> v = sc_->pop();
                r.scene_score = v.first;
                r.scene_cut = v.second;
            }
            if (cb_) {
                const std::array<double, 6> v = cb_->pop();
                for (int k = 0; k < 5; ++k) r.cambi_scale[k] = v[k];
                r.cambi = v[5];
                for (int k = 0; k < 6; ++k) s_cb[k]->push_back(v[k]);
            }
            if (cbr_) {
                const std::array<double, 6> v = cbr_->pop();
                for (int k = 0; k < 5; ++k) r.cambi_ref_scale[k] = v[k];
                r.cambi_ref = v[5];
                for (int k = 0; k < 6; ++k) s_cbr[k]->push_back(v[k]);
            }
            if (fl_) {
                const std::array<double, 3> v = fl_->pop();
                r.flip = v[0]; r.flip_min = v[1]; r.flip_max = v[2];
                for (int k = 0; k < 3; ++k) s_fl[k]->push_back(v[k]);
            }
            if (yv_) {
                const std::array<double, 8> v = yv_->pop();
                for (int k = 0; k < 8; ++k)
                    if (s_yv[k]) { r.yuv[k] = v[k]; s_yv[k]->push_back(v[k]); }
            }
            if (hv_) {
                const std::array<double, 2> v = hv_->pop();
                for (int k = 0; k < 2; ++k)
                    if (s_hv[k]) { r.hvs[k] = v[k]; s_hv[k]->push_back(v[k]); }
            }
            if (ci_) {
                const std::array<double, 2> v = ci_->pop();
                for (int k = 0; k < 2; ++k) { r.ciede[k] = v[k]; s_ci[k]->push_back(v[k]); }
            }
            if (si_) {
                const SitiRun::Value v = si_->pop();
                r.si = v.si; r.ti = v.ti; r.ti_valid = v.ti_valid;
            }
            if (gm_) {
                const std::array<double, 2> v = gm_->pop();
                for (int k = 0; k < 2; ++k) { r.gmsd[k] = v[k]; s_gm[k]->push_back(v[k]); }
            }
            if (hp_) {
                r.haarpsi = hp_->pop();
                s_hp->push_back(*r.haarpsi);
            }
            if (it_) {
                const std::array<double, 2> v = it_->pop();
                for (int k = 0; k < 2; ++k) { r.deitp[k] = v[k]; s_it[k]->push_back(v[k]); }
            }
            if (md_) {
                r.mdsi = md_->pop();
                s_md->push_back(*r.mdsi);
            }
            if (mo_) {
                r.motion = mo_->pop();
                if (held) {
                    held->motion2 = mo_->motion2(*held->motion, *r.motion);
                    emit(*held);
                }
                held = r;
            } else {
                emit(r);
            }
        }
        in_flight[i] = false;
        filled[i] = 0;
    };
    auto submit = [&](int i) {
        if (filled[i] == 0) return;
        if (eng_[i]) chk(tm_engine_compute_async(eng_[i], filled[i]), "tm_engine_compute_async");
        if (xp_) xp_->flush();
        if (mo_) mo_->flush();
        if (vf_) vf_->flush();
        if (ad_) ad_->flush();
        if (sc_) sc_->flush();
        if (cb_) cb_->flush();
        if (cbr_) cbr_->flush();
        if (fl_) fl_->flush();
        if (yv_) yv_->flush();
        if (hv_) hv_->flush();
        if (ci_) ci_->flush();
        if (si_) si_->flush();
        if (gm_) gm_->flush();
        if (hp_) hp_->flush();
        if (it_) it_->flush();
        if (md_) md_->flush();
        in_flight[i] = true;
    };

    // the two sources are read concurrently: the reference stream on a helper thread, the distorted one here
    HwFrame fref, fdis;
    struct Fetch {
        std::mutex m;
        std::condition_variable cv;
        bool want = false, done = false, quit = false, ok = false, keep = true;
        std::exception_ptr err;
    } fx;
    std::thread helper([&] {
        std::unique_lock<std::mutex> lk(fx.m);
        for (;;) {
            fx.cv.wait(lk, [&] { return fx.want || fx.quit; });
            if (fx.quit) return;
            fx.want = false;
            const bool keep = fx.keep;
            lk.unlock();
            bool ok = false;
            std::exception_ptr err;
            try { ok = keep ? frames_ref.next_frame(fref) : frames_ref.skip_one(); } catch (...) { err = std::current_exception(); }
            lk.lock();
            fx.ok = ok; fx.err = err; fx.done = true;
            fx.cv.notify_all();
        }
    });
    struct Joiner {
        Fetch &f; std::thread &t;
        ~Joiner() { { std::lock_guard<std::mutex> g(f.m); f.quit = true; } f.cv.notify_all(); if (t.joinable()) t.join(); }
    } joiner{fx, helper};
    // keep = false: the pair is consumed but not handed out (dropped by `every`): no upload preparation, and the sources' rings of
    // page-locked surfaces do not advance -- a surface is only reused after `lookahead` KEPT frames, which is what the engines'
    // asynchronous DMA relies on
    auto next_pair = [&](bool keep) {
        { std::lock_guard<std::mutex> g(fx.m); fx.want = true; fx.done = false; fx.keep = keep; }
        fx.cv.notify_all();
        bool ok_dis = false;
        std::exception_ptr err_dis;
        try { ok_dis = keep ? frames_dis.next_frame(fdis) : frames_dis.skip_one(); } catch (...) { err_dis = std::current_exception(); }
        std::unique_lock<std::mutex> lk(fx.m);
        fx.cv.wait(lk, [&] { return fx.done; });
        if (fx.err) std::rethrow_exception(fx.err);
        if (err_dis) std::rethrow_exception(err_dis);
        return fx.ok && ok_dis;
    };
    for (;;) {
        const bool dropped = opts.every > 1 && decode_count != 0 && decode_count % opts.every != 0; // lib.rs:391-394
        auto t0 = tick();
        if (!dropped && kept > UPLOADS_IN_FLIGHT && eng_[0]) { // the call below may overwrite the surfaces of pair kept - UPLOADS_IN_FLIGHT - 1
            const Fence &f = fences[(kept - UPLOADS_IN_FLIGHT - 1) % fences.size()]; // (it has one: UPLOADS_IN_FLIGHT >= FENCE_EVERY)
            const int r = tm_engine_upload_done(f.e, f.token, 1);
            if (r < 0) chk(-r, "tm_engine_upload_done");
        }
        timing_.wait_upload += since(t0);
        t0 = tick();
        const bool more = next_pair(!dropped);
        timing_.wait_frames += since(t0);
        if (!more) break;
        if (dropped) {
            ++decode_count;
            continue;
        }
        if (opts.frames > 0 && decode_count >= opts.frames) break; // lib.rs:396-398
        ++decode_count;
        t0 = tick();
        if (xp_) xp_->push(fref, fdis);
        if (mo_) mo_->push(fref);
        if (vf_) vf_->push(fref, fdis);
        if (ad_) ad_->push(fref, fdis);
        if (sc_) sc_->push(fref);
        if (cb_) cb_->push(fdis);
        if (cbr_) cbr_->push(fref);
        if (fl_) fl_->push(fref, fdis);
        if (yv_) yv_->push(fref, fdis);
        if (hv_) hv_->push(fref, fdis);
        if (ci_) ci_->push(fref, fdis, cref, cdis);
        if (si_) si_->push(fref);
        if (gm_) gm_->push(fref, fdis);
        if (hp_) hp_->push(fref, fdis);
        if (it_) it_->push(fref, fdis, cref, cdis);
        if (md_) md_->push(fref, fdis, cref, cdis);
        if (eng_[cur]) {
            set_frame(eng_[cur], filled[cur], TM_SIDE_REF, fref, cref);
            set_frame(eng_[cur], filled[cur], TM_SIDE_DIS, fdis, cdis);
        }
        ++kept;
        if (eng_[cur] && (kept - first_unfenced >= FENCE_EVERY || filled[cur] + 1 == batch_)) { // (a fence covers one engine's uploads: never across a batch)
            Fence f;
            f.e = eng_[cur];
            chk(tm_engine_upload_fence(f.e, &f.token), "tm_engine_upload_fence");
            for (; first_unfenced < kept; ++first_unfenced) fences[first_unfenced % fences.size()] = f;
        }
        timing_.set_frames += since(t0);
        if (++filled[cur] == batch_) {
            t0 = tick();
            submit(cur);
            timing_.submit += since(t0);
            t0 = tick();
            if (eng_[1]) {
                cur ^= 1;
                drain(cur); // the batch submitted before this one: done (or nearly) while we were reading
            } else {
                drain(cur);
            }
            timing_.drain += since(t0);
        }
    }
    submit(cur);
    if (eng_[1]) drain(cur ^ 1);
    drain(cur);
    if (held) { // the last picture of the stream: its motion2 is its motion
        held->motion2 = held->motion;
        emit(*held);
        held.reset();
    }
    if (decode_count_out) *decode_count_out = decode_count;

    MetricsResults res;
    res.frame_count = compute_count;
    if (compute_count == 0 && (s_psnr || s_ssim || s_msssim || s_ssimu || xp_ || mo_ || vf_ || ad_ || sc_ || cb_ || fl_ || yv_ || hv_ || ci_ || si_ || gm_ || hp_ || it_ || md_))
        throw NoFramesSelected();
    if (xp_) {
        std::optional<MetricAggregate> *dst[3] = {&res.xpsnr_y, &res.xpsnr_u, &res.xpsnr_v};
        for (int c = 0; c < 3; ++c) {
            *dst[c] = MetricAggregate::from(std::move(*s_xp[c]));
            (*dst[c])->sequence = xp_->sequence_score(c);
        }
    }
    if (s_si) { // the sequence values are the maxima (P.910); a stream of one picture has no TI: its sequence TI is 0
        res.si = MetricAggregate::from(std::move(*s_si));
        res.si->sequence = res.si->stats.max;
        res.ti.emplace(); // scores: one per frame like every other metric; stats: of the frames that have a TI (none: all zero)
        res.ti->stats = ti_valid.empty() ? Stats{} : Stats::compute(ti_valid);
        res.ti->scores = std::move(*s_ti);
        res.ti->sequence = res.ti->stats.max;
    }
    if (s_mo) {
        res.motion = MetricAggregate::from(std::move(*s_mo));
        res.motion2 = MetricAggregate::from(std::move(*s_mo2));
    }
    if (vf_) {
        for (int k = 0; k < 4; ++k) res.vif_scale[k] = MetricAggregate::from(std::move(*s_vf[k]));
        res.vif = MetricAggregate::from(std::move(*s_vf[4]));
    }
    if (ad_) {
        for (int k = 0; k < 4; ++k) res.adm_scale[k] = MetricAggregate::from(std::move(*s_ad[k]));
        res.adm2 = MetricAggregate::from(std::move(*s_ad[4]));
    }
    if (s_sc) {
        res.scene_score = MetricAggregate::from(std::move(*s_sc));
        res.scene_starts = std::move(scene_starts);
    }
    if (cb_) {
        for (int k = 0; k < 5; ++k) res.cambi_scale[k] = MetricAggregate::from(std::move(*s_cb[k]));
        res.cambi = MetricAggregate::from(std::move(*s_cb[5]));
    }
    if (cbr_) {
        for (int k = 0; k < 5; ++k) res.cambi_ref_scale[k] = MetricAggregate::from(std::move(*s_cbr[k]));
        res.cambi_ref = MetricAggregate::from(std::move(*s_cbr[5]));
    }
    if (fl_) {
        res.flip = MetricAggregate::from(std::move(*s_fl[0]));
        res.flip_min = MetricAggregate::from(std::move(*s_fl[1]));
        res.flip_max = MetricAggregate::from(std::move(*s_fl[2]));
    }
    for (int k = 0; k < 8; ++k)
        if (s_yv[k]) {
            res.yuv[k] = MetricAggregate::from(std::move(*s_yv[k]));
            res.yuv[k]->sequence = yv_->sequence_score(k);
        }
    for (int k = 0; k < 2; ++k)
        if (s_hv[k]) {
            res.hvs[k] = MetricAggregate::from(std::move(*s_hv[k]));
            res.hvs[k]->sequence = hv_->sequence_score(k);
        }
    for (int k = 0; k < 2; ++k)
        if (s_ci[k]) {
            res.ciede[k] = MetricAggregate::from(std::move(*s_ci[k]));
            res.ciede[k]->sequence = ci_->sequence_score(k);
        }
    for (int k = 0; k < 2; ++k)
        if (s_gm[k]) {
            res.gmsd[k] = MetricAggregate::from(std::move(*s_gm[k]));
            res.gmsd[k]->sequence = gm_->sequence_score(k);
        }
    if (s_hp) {
        res.haarpsi = MetricAggregate::from(std::move(*s_hp));
        res.haarpsi->sequence = hp_->sequence_score();
    }
    if (it_)
        for (int k = 0; k < 2; ++k) {
            res.deitp[k] = MetricAggregate::from(std::move(*s_it[k]));
            res.deitp[k]->sequence = it_->sequence_score(k);
        }
    if (md_) {
        res.mdsi = MetricAggregate::from(std::move(*s_md));
        res.mdsi->sequence = md_->sequence_score();
    }
    if (s_psnr) res.psnr = MetricAggregate::from(std::move(*s_psnr));
    if (s_ssim) res.ssim = MetricAggregate::from(std::move(*s_ssim));
    if (s_msssim) res.msssim = MetricAggregate::from(std::move(*s_msssim));
    if (s_ssimu) res.ssimulacra2 = MetricAggregate::from(std::move(*s_ssimu));
    return res;
}

} // namespace tm_host
