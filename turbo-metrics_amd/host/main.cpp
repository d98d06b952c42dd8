// main.cpp -- `turbo-metrics`: the command line of the reference (crates/turbo-metrics-cli/src/main.rs:31-356) over the
// MI355X engine.  Same positional arguments, same flags (-m/--metrics, --every, --skip, --skip-ref, --skip-dis, --frames,
// --output), same stdout formats (output.cpp), status on stderr, ExitCode::FAILURE on the same conditions.
// Additions (no counterpart in the reference, all optional): --batch, --device, --devices, --ranks, --no-pipeline, --full-sums, and the
// description of headerless YUV input (--width, --height, --bits, --color-primaries, --matrix-coefficients,
// --transfer-characteristics, --full-range).
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include "frame_sources.hpp"
#include "output.hpp"
#include "ranks.hpp"
#include "turbo_metrics.hpp"

using namespace tm_host;

namespace {

enum Level { L_ERROR = 0, L_WARN, L_INFO, L_DEBUG, L_TRACE };
Level g_level = L_INFO;

void log_line(Level lv, const char *target, const std::string &msg)
{
    if (lv > g_level) return;
    static const char *names[] = {"ERROR", " WARN", " INFO", "DEBUG", "TRACE"};
    std::cerr << names[lv] << " " << target << ": " << msg << "\n"; // tracing fmt::layer().compact().without_time()
}

const char *kTarget = "turbo_metrics_cli";

void usage(std::ostream &os)
{
    os << "Turbo metrics compares two images or videos using quality metrics\n\n"
          "Usage: turbo-metrics [OPTIONS] <REFERENCE> <DISTORTED>\n\n"
          "Arguments:\n"
          "  <REFERENCE>  Reference media (PNG / PPM / PFM image, Y4M or raw planar YUV, IVF / Matroska video through TM_DECODER). Use `-` to read from stdin\n"
          "  <DISTORTED>  Distorted media. Use `-` to read from stdin\n\n"
          "Options:\n"
          "  -m, --metrics <METRICS>    Select the metrics to compute [possible values: psnr, ssim, msssim, ssimulacra2, xpsnr]\n"
          "                             [further values, each described below: vif, adm, cambi, flip, psnr-yuv, ssim-yuv]\n"
          "                             [and: psnr-hvs, psnr-hvs-m]\n"
          "                             [and: ciede2000]\n"
          "                             [and: gmsd]\n"
          "                             [and: haarpsi]\n"
          "                             [and: deitp]\n"
          "                             [and: mdsi]\n"
          "                             and vif: VMAF's VIF of the luma planes, four scales (YUV inputs; runs beside the others or alone)\n"
          "                             and adm: VMAF's ADM of the luma planes, adm2 and four scales (likewise)\n"
          "      --every <EVERY>        Only compute metrics every few frames [default: 0]\n"
          "      --skip <SKIP>          Index of the first frame to start computing at [default: 0]\n"
          "      --skip-ref <SKIP_REF>  Index of the first reference frame, additive with `skip` [default: 0]\n"
          "      --skip-dis <SKIP_DIS>  Index of the first distorted frame, additive with `skip` [default: 0]\n"
          "      --frames <FRAMES>      Amount of frames to compute [default: 0]\n"
          "      --output <OUTPUT>      stdout format [possible values: default, json, json-lines, csv]\n"
          "      --batch <N>            frame pairs per GPU launch [default: by picture size, 16 at 1080p, 8 at 4K]\n"
          "      --device <N>           GPU ordinal [default: 0]\n"
          "      --devices <N>          shard the frame pairs of two regular files over N GPUs (0 = all visible) [default: 1]\n"
          "      --ranks <N>            the same shards as N processes, one per GPU, scores gathered by ONE RCCL reduce to rank 0\n"
          "                             (TM_RANK_TRANSPORT=pipe: over pipes instead; TM_RANK_TIMEOUT_S: give up after that many seconds)\n"
          "      --no-pipeline          do not overlap reading/upload of the next batch with the current one\n"
          "      --loop <MODE>          batched (default: compute_all), reference (the reference's loop: one blocking compute_one per pair),\n"
          "                             deferred (that loop with compute_one_deferred + collect: --in-flight pairs in flight)\n"
          "      --in-flight <N>        pairs in flight with --loop deferred, 2 ... 8: pair k is collected after pair k + N - 1 went in [default: 2]\n"
          "      --full-sums            compute all 108 SSIMULACRA2 sums, also the zero-weighted ones\n"
          "      --width <W> --height <H> [--bits 8|10|12|16]   headerless planar 4:2:0 input\n"
          "      --color-primaries <N> --matrix-coefficients <N> --transfer-characteristics <N>   H.273 codes (1, 5, 6; 2 = by height)\n"
          "      --full-range           the YUV input is full range (unsupported by the reference and here)\n"
          "      --motion               also compute VMAF's integer motion / motion2 of the REFERENCE stream (YUV inputs; runs beside -m or alone)\n"
          "      --siti                 also compute ITU-T P.910 spatial / temporal information (si, ti) of the REFERENCE stream; the sequence values are\n"
          "                             the maxima (YUV inputs; runs beside -m or alone)\n"
          "      --siti-gain <X>        scale si and ti by X (with --siti) [default: 1]\n"
          "      --siti-range <RANGE>   full: code values as they are; limited: gain 255/219, the limited-to-full-range stretch (with --siti)\n"
          "                             [default: full] [possible values: full, limited]\n"
          "      --scenes               also find the scene cuts of the REFERENCE stream from luma histograms: per-frame scene_score and scene_cut,\n"
          "                             and scene_starts, the frames at which a scene begins (YUV inputs; runs beside -m or alone)\n"
          "      --scene-threshold <X>  a frame whose scene_score reaches X starts a scene, 0 < X <= 1 (with --scenes) [default: 0.5]\n"
          "      --scene-bins <N>       histogram bins the score compares, after merging neighbours: 8, 16, 32, 64, 128 or 256 (with --scenes) [default: 64]\n"
          "  -m cambi                   CAMBI, VMAF's banding index, of the DISTORTED stream: per-frame cambi and cambi_scale0 .. cambi_scale4, and their\n"
          "                             sequence means (YUV inputs of at least 32 x 32; runs beside the other -m values or alone)\n"
          "  -m flip                    LDR-FLIP, the perceptual difference map of pairs of 8-bit RGB images (PNG, PPM): per-pair flip (the map's mean),\n"
          "                             flip_min and flip_max, after all other columns; alone or beside the other -m values\n"
          "      --flip-ppd <X>         pixels per degree of the viewing condition, 8 ... 256; above 74.04 the run ends with an error (with -m flip) [default: 67.02]\n"
          "      --flip-map <PREFIX>    write every pair's FLIP map as a one-channel PFM, PREFIX000000.pfm, PREFIX000001.pfm, ... (with -m flip)\n"
          "  -m psnr-yuv                PSNR per plane on the coded samples of 4:2:0 YUV pairs, as ffmpeg's psnr filter and libvmaf print it: psnr_y, psnr_u,\n"
          "                             psnr_v, psnr_avg, after all other columns; the sequence values come from the summed squared error\n"
          "  -m ssim-yuv                the SSIM of x264 and ffmpeg's ssim filter per plane of 4:2:0 YUV pairs: ssim_y, ssim_u, ssim_v, ssim_all, after all\n"
          "                             other columns; the sequence values are the means over the frames; both run alone or beside the other -m values\n"
          "  -m psnr-hvs                PSNR-HVS of the luma planes of YUV pairs: the 8x8 DCT coefficients of the difference weighted by a contrast\n"
          "                             sensitivity table, non-overlapping blocks (not libvmaf's variant): psnr_hvs, after all other columns\n"
          "  -m psnr-hvs-m              PSNR-HVS-M: the same after contrast masking by the two pictures' blocks: psnr_hvs_m, after all other columns; the\n"
          "                             sequence values come from the summed weighted error; both run alone or beside the other -m values\n"
          "  -m ciede2000               CIEDE2000 of 4:2:0 YUV pairs: the colour difference dE00 (Sharma, Wu, Dalal 2005) of every luma position, chroma taken\n"
          "                             without interpolation, Lab from limited-range Y'CbCr through the sRGB curve with the matrix of --matrix-coefficients:\n"
          "                             ciede2000 = min(45 - 20 log10(mean dE00), 100) and ciede2000_de, the mean dE00, after all other columns; the sequence\n"
          "                             values come from the summed dE00; alone or beside the other -m values\n"
          "      --ciede-libvmaf        the matrix and the factors kL, kC, kH = 0.65, 1, 4 libvmaf's ciede feature is recalled to use (with -m ciede2000)\n"
          "      --ciede-map <PREFIX>   write every pair's dE00 map as a one-channel PFM, PREFIX000000.pfm, PREFIX000001.pfm, ... (with -m ciede2000)\n"
          "  -m gmsd                    GMSD, the gradient magnitude similarity deviation (Xue et al. 2014) of the luma planes of YUV pairs: the standard\n"
          "                             deviation of the similarity of the Prewitt gradient magnitudes after a 2x2 mean and 2:1 decimation (0: identical),\n"
          "                             and gmsm, its mean: gmsd, gmsm, after all other columns; the sequence values are pooled over all positions of all\n"
          "                             pairs; alone or beside the other -m values\n"
          "      --gmsd-population      divide by N instead of N - 1 in the standard deviation (with -m gmsd)\n"
          "      --gmsd-map <PREFIX>    write every pair's GMS map as a one-channel PFM, PREFIX000000.pfm, PREFIX000001.pfm, ... (with -m gmsd)\n"
          "  -m haarpsi                 HaarPSI, the Haar wavelet-based perceptual similarity index (Reisenhofer et al. 2018; grayscale form) of the luma\n"
          "                             planes of YUV pairs: Haar coefficient similarity at two scales after a 2x2 mean and 2:1 decimation, weighted by the\n"
          "                             third scale (1: identical; NaN where both pictures are flat): haarpsi, after all other columns; the sequence value\n"
          "                             comes from the summed weighted sums of all pairs; alone or beside the other -m values\n"
          "      --haarpsi-map <PREFIX> write every pair's local similarity map as a one-channel PFM, PREFIX000000.pfm, PREFIX000001.pfm, ... (with -m haarpsi)\n"
          "  -m deitp                   dE ITP (ITU-R BT.2124), the HDR colour difference, of 4:2:0 YUV pairs: 720 times the distance in ICtCp (BT.2100) of\n"
          "                             every luma position, chroma taken without interpolation; 1 is about one just-noticeable difference.  The matrix is\n"
          "                             always BT.2020 non-constant luminance: --matrix-coefficients is not consulted.  Limited range.  Prints deitp, the\n"
          "                             pair's mean, and deitp_max after all other columns; the sequence mean comes from the summed dE ITP of all pairs;\n"
          "                             alone or beside the other -m values\n"
          "      --itp-transfer <pq|hlg>  the transfer function of the samples: BT.2100 PQ, or HLG on a 1000 cd/m2 display (with -m deitp) [default: pq]\n"
          "      --itp-map <PREFIX>     write every pair's dE ITP map as a one-channel PFM, PREFIX000000.pfm, PREFIX000001.pfm, ... (with -m deitp)\n"
          "  -m mdsi                    MDSI, the mean deviation similarity index, of 4:2:0 YUV pairs: gradient similarity of the luma-like plane and\n"
          "                             chromaticity similarity at every f-th position of the f x f box mean, pooled by the mean absolute deviation of the\n"
          "                             fourth roots (0: identical; larger is worse).  Limited range; the matrix follows --matrix-coefficients as for\n"
          "                             ciede2000.  Prints mdsi after all other columns.  MDSI does not pool across pictures: the sequence value is the\n"
          "                             mean of the per-pair values; alone or beside the other -m values\n"
          "      --mdsi-factor <N>      the decimation factor f, 1 ... 128 (with -m mdsi) [default: max(1, round(min(width, height) / 256))]\n"
          "      --mdsi-map <PREFIX>    write every pair's GCS map (ceil(height / f) rows of ceil(width / f)) as a one-channel PFM, PREFIX000000.pfm, ...\n"
          "                             (with -m mdsi)\n"
          "      --psnr-yuv-cap         cap every PSNR at libvmaf's 6 * depth + 12 dB instead of printing inf (with -m psnr-yuv)\n"
          "      --ssim-yuv-map <PREFIX>  write every pair's luma SSIM window map as a one-channel PFM, PREFIX000000.pfm, ... (with -m ssim-yuv)\n"
          "      --cambi-window <N>     side of the window the banding is looked for in, 3 ... 127 (with -m cambi) [default: 63 * width / 3840, at least 3]\n"
          "      --cambi-topk <X>       share of the largest c-values a scale's score averages, 0 < X <= 1 (with -m cambi) [default: 0.6]\n"
          "      --cambi-ref            also print cambi_ref and cambi_ref_scale0 .. cambi_ref_scale4 of the REFERENCE stream (with -m cambi)\n"
          "      --xpsnr-fps <N[/D]>    frame rate that picks XPSNR's temporal order (below 32: first order) [default: the Y4M F token, else 25]\n"
          "  -h, --help                 Print help\n"
          "  -V, --version              Print version\n";
}

bool parse_u32(const std::string &s, uint32_t &out)
{
    if (s.empty()) return false;
    char *end = nullptr;
    const unsigned long v = strtoul(s.c_str(), &end, 10);
    if (*end || v > 0xFFFFFFFFul || s[0] == '-') return false;
    out = (uint32_t)v;
    return true;
}

std::string format_duration(std::chrono::milliseconds d) // main.rs:357-385
{
    long long secs = d.count() / 1000;
    const long long millis = d.count() % 1000, minutes = secs / 60;
    secs %= 60;
    std::string s;
    if (minutes > 0) { s += std::to_string(minutes) + " m"; if (secs > 0) s += " "; }
    if (secs > 0) { s += std::to_string(secs) + " s"; if (millis > 0) s += " "; }
    if (millis > 0) s += std::to_string(millis) + " ms";
    return s;
}

void log_source(const char *target, const FrameSource &src)
{
    const auto cc = src.color_characteristics();
    log_line(L_INFO, target, "codec=" + src.format_id().str() + " width=" + std::to_string(src.width()) + " height=" + std::to_string(src.height()) +
                                 " cp=" + to_string(cc.first.cp) + " mc=" + to_string(cc.first.mc) + " tc=" + to_string(cc.first.tc) +
                                 " cr=" + to_string(cc.second) + " frame_count=" + std::to_string(src.frame_count()));
}

} // namespace

// --batch not given: at most 72 Mpx per launch, 2 .. 16 pairs (16 at 1080p and below, 8 at 4K; round 6: with 10-bit pictures packed on the
// link the 4K loop is no longer bound by PCIe alone -- 4 pairs per launch 1 246 pairs/s, 16: 1 333, profiles/r06b_bench.json).  Host-fed streams are
// bound by the file reads and PCIe long before the engine (1080p: ~7.5 k pairs/s over PCIe against 12.7 k pairs/s of the engine at 16
// pairs per launch; 4K: 1.1 k against 3.0 k at 4), and since round 4 the page-locked frame rings no longer grow with the batch
// (upload fences), so the batch only has to be large enough for the kernels and small enough for the engines' memory
// (two engines x batch x 0.24 GB at 1080p, x 0.95 GB at 4K).
static uint32_t auto_batch(uint32_t w, uint32_t h)
{
    const double mpx = (double)w * (double)h / 1e6;
    uint32_t b = 16;
    while (b > 2 && (double)b * mpx > 72.0) b /= 2;
    return b;
}

int main(int argc, char **argv)
{
    if (const char *env = getenv("RUST_LOG")) {
        const std::string v = env;
        if (v == "error") g_level = L_ERROR; else if (v == "warn") g_level = L_WARN; else if (v == "info") g_level = L_INFO;
        else if (v == "debug") g_level = L_DEBUG; else if (v == "trace") g_level = L_TRACE;
    }
    std::vector<std::string> pos;
    Metrics metrics;
    Options opts;
    Output output = Output::Default;
    SourceHints hints;
    uint32_t batch = 0 /* 0: chosen from the picture size */, device = 0, devices = 1, ranks = 0 /* 0: not asked for */, in_flight_pairs = 2;
    uint32_t xpsnr_fps_num = 0, xpsnr_fps_den = 1; // --xpsnr-fps (0: not given)
    bool pipeline = true, full_sums = false, in_flight_given = false, scene_values_given = false, cambi_values_given = false, flip_values_given = false, siti_gain_given = false, siti_range_given = false, siti_limited = false;
    bool psnr_yuv_values_given = false, ssim_yuv_values_given = false, ciede_values_given = false, gmsd_values_given = false, haarpsi_values_given = false, itp_values_given = false, mdsi_values_given = false;
    enum class Loop { Batched, Reference, Deferred } loop = Loop::Batched;
    std::vector<std::pair<int, long long>> tune;

    auto bad = [&](const std::string &m) {
        std::cerr << "error: " << m << "\n\nFor more information, try '--help'.\n";
        return 2; // clap's usage-error exit code
    };
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i], val;
        bool has_val = false;
        if (a.rfind("--", 0) == 0) {
            const size_t eq = a.find('=');
            if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); has_val = true; }
        }
        auto value = [&](std::string &dst) {
            if (has_val) { dst = val; return true; }
            if (i + 1 >= argc) return false;
            dst = argv[++i];
            return true;
        };
        auto u32 = [&](uint32_t &dst) {
            std::string s;
            return value(s) && parse_u32(s, dst);
        };
        if (a == "-h" || a == "--help") { usage(std::cout); return 0; }
        if (a == "-V" || a == "--version") { std::cout << "turbo-metrics " << tm_version() << "\n"; return 0; }
        if (a == "-m" || a == "--metrics") {
            std::string s;
            if (!value(s)) return bad("a value is required for '--metrics <METRICS>' but none was supplied");
            if (s == "psnr") metrics.psnr = true; else if (s == "ssim") metrics.ssim = true; else if (s == "msssim") metrics.msssim = true;
            else if (s == "ssimulacra2") metrics.ssimulacra2 = true;
            else if (s == "xpsnr") metrics.xpsnr = true;
            else if (s == "vif") metrics.vif = true;
            else if (s == "adm") metrics.adm = true;
            else if (s == "cambi") metrics.cambi = true;
            else if (s == "flip") metrics.flip = true;
            else if (s == "psnr-yuv") metrics.psnr_yuv = true;
            else if (s == "ssim-yuv") metrics.ssim_yuv = true;
            else if (s == "psnr-hvs") metrics.psnr_hvs = true;
            else if (s == "psnr-hvs-m") metrics.psnr_hvs_m = true;
            else if (s == "ciede2000") metrics.ciede = true;
            else if (s == "gmsd") metrics.gmsd = true;
            else if (s == "haarpsi") metrics.haarpsi = true;
            else if (s == "deitp") metrics.deitp = true;
            else if (s == "mdsi") metrics.mdsi = true;
            else return bad("invalid value '" + s + "' for '--metrics <METRICS>'\n  [possible values: psnr, ssim, msssim, ssimulacra2, xpsnr, vif, adm, cambi, flip, psnr-yuv, ssim-yuv, psnr-hvs, psnr-hvs-m] [and: ciede2000] [and: gmsd] [and: haarpsi] [and: deitp] [and: mdsi]");
        } else if (a.rfind("-m", 0) == 0 && a.size() > 2 && a[1] == 'm') { // -mpsnr
            const std::string s = a.substr(2);
            if (s == "psnr") metrics.psnr = true; else if (s == "ssim") metrics.ssim = true; else if (s == "msssim") metrics.msssim = true;
            else if (s == "ssimulacra2") metrics.ssimulacra2 = true;
            else if (s == "xpsnr") metrics.xpsnr = true;
            else if (s == "vif") metrics.vif = true;
            else if (s == "adm") metrics.adm = true;
            else if (s == "cambi") metrics.cambi = true;
            else if (s == "flip") metrics.flip = true;
            else if (s == "psnr-yuv") metrics.psnr_yuv = true;
            else if (s == "ssim-yuv") metrics.ssim_yuv = true;
            else if (s == "psnr-hvs") metrics.psnr_hvs = true;
            else if (s == "psnr-hvs-m") metrics.psnr_hvs_m = true;
            else if (s == "ciede2000") metrics.ciede = true;
            else if (s == "gmsd") metrics.gmsd = true;
            else if (s == "haarpsi") metrics.haarpsi = true;
            else if (s == "deitp") metrics.deitp = true;
            else if (s == "mdsi") metrics.mdsi = true;
            else return bad("invalid value '" + s + "' for '--metrics <METRICS>'\n  [possible values: psnr, ssim, msssim, ssimulacra2, xpsnr, vif, adm, cambi, flip, psnr-yuv, ssim-yuv, psnr-hvs, psnr-hvs-m] [and: ciede2000] [and: gmsd] [and: haarpsi] [and: deitp] [and: mdsi]");
        } else if (a == "--every") { if (!u32(opts.every)) return bad("invalid value for '--every <EVERY>'"); }
        else if (a == "--skip") { if (!u32(opts.skip)) return bad("invalid value for '--skip <SKIP>'"); }
        else if (a == "--skip-ref") { if (!u32(opts.skip_ref)) return bad("invalid value for '--skip-ref <SKIP_REF>'"); }
        else if (a == "--skip-dis") { if (!u32(opts.skip_dis)) return bad("invalid value for '--skip-dis <SKIP_DIS>'"); }
        else if (a == "--frames") { if (!u32(opts.frames)) return bad("invalid value for '--frames <FRAMES>'"); }
        else if (a == "--output") {
            std::string s;
            if (!value(s) || !parse_output(s, output)) return bad("invalid value '" + s + "' for '--output <OUTPUT>'\n  [possible values: default, json, json-lines, csv]");
        } else if (a == "--batch") { if (!u32(batch) || batch == 0) return bad("invalid value for '--batch <N>'"); }
        else if (a == "--device") { if (!u32(device)) return bad("invalid value for '--device <N>'"); }
        else if (a == "--devices") { if (!u32(devices)) return bad("invalid value for '--devices <N>'"); }
        else if (a == "--ranks") { if (!u32(ranks) || ranks == 0 || ranks > 64) return bad("invalid value for '--ranks <N>'"); }
        else if (a == "--no-pipeline") pipeline = false;
        else if (a == "--in-flight") { if (!u32(in_flight_pairs) || in_flight_pairs < 2 || in_flight_pairs > TurboMetrics::MAX_DEFERRED_DEPTH) return bad("invalid value for '--in-flight <N>'\n  [2 ... 8]"); in_flight_given = true; }
        else if (a == "--loop") {
            std::string s;
            if (!value(s)) return bad("a value is required for '--loop <MODE>'");
            if (s == "batched") loop = Loop::Batched; else if (s == "reference") loop = Loop::Reference; else if (s == "deferred") loop = Loop::Deferred;
            else return bad("invalid value '" + s + "' for '--loop <MODE>'\n  [possible values: batched, reference, deferred]");
        }
        else if (a == "--full-sums") full_sums = true;
        else if (a == "--motion") metrics.motion = true;
        else if (a == "--scenes") metrics.scenes = true;
        else if (a == "--siti") metrics.siti = true;
        else if (a == "--siti-gain") {
            std::string v;
            if (!value(v)) return bad("a value is required for '--siti-gain <X>' but none was supplied");
            char *end = nullptr;
            const double x = strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x > 0.0) || !(x <= 1e6)) return bad("invalid value '" + v + "' for '--siti-gain <X>'\n  [0 < X <= 1e6]");
            metrics.siti_gain = x;
            siti_gain_given = true;
        }
        else if (a == "--siti-range") {
            std::string v;
            if (!value(v)) return bad("a value is required for '--siti-range <RANGE>' but none was supplied");
            if (v == "limited") siti_limited = true;
            else if (v == "full") siti_limited = false;
            else return bad("invalid value '" + v + "' for '--siti-range <RANGE>'\n  [possible values: full, limited]");
            siti_range_given = true;
        }
        else if (a == "--scene-threshold") {
            std::string v;
            if (!value(v)) return bad("a value is required for '--scene-threshold <X>' but none was supplied");
            char *end = nullptr;
            const double x = strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x > 0.0 && x <= 1.0)) return bad("invalid value '" + v + "' for '--scene-threshold <X>'\n  [0 < X <= 1]");
            metrics.scene_threshold = x;
            scene_values_given = true;
        }
        else if (a == "--scene-bins") {
            std::string v;
            if (!value(v)) return bad("a value is required for '--scene-bins <N>' but none was supplied");
            uint32_t n = 0;
            if (!parse_u32(v, n) || (n != 8 && n != 16 && n != 32 && n != 64 && n != 128 && n != 256))
                return bad("invalid value '" + v + "' for '--scene-bins <N>'\n  [possible values: 8, 16, 32, 64, 128, 256]");
            metrics.scene_bins = n;
            scene_values_given = true;
        }
        else if (a == "--cambi-window") {
            std::string v;
            if (!value(v)) return bad("a value is required for '--cambi-window <N>' but none was supplied");
            uint32_t n = 0;
            if (!parse_u32(v, n) || n < 3 || n > 127) return bad("invalid value '" + v + "' for '--cambi-window <N>'\n  [3 ... 127]");
            metrics.cambi_window = n;
            cambi_values_given = true;
        }
        else if (a == "--cambi-topk") {
            std::string v;
            if (!value(v)) return bad("a value is required for '--cambi-topk <X>' but none was supplied");
            char *end = nullptr;
            const double x = strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x > 0.0 && x <= 1.0)) return bad("invalid value '" + v + "' for '--cambi-topk <X>'\n  [0 < X <= 1]");
            metrics.cambi_topk = x;
            cambi_values_given = true;
        }
        else if (a == "--flip-ppd") {
            std::string v;
            if (!value(v)) return bad("a value is required for '--flip-ppd <X>' but none was supplied");
            char *end = nullptr;
            const double x = strtod(v.c_str(), &end);
            if (v.empty() || *end || !(x >= 8.0 && x <= 256.0)) return bad("invalid value '" + v + "' for '--flip-ppd <X>'\n  [8 ... 256]");
            metrics.flip_ppd = x;
            flip_values_given = true;
        }
        else if (a == "--psnr-yuv-cap") { metrics.psnr_yuv_cap = true; psnr_yuv_values_given = true; }
        else if (a == "--ssim-yuv-map") {
            if (!value(metrics.ssim_yuv_map) || metrics.ssim_yuv_map.empty()) return bad("a value is required for '--ssim-yuv-map <PREFIX>' but none was supplied");
            ssim_yuv_values_given = true;
        }
        else if (a == "--flip-map") {
            if (!value(metrics.flip_map) || metrics.flip_map.empty()) return bad("a value is required for '--flip-map <PREFIX>' but none was supplied");
            flip_values_given = true;
        }
        else if (a == "--ciede-libvmaf") { metrics.ciede_libvmaf = true; ciede_values_given = true; }
        else if (a == "--ciede-map") {
            if (!value(metrics.ciede_map) || metrics.ciede_map.empty()) return bad("a value is required for '--ciede-map <PREFIX>' but none was supplied");
            ciede_values_given = true;
        }
        else if (a == "--gmsd-population") { metrics.gmsd_population = true; gmsd_values_given = true; }
        else if (a == "--gmsd-map") {
            if (!value(metrics.gmsd_map) || metrics.gmsd_map.empty()) return bad("a value is required for '--gmsd-map <PREFIX>' but none was supplied");
            gmsd_values_given = true;
        }
        else if (a == "--haarpsi-map") {
            if (!value(metrics.haarpsi_map) || metrics.haarpsi_map.empty()) return bad("a value is required for '--haarpsi-map <PREFIX>' but none was supplied");
            haarpsi_values_given = true;
        }
        else if (a == "--itp-transfer") {
            std::string v;
            if (!value(v) || (v != "pq" && v != "hlg")) return bad("invalid value for '--itp-transfer <pq|hlg>'");
            metrics.itp_hlg = v == "hlg";
            itp_values_given = true;
        }
        else if (a == "--mdsi-factor") {
            if (!u32(metrics.mdsi_factor) || metrics.mdsi_factor < 1 || metrics.mdsi_factor > 128) return bad("invalid value for '--mdsi-factor <N>' (1 ... 128)");
            mdsi_values_given = true;
        }
        else if (a == "--mdsi-map") {
            if (!value(metrics.mdsi_map) || metrics.mdsi_map.empty()) return bad("a value is required for '--mdsi-map <PREFIX>' but none was supplied");
            mdsi_values_given = true;
        }
        else if (a == "--itp-map") {
            if (!value(metrics.itp_map) || metrics.itp_map.empty()) return bad("a value is required for '--itp-map <PREFIX>' but none was supplied");
            itp_values_given = true;
        }
        else if (a == "--cambi-ref") { metrics.cambi_ref = true; cambi_values_given = true; }
        else if (a == "--xpsnr-fps") {
            std::string v;
            if (!value(v)) return bad("a value is required for '--xpsnr-fps <N[/D]>'");
            const size_t sl = v.find('/');
            if (!parse_u32(v.substr(0, sl), xpsnr_fps_num) || (sl != std::string::npos && !parse_u32(v.substr(sl + 1), xpsnr_fps_den)) ||
                xpsnr_fps_num == 0 || xpsnr_fps_den == 0)
                return bad("invalid value '" + v + "' for '--xpsnr-fps <N[/D]>'");
        }
        else if (a == "--tune") { // --tune <param>=<value>: tm_engine_debug_set_param (measurements; not in the usage text)
            std::string kv; if (!value(kv) || kv.find('=') == std::string::npos) return bad("invalid value for '--tune <param>=<value>'");
            tune.emplace_back(atoi(kv.c_str()), atoll(kv.c_str() + kv.find('=') + 1));
        }
        else if (a == "--width") { if (!u32(hints.width)) return bad("invalid value for '--width <W>'"); }
        else if (a == "--height") { if (!u32(hints.height)) return bad("invalid value for '--height <H>'"); }
        else if (a == "--bits") { uint32_t b; if (!u32(b) || (b != 8 && b != 10 && b != 12 && b != 16)) return bad("invalid value for '--bits'"); hints.bits = (int)b; }
        else if (a == "--color-primaries") { uint32_t v; if (!u32(v)) return bad("invalid value for '--color-primaries'"); hints.cp = (int)v; }
        else if (a == "--matrix-coefficients") { uint32_t v; if (!u32(v)) return bad("invalid value for '--matrix-coefficients'"); hints.mc = (int)v; }
        else if (a == "--transfer-characteristics") { uint32_t v; if (!u32(v)) return bad("invalid value for '--transfer-characteristics'"); hints.tc = (int)v; }
        else if (a == "--full-range") hints.full_range = true;
        else if (a == "--raw") hints.force_raw = true;
        else if (a.size() > 1 && a[0] == '-' && a != "-") return bad("unexpected argument '" + a + "' found");
        else pos.push_back(a);
    }
    if (pos.size() != 2) return bad("the following required arguments were not provided:\n  <REFERENCE>\n  <DISTORTED>");
    if (scene_values_given && !metrics.scenes) return bad("'--scene-threshold <X>' and '--scene-bins <N>' belong to '--scenes'");
    if ((siti_gain_given || siti_range_given) && !metrics.siti) return bad("'--siti-gain <X>' and '--siti-range <RANGE>' belong to '--siti'");
    if (siti_gain_given && siti_range_given) return bad("'--siti-gain <X>' and '--siti-range <RANGE>' cannot be used together");
    if (siti_limited) metrics.siti_gain = 255.0 / 219.0;
    if (cambi_values_given && !metrics.cambi) return bad("'--cambi-window <N>', '--cambi-topk <X>' and '--cambi-ref' belong to '-m cambi'");
    if (flip_values_given && !metrics.flip) return bad("'--flip-ppd <X>' and '--flip-map <PREFIX>' belong to '-m flip'");
    if (psnr_yuv_values_given && !metrics.psnr_yuv) return bad("'--psnr-yuv-cap' belongs to '-m psnr-yuv'");
    if (ssim_yuv_values_given && !metrics.ssim_yuv) return bad("'--ssim-yuv-map <PREFIX>' belongs to '-m ssim-yuv'");
    if (metrics.psnr_yuv || metrics.ssim_yuv) { // like FLIP: one device, the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m psnr-yuv / ssim-yuv do not run with ") + why); return EXIT_FAILURE; }
    }
    if (ciede_values_given && !metrics.ciede) return bad("'--ciede-libvmaf' and '--ciede-map <PREFIX>' belong to '-m ciede2000'");
    if (metrics.ciede) { // like -m psnr-yuv: one device, the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m ciede2000 does not run with ") + why); return EXIT_FAILURE; }
    }
    if (gmsd_values_given && !metrics.gmsd) return bad("'--gmsd-population' and '--gmsd-map <PREFIX>' belong to '-m gmsd'");
    if (metrics.gmsd) { // like -m psnr-hvs: one device, the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m gmsd does not run with ") + why); return EXIT_FAILURE; }
    }
    if (haarpsi_values_given && !metrics.haarpsi) return bad("'--haarpsi-map <PREFIX>' belongs to '-m haarpsi'");
    if (metrics.haarpsi) { // like -m gmsd: one device, the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m haarpsi does not run with ") + why); return EXIT_FAILURE; }
    }
    if (itp_values_given && !metrics.deitp) return bad("'--itp-transfer <pq|hlg>' and '--itp-map <PREFIX>' belong to '-m deitp'");
    if (mdsi_values_given && !metrics.mdsi) return bad("'--mdsi-factor <N>' and '--mdsi-map <PREFIX>' belong to '-m mdsi'");
    if (metrics.mdsi) { // like -m ciede2000: one device, the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m mdsi does not run with ") + why); return EXIT_FAILURE; }
    }
    if (metrics.deitp) { // like -m ciede2000: one device, the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m deitp does not run with ") + why); return EXIT_FAILURE; }
    }
    if (metrics.psnr_hvs || metrics.psnr_hvs_m) { // like VIF: one device, the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m psnr-hvs / psnr-hvs-m do not run with ") + why); return EXIT_FAILURE; }
    }
    if (metrics.flip) { // FLIP, like CAMBI, runs on one device in the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m flip does not run with ") + why); return EXIT_FAILURE; }
    }
    if (metrics.cambi) { // CAMBI, like VIF and ADM, runs on one device in the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m cambi does not run with ") + why); return EXIT_FAILURE; }
    }
    if (metrics.scenes) { // a frame is compared with the frame before it in ONE stream on one device
        const char *why = devices != 1 ? "--devices (shards would cut the sequence)"
                        : ranks > 0 ? "--ranks (shards would cut the sequence)"
                        : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("--scenes does not run with ") + why); return EXIT_FAILURE; }
    }

    if (metrics.xpsnr) { // XPSNR is stateful across the frames of ONE sequence on one device
        const char *why = opts.every > 1 ? "--every > 1 (skipped pictures never reach its temporal history)"
                        : devices != 1 ? "--devices (shards would cut its temporal history)"
                        : ranks > 0 ? "--ranks (shards would cut its temporal history)"
                        : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m xpsnr does not run with ") + why); return EXIT_FAILURE; }
    }

    if (metrics.vif) { // VIF runs on one device in the batched loop; sharding it is a later change
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m vif does not run with ") + why); return EXIT_FAILURE; }
    }

    if (metrics.adm) { // ADM, like VIF, runs on one device in the batched loop
        const char *why = devices != 1 ? "--devices" : ranks > 0 ? "--ranks" : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("-m adm does not run with ") + why); return EXIT_FAILURE; }
    }

    if (metrics.siti) { // TI compares consecutive pictures of ONE sequence on one device
        const char *why = opts.every > 1 ? "--every > 1 (skipped pictures would never reach its history)"
                        : devices != 1 ? "--devices (shards would cut its history)"
                        : ranks > 0 ? "--ranks (shards would cut its history)"
                        : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("--siti does not run with ") + why); return EXIT_FAILURE; }
    }

    if (metrics.motion) { // motion compares consecutive pictures of ONE sequence on one device
        const char *why = opts.every > 1 ? "--every > 1 (skipped pictures would never reach its history)"
                        : devices != 1 ? "--devices (shards would cut its history)"
                        : ranks > 0 ? "--ranks (shards would cut its history)"
                        : loop != Loop::Batched ? "--loop reference / deferred" : nullptr;
        if (why) { log_line(L_ERROR, kTarget, std::string("--motion does not run with ") + why); return EXIT_FAILURE; }
    }

    const bool ref_is_stdin = pos[0] == "-", dis_is_stdin = pos[1] == "-";
    if (ref_is_stdin && dis_is_stdin) {
        log_line(L_ERROR, kTarget, "Can't read both reference and distorted from stdin");
        return EXIT_FAILURE;
    }

    // ---- --ranks N: one process per GPU and ONE RCCL reduce of the per-frame scores (ranks.hpp).  This process is either the launcher
    // (it makes no GPU call: it starts the N ranks and waits for them) or, with TM_RANK in the environment, one of the ranks.
    RankEnv renv;
    bool is_rank = false;
    try { is_rank = rank_env(renv); }
    catch (const std::exception &e) { log_line(L_ERROR, kTarget, std::string("Could not join the ranks : ") + e.what()); return EXIT_FAILURE; }
    if (ranks > 0 && !is_rank) {
        if (ref_is_stdin || dis_is_stdin) { log_line(L_ERROR, kTarget, "--ranks needs two regular planar-YUV files of known length, not stdin"); return EXIT_FAILURE; }
        if (loop != Loop::Batched) { log_line(L_ERROR, kTarget, "--loop reference / deferred run on one device: not with --ranks"); return EXIT_FAILURE; }
        if (devices != 1) { log_line(L_ERROR, kTarget, "--ranks (one process per GPU) and --devices (one process, N GPUs) exclude each other"); return EXIT_FAILURE; }
        if (metrics.mask() == 0) { log_line(L_ERROR, kTarget, "Could not initialize engine : no metric selected (-m psnr|ssim|msssim|ssimulacra2)"); return EXIT_FAILURE; }
        const char *to = getenv("TM_RANK_TIMEOUT_S");
        std::cout.flush();
        return launch_ranks(argv, (int)ranks, to ? atof(to) : 0.0);
    }
    if (is_rank && (ranks == 0 || (int)ranks != renv.world)) { log_line(L_ERROR, kTarget, "TM_RANK is set but --ranks does not match TM_WORLD"); return EXIT_FAILURE; }
    if (is_rank && renv.rank != 0 && g_level > L_WARN && !getenv("RUST_LOG")) g_level = L_WARN; // rank 0 tells the story once

    // The reference initialises the device first because its frame sources decode on it (main.rs:138-139).  Here the sources
    // come first: a compressed-video source starts its decoder as a child process, and that must happen before this process
    // has touched the GPU runtime (a source only page-locks memory when its first frame is asked for, after init_hip).
    std::unique_ptr<FrameSource> source_ref, source_dis;
    try {
        source_ref = create_source(pos[0], hints);
    } catch (const std::exception &e) {
        log_line(L_ERROR, kTarget, std::string("Could not read reference : ") + e.what());
        return EXIT_FAILURE;
    }
    try {
        source_dis = create_source(pos[1], hints);
    } catch (const std::exception &e) {
        log_line(L_ERROR, kTarget, std::string("Could not read distorted : ") + e.what());
        return EXIT_FAILURE;
    }
    if (source_ref->width() != source_dis->width() || source_ref->height() != source_dis->height()) {
        // the reference logs this and carries on into undefined territory (main.rs:156-158); here it is fatal
        log_line(L_ERROR, kTarget, "Reference and distorted are not the same size");
        return EXIT_FAILURE;
    }
    if (is_rank) { // rank r works on device (device + r); TM_SHARE_DEVICE=1 (tests on a 1-GPU box) lets the ranks share what is visible
        const int visible = std::max(1, tm_device_count());
        const bool share = getenv("TM_SHARE_DEVICE") && atoi(getenv("TM_SHARE_DEVICE")) != 0;
        if (!share && renv.world > visible) {
            if (renv.rank == 0) log_line(L_ERROR, kTarget, "--ranks " + std::to_string(renv.world) + " but only " + std::to_string(visible) + " GPU(s) visible");
            return EXIT_FAILURE;
        }
        device = (device + (uint32_t)renv.rank) % (uint32_t)visible;
    }
    try {
        init_hip((int)device);
        if (g_level >= L_TRACE) // the engine library's own diagnostics (placement search, hardware queues): a function of the laboratory build
            if (auto fn = (void (*)(int))dlsym(RTLD_DEFAULT, "tm_set_debug_log")) fn(1);
    } catch (const std::exception &e) {
        log_line(L_ERROR, kTarget, std::string("Could not initialize the GPU : ") + e.what());
        return EXIT_FAILURE;
    }

    // One block of decode indices [lo, hi) on the device this thread is bound to: its own sources (opened on the same files), its own
    // engines, the reference's selection loop (lib.rs:385-404) with decode_start = lo.  Shared by --devices (a thread per device) and
    // --ranks (a process per device).
    struct Block { std::vector<FrameScores> scores; uint32_t decoded = 0; };
    // ready (optional): called once the block's engines exist and its sources have page-locked their rings -- where the one-device run starts its
    // clock (main.rs:252: after the decoders and the engine exist)
    // each: sees every FrameScores of the block as it arrives (rank 0 prints its own block while the others compute)
    // computed (optional): called when the block's last score is there, before its engines and rings are given back
    const auto score_block = [&](uint32_t w, uint32_t h, uint32_t lo, uint32_t hi, Block &out, const std::function<void()> &ready = nullptr,
                                 const std::function<void(const FrameScores &)> &each = nullptr, const std::function<void()> &computed = nullptr) {
        if (lo >= hi) { if (ready) ready(); if (computed) computed(); return; }
        auto sr = create_source(pos[0], hints), sd = create_source(pos[1], hints);
        const uint32_t b = std::min(batch, hi - lo);
        TurboMetrics tmx(w, h, metrics, b, pipeline && hi - lo > b);
        if (full_sums) tmx.set_full_sums(true);
        for (auto &t : tune) if (t.first < 100) tmx.debug_set_param(t.first, t.second);
        Options o = opts;
        o.decode_start = lo;
        o.frames = hi; // absolute decode index at which this block stops (lib.rs:396-398)
        if (ready) { TurboMetrics::prepare_sources(*sr, *sd, o); ready(); }
        uint32_t dc = lo;
        try { tmx.compute_all(*sr, *sd, o, [&](const FrameScores &fs) { out.scores.push_back(fs); if (each) each(fs); }, &dc); }
        catch (const NoFramesSelected &) { dc = hi; } // a block in which `every` selects no frame is empty, not an error (any other exception is one)
        out.decoded = dc - lo;
        if (computed) computed();
        if (g_level >= L_DEBUG) {
            const TurboMetrics::LoopTiming &t = tmx.loop_timing();
            char b[256];
            snprintf(b, sizeof b, "block [%u, %u): %.0f ms waiting for an upload slot, %.0f ms for the sources, %.0f ms handing frames to the engine, %.0f ms submitting, %.0f ms waiting for results + output",
                     lo, hi, t.wait_upload * 1e3, t.wait_frames * 1e3, t.set_frames * 1e3, t.submit * 1e3, t.drain * 1e3);
            log_line(L_DEBUG, kTarget, b);
        }
    };
    // what the one-device run prints behind the last per-frame line
    const auto report = [&](const std::vector<FrameScores> &all, uint32_t decoded, uint32_t w, uint32_t h, std::chrono::steady_clock::time_point start, const std::string &where) -> int {
        MetricsResults results;
        try { results = aggregate_scores(all, metrics); }
        catch (const std::exception &e) { std::cout.flush(); log_line(L_ERROR, kTarget, std::string("Computation failed : ") + e.what()); return EXIT_FAILURE; }
        const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - start);
        const long long dms = ms.count() > 0 ? ms.count() : 1;
        const unsigned long long fps = (unsigned long long)results.frame_count * 1000ull / (unsigned long long)dms;
        char perf_s[64];
        snprintf(perf_s, sizeof perf_s, "%.3f", (double)w * (double)h * (double)results.frame_count / (double)dms / 1000.0);
        log_line(L_INFO, kTarget, "Processed: " + std::to_string(results.frame_count) + " (decoded: ~" + std::to_string(decoded + opts.skip) +
                                      ") frame pairs in " + format_duration(ms) + " (" + std::to_string(fps) + " fps) (Mpx/s: " + perf_s + ") on " + where);
        output_results(output, results, std::cout);
        std::cout.flush();
        return EXIT_SUCCESS;
    };

    if (is_rank) {
        const bool root = renv.rank == 0;
        const size_t known = std::min(source_ref->frame_count(), source_dis->frame_count());
        const uint32_t lead = opts.skip + std::max(opts.skip_ref, opts.skip_dis);
        if (known == 0 || known <= lead || !source_ref->shardable() || !source_dis->shardable()) {
            if (root) log_line(L_ERROR, kTarget, "--ranks needs two regular planar-YUV files of known length");
            return EXIT_FAILURE;
        }
        uint32_t total = (uint32_t)(known - lead); // decode indices available
        if (opts.frames > 0) total = std::min(total, opts.frames);
        if (root) { log_source("reference", *source_ref); log_source("distorted", *source_dis); }
        const uint32_t w = source_ref->width(), h = source_ref->height();
        if (batch == 0) batch = auto_batch(w, h);
        set_concurrent_streams(2 * (unsigned)renv.world); // the ranks' reader threads share the usable CPUs of the node
        source_ref.reset(); source_dis.reset();
        if (known < 20000) tm_set_placement_candidates(1);
        try {
            // The transport is made AFTER the block's engines (inside `ready`, which every rank reaches exactly once): the runtime binds a stream to
            // one of its four hardware queues when the stream is created, and a communicator that exists first -- RCCL creates streams of its own --
            // takes the queues the engine's side and upload streams would have had to themselves (profiles/r06y6_queue_map.log; `--ranks 1` over
            // RCCL then ran at 0.83 x the one-device rate, profiles/r06y8_ranks_order.log).
            std::unique_ptr<RankTransport> transport;
            auto start = std::chrono::steady_clock::now();
            uint32_t lo = 0, hi = 0;
            shard_range(total, (uint32_t)renv.rank, (uint32_t)renv.world, lo, hi);
            Block blk;
            // rank 0's clock starts where the one-device run's does: engines created, rings page-locked (the other ranks set up at the same time; the
            // figure then covers rank 0's block, the wait for the slowest rank and the reduce)
            // rank 0 holds the FIRST block: its lines go out as they are computed, like the one-device run's; the other blocks' follow the reduce
            if (root) output_prepare(output, metrics, std::cout);
            // (the clock is stopped while the block's engines and page-locked rings are freed: the one-device run frees its own after its report)
            auto computed_at = start;
            score_block(w, h, lo, hi, blk,
                        [&] {
                            transport = make_rank_transport(renv);
                            if (root) log_line(L_DEBUG, kTarget, std::string("ranks: ") + std::to_string(renv.world) + " over " + transport->name());
                            start = std::chrono::steady_clock::now();
                        },
                        root ? std::function<void(const FrameScores &)>([&](const FrameScores &fs) { output_single_score(output, fs, std::cout); }) : nullptr,
                        [&] { computed_at = std::chrono::steady_clock::now(); });
            start += std::chrono::steady_clock::now() - computed_at;
            ScoreVector sv(metrics, total);
            size_t k = 0;
            for (uint32_t dc = lo; dc < hi && k < blk.scores.size(); ++dc) {
                if (opts.every > 1 && dc != 0 && dc % opts.every != 0) continue; // lib.rs:391-394
                sv.put(dc, blk.scores[k++]);
            }
            if (k != blk.scores.size()) throw std::runtime_error("a block produced more scores than it has selected frames");
            sv.add_decoded(blk.decoded);
            transport->reduce_sum_to_root(sv.v); // the ONE collective of the path
            if (!root) return EXIT_SUCCESS;
            const std::vector<FrameScores> all = sv.frames();
            for (size_t i = blk.scores.size(); i < all.size(); ++i) output_single_score(output, all[i], std::cout); // (rank 0's own are out already)
            return report(all, sv.decoded(), w, h, start, std::to_string(renv.world) + " ranks (" + transport->name() + ")");
        } catch (const RankPeerLost &e) { // not this rank's failure: the launcher reports the rank that went away
            std::cout.flush();
            log_line(L_WARN, kTarget, "rank " + std::to_string(renv.rank) + " gives up : " + e.what());
            return RANK_PEER_LOST;
        } catch (const std::exception &e) {
            std::cout.flush();
            log_line(L_ERROR, kTarget, "Computation failed (rank " + std::to_string(renv.rank) + ") : " + e.what());
            return EXIT_FAILURE;
        }
    }

    // ---- frame-pair sharding over several GPUs (the reference is single-GPU: device 0 hard-coded, lib.rs:442).
    // One host thread per device, each with its own sources (opened on the same files) and its own engines; decode indices
    // [0, L) are cut into contiguous blocks, every thread runs the reference's selection loop on its block, and the per-frame
    // scores are concatenated in block order: the output is byte-identical to the single-device run.  (bench.py measures the
    // one-process-per-GPU arrangement with the RCCL reduce; inside one process the "reduce" is this concatenation.)
    {
        int visible = tm_device_count();
        if (visible < 1) visible = 1;
        // TM_SHARE_DEVICE=1 (tests on a 1-GPU box): the shards share the visible devices round-robin
        const bool share = getenv("TM_SHARE_DEVICE") && atoi(getenv("TM_SHARE_DEVICE")) != 0;
        uint32_t want = devices == 0 ? (uint32_t)visible : devices;
        if (want > 1 && !share && want > (uint32_t)visible) {
            log_line(L_ERROR, kTarget, "--devices " + std::to_string(want) + " but only " + std::to_string(visible) + " GPU(s) visible");
            return EXIT_FAILURE;
        }
        const size_t known = std::min(source_ref->frame_count(), source_dis->frame_count());
        const uint32_t lead = opts.skip + std::max(opts.skip_ref, opts.skip_dis);
        if (want > 1 && (ref_is_stdin || dis_is_stdin || known == 0 || known <= lead || !source_ref->shardable() || !source_dis->shardable())) {
            log_line(L_WARN, kTarget, "--devices needs two regular planar-YUV files of known length: running on one device");
            want = 1;
        }
        if (want > 1 && loop != Loop::Batched) log_line(L_WARN, kTarget, "--loop reference / deferred run on one device: --devices ignored");
        if (in_flight_given && loop != Loop::Deferred) log_line(L_WARN, kTarget, "--in-flight belongs to --loop deferred: ignored");
        if (want > 1 && loop != Loop::Batched) want = 1;
        if (want > 1) {
            if (metrics.mask() == 0) { log_line(L_ERROR, kTarget, "Could not initialize engine : no metric selected (-m psnr|ssim|msssim|ssimulacra2)"); return EXIT_FAILURE; }
            uint32_t total = (uint32_t)(known - lead); // decode indices available
            if (opts.frames > 0) total = std::min(total, opts.frames);
            want = std::min(want, std::max(1u, total));
            const uint32_t per = (total + want - 1) / want;
            log_source("reference", *source_ref);
            log_source("distorted", *source_dis);
            const uint32_t w = source_ref->width(), h = source_ref->height();
            if (batch == 0) batch = auto_batch(w, h);
            set_concurrent_streams(2 * want); // every shard reads its own pair of streams: the reader threads share the usable CPUs
            source_ref.reset(); source_dis.reset(); // every shard opens its own
            if (known < 20000) tm_set_placement_candidates(1); // as below: the search pays off on long streams only
            struct Shard { Block blk; std::string err; };
            std::vector<Shard> shards(want);
            const auto start = std::chrono::steady_clock::now();
            std::vector<std::thread> th;
            for (uint32_t r = 0; r < want; ++r)
                th.emplace_back([&, r] {
                    Shard &sh = shards[r];
                    try {
                        const uint32_t lo = std::min(total, r * per), hi = std::min(total, lo + per);
                        if (lo >= hi) return;
                        init_hip((int)((device + r) % (uint32_t)std::max(1, visible)));
                        score_block(w, h, lo, hi, sh.blk);
                    } catch (const std::exception &e) { sh.err = e.what(); }
                });
            for (auto &t : th) t.join();
            for (const Shard &sh : shards)
                if (!sh.err.empty()) { log_line(L_ERROR, kTarget, "Computation failed : " + sh.err); return EXIT_FAILURE; }
            output_prepare(output, metrics, std::cout);
            std::vector<FrameScores> all;
            uint32_t decoded = 0;
            for (const Shard &sh : shards) {
                for (const FrameScores &fs : sh.blk.scores) { output_single_score(output, fs, std::cout); all.push_back(fs); }
                decoded += sh.blk.decoded;
            }
            return report(all, decoded, w, h, start, std::to_string(want) + " devices");
        }
    }

    std::unique_ptr<TurboMetrics> turbo;
    try {
        if (metrics.mask() == 0 && !metrics.xpsnr && !metrics.motion && !metrics.vif && !metrics.adm && !metrics.scenes && !metrics.cambi && !metrics.flip && !metrics.psnr_yuv && !metrics.ssim_yuv && !metrics.psnr_hvs && !metrics.psnr_hvs_m && !metrics.ciede && !metrics.siti && !metrics.gmsd && !metrics.haarpsi && !metrics.deitp && !metrics.mdsi) throw std::runtime_error("no metric selected (-m psnr|ssim|msssim|ssimulacra2)");
        // a source that knows its length never needs more slots than it has pairs (a single image pair: one slot, one engine)
        const size_t known = std::min(source_ref->frame_count(), source_dis->frame_count());
        if (batch == 0) batch = auto_batch(source_ref->width(), source_ref->height());
        if (known > 0 && known <= batch) { batch = (uint32_t)known; pipeline = false; }
        if (loop != Loop::Batched) { batch = 1; pipeline = false; } // one pair per call, like the reference
        // the placement search of tm_engine_create (~10 ms per candidate and engine) pays off on long streams only
        if (known > 0 && known < 20000) tm_set_placement_candidates(1);
        turbo = std::make_unique<TurboMetrics>(source_ref->width(), source_ref->height(), metrics, batch, pipeline);
        if (full_sums) turbo->set_full_sums(true);
        if (metrics.xpsnr) { // --xpsnr-fps, else the Y4M frame rate, else ffmpeg's rawvideo default of 25 fps
            const auto fr = source_ref->frame_rate();
            if (xpsnr_fps_num) turbo->set_xpsnr_fps(xpsnr_fps_num, xpsnr_fps_den);
            else if (fr.first && fr.second) turbo->set_xpsnr_fps(fr.first, fr.second);
        }
        for (auto &t : tune) if (t.first < 100) turbo->debug_set_param(t.first, t.second);
        // --loop deferred: every engine of the turn exists before the clock starts (the reference allocates everything up front too,
        // ssimulacra2-cuda/src/lib.rs:21)
        if (loop == Loop::Deferred) turbo->set_deferred_depth(in_flight_pairs, true);
    } catch (const std::exception &e) {
        log_line(L_ERROR, kTarget, std::string("Could not initialize engine : ") + e.what());
        return EXIT_FAILURE;
    }

    log_source("reference", *source_ref);
    log_source("distorted", *source_dis);
    // the sources' frame rings are page-locked here, before the clock starts: the counterpart of the surface pool the reference's decoder
    // allocates when it is created (its clock, main.rs:252, starts after decoders and engine exist too)
    {   // --tune 100=<pairs in flight> / 101=<pairs per fence>: host-side upload tuning (the rest goes to the engines)
        size_t in_flight = 4, fence_every = 1;
        bool given = false;
        for (auto &t : tune) { if (t.first == 100) { in_flight = (size_t)t.second; given = true; } if (t.first == 101) { fence_every = (size_t)t.second; given = true; } }
        if (given) TurboMetrics::set_upload_tuning(in_flight, fence_every); // (default: by picture size, TurboMetrics::prepare_sources)
    }
    try { TurboMetrics::prepare_sources(*source_ref, *source_dis, opts, loop == Loop::Deferred ? in_flight_pairs : 0); }
    catch (const std::exception &e) { log_line(L_ERROR, kTarget, std::string("Could not initialize the sources : ") + e.what()); return EXIT_FAILURE; }
    log_line(L_DEBUG, kTarget, "Initialized, now processing ...");

    const auto start = std::chrono::steady_clock::now();
    output_prepare(output, metrics, std::cout);
    MetricsResults results;
    uint32_t decode_count = 0;
    try {
        if (loop == Loop::Batched) {
            results = turbo->compute_all(*source_ref, *source_dis, opts,
                                         [&](const FrameScores &r) { output_single_score(output, r, std::cout); }, &decode_count);
        } else {
            // The reference's own loop, statement for statement (turbo-metrics-cli/src/main.rs:284-326): one pair per call.  `deferred`
            // is the same loop with the two-line change INTEGRATION.md section 3 shows: submit pair k, then collect pair k - 1.
            const auto cref = source_ref->color_characteristics(), cdis = source_dis->color_characteristics();
            std::vector<FrameScores> all;
            const auto emit = [&](const FrameScores &r) { output_single_score(output, r, std::cout); all.push_back(r); };
            source_ref->skip_frames(opts.skip_ref + opts.skip);
            source_dis->skip_frames(opts.skip_dis + opts.skip);
            HwFrame fref, fdis;
            std::deque<uint64_t> tickets; // --loop deferred: pairs in flight, oldest first
            while (source_ref->next_frame(fref) && source_dis->next_frame(fdis)) {
                if (opts.every > 1 && decode_count != 0 && decode_count % opts.every != 0) { decode_count += 1; continue; }
                if (opts.frames > 0 && decode_count >= opts.frames) break;
                decode_count += 1;
                if (loop == Loop::Reference) {
                    emit(turbo->compute_one(fref, cref, fdis, cdis));
                } else {
                    tickets.push_back(turbo->compute_one_deferred(fref, cref, fdis, cdis));
                    if (tickets.size() >= in_flight_pairs) { emit(turbo->collect(tickets.front())); tickets.pop_front(); }
                }
            }
            for (uint64_t t : tickets) emit(turbo->collect(t));
            results = aggregate_scores(all, metrics);
        }
    } catch (const std::exception &e) {
        std::cout.flush();
        log_line(L_ERROR, kTarget, std::string("Computation failed : ") + e.what());
        return EXIT_FAILURE;
    }
    const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - start);
    const long long dms = ms.count() > 0 ? ms.count() : 1; // the reference divides by as_millis() (main.rs:332)
    const unsigned long long fps = (unsigned long long)results.frame_count * 1000ull / (unsigned long long)dms;
    const double perf = (double)source_ref->width() * (double)source_ref->height() * (double)results.frame_count / (double)dms / 1000.0;
    char perf_s[64];
    snprintf(perf_s, sizeof perf_s, "%.3f", perf);
    log_line(L_INFO, kTarget, "Processed: " + std::to_string(results.frame_count) + " (decoded: ~" + std::to_string(decode_count + opts.skip) +
                                  ") frame pairs in " + format_duration(ms) + " (" + std::to_string(fps) + " fps) (Mpx/s: " + perf_s + ")");
    {
        const TurboMetrics::LoopTiming &t = turbo->loop_timing();
        char b[256];
        snprintf(b, sizeof b, "main thread: %.0f ms waiting for an upload slot, %.0f ms for the sources, %.0f ms handing frames to the engine, %.0f ms submitting, %.0f ms waiting for results + output",
                 t.wait_upload * 1e3, t.wait_frames * 1e3, t.set_frames * 1e3, t.submit * 1e3, t.drain * 1e3);
        log_line(L_DEBUG, kTarget, b);
    }
    output_results(output, results, std::cout);
    std::cout.flush();
    return EXIT_SUCCESS;
}
