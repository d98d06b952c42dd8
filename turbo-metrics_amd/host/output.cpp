// output.cpp -- see output.hpp
#include "output.hpp"

#include <sstream>
#include <vector>

#include "rust_fmt.hpp"

namespace tm_host {

bool parse_output(const std::string &s, Output &out)
{
    if (s == "default") out = Output::Default;
    else if (s == "json") out = Output::Json;
    else if (s == "json-lines") out = Output::JsonLines;
    else if (s == "csv") out = Output::CSV;
    else return false;
    return true;
}

namespace {

struct Named { const char *name; double value; };

std::vector<Named> stat_fields(const Stats &s)
{
    return {{"min", s.min}, {"max", s.max}, {"mean", s.mean}, {"var", s.var}, {"sample_var", s.sample_var}, {"stddev", s.stddev},
            {"sample_stddev", s.sample_stddev}, {"p1", s.p1}, {"p5", s.p5}, {"p50", s.p50}, {"p95", s.p95}, {"p99", s.p99}};
}

void csv_header(bool psnr, bool ssim, bool msssim, bool ssimu, std::ostream &os, bool xpsnr = false, bool motion = false, bool vif = false, bool adm = false,
                bool scene = false, bool cambi = false, bool cambi_ref = false, bool flip = false, bool psnr_yuv = false, bool ssim_yuv = false, bool psnr_hvs = false,
                bool psnr_hvs_m = false, bool ciede = false, bool siti = false, bool gmsd = false, bool haarpsi = false, bool deitp = false,
                bool mdsi = false)
{
    bool first = true;
    auto put = [&](bool on, const char *n) { if (on) { os << (first ? "" : ",") << n; first = false; } };
    put(psnr, "psnr"); put(ssim, "ssim"); put(msssim, "msssim"); put(ssimu, "ssimulacra2");
    put(xpsnr, "xpsnr_y"); put(xpsnr, "xpsnr_u"); put(xpsnr, "xpsnr_v");
    put(motion, "motion"); put(motion, "motion2");
    put(vif, "vif_scale0"); put(vif, "vif_scale1"); put(vif, "vif_scale2"); put(vif, "vif_scale3"); put(vif, "vif");
    put(adm, "adm2"); put(adm, "adm_scale0"); put(adm, "adm_scale1"); put(adm, "adm_scale2"); put(adm, "adm_scale3");
    put(scene, "scene_score"); put(scene, "scene_cut");
    for (const char *n : {"cambi", "cambi_scale0", "cambi_scale1", "cambi_scale2", "cambi_scale3", "cambi_scale4"}) put(cambi, n);
    for (const char *n : {"cambi_ref", "cambi_ref_scale0", "cambi_ref_scale1", "cambi_ref_scale2", "cambi_ref_scale3", "cambi_ref_scale4"}) put(cambi_ref, n);
    put(flip, "flip"); put(flip, "flip_min"); put(flip, "flip_max");
    for (int k = 0; k < 8; ++k) put(k < 4 ? psnr_yuv : ssim_yuv, kYuvNames[k]);
    put(psnr_hvs, kHvsNames[0]); put(psnr_hvs_m, kHvsNames[1]);
    put(ciede, kCiedeNames[0]); put(ciede, kCiedeNames[1]);
    put(siti, "si"); put(siti, "ti");
    put(gmsd, kGmsdNames[0]); put(gmsd, kGmsdNames[1]);
    put(haarpsi, "haarpsi");
    put(deitp, kItpNames[0]); put(deitp, kItpNames[1]);
    put(mdsi, "mdsi");
    if (first) os << "\"\""; // csv::Writer writes an empty record as ""
    os << "\n";
}

void csv_row(const std::optional<double> &a, const std::optional<double> &b, const std::optional<double> &c, const std::optional<double> &d,
             std::ostream &os, const std::optional<double> &xy = std::nullopt, const std::optional<double> &xu = std::nullopt,
             const std::optional<double> &xv = std::nullopt, const std::optional<double> &mo = std::nullopt,
             const std::optional<double> &mo2 = std::nullopt, const std::optional<double> *vif5 = nullptr,
             const std::optional<double> *adm5 = nullptr, const std::optional<double> &scene_score = std::nullopt,
             const std::optional<bool> &scene_cut = std::nullopt, const std::optional<double> *cambi6 = nullptr,
             const std::optional<double> *cambi_ref6 = nullptr, const std::optional<double> *flip3 = nullptr, const std::optional<double> *yuv8 = nullptr,
             const std::optional<double> *hvs2 = nullptr, const std::optional<double> *ciede2 = nullptr, const std::optional<double> &si = std::nullopt,
             const std::optional<double> &ti = std::nullopt, const std::optional<double> *gmsd2 = nullptr,
             const std::optional<double> &haarpsi = std::nullopt, const std::optional<double> *deitp2 = nullptr,
             const std::optional<double> &mdsi = std::nullopt)
{
    bool first = true;
    auto put = [&](const std::optional<double> &v) { if (v) { os << (first ? "" : ",") << display(*v); first = false; } };
    put(a); put(b); put(c); put(d); put(xy); put(xu); put(xv); put(mo); put(mo2);
    if (vif5)
        for (int k = 0; k < 5; ++k) put(vif5[k]);
    if (adm5)
        for (int k = 0; k < 5; ++k) put(adm5[k]);
    put(scene_score);
    if (scene_cut) { os << (first ? "" : ",") << (*scene_cut ? 1 : 0); first = false; } // a flag: 0 / 1, not a float
    if (cambi6)
        for (int k = 0; k < 6; ++k) put(cambi6[k]);
    if (cambi_ref6)
        for (int k = 0; k < 6; ++k) put(cambi_ref6[k]);
    if (flip3)
        for (int k = 0; k < 3; ++k) put(flip3[k]);
    if (yuv8)
        for (int k = 0; k < 8; ++k) put(yuv8[k]);
    if (hvs2)
        for (int k = 0; k < 2; ++k) put(hvs2[k]);
    if (ciede2)
        for (int k = 0; k < 2; ++k) put(ciede2[k]);
    put(si); put(ti);
    if (gmsd2)
        for (int k = 0; k < 2; ++k) put(gmsd2[k]);
    put(haarpsi);
    if (deitp2)
        for (int k = 0; k < 2; ++k) put(deitp2[k]);
    put(mdsi);
    if (first) os << "\"\"";
    os << "\n";
}

// [0, 4, 7]
std::string index_list(const std::vector<size_t> &v, const char *sep)
{
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? sep : "") + std::to_string(v[i]);
    return s + "]";
}

std::string frame_scores_json(const FrameScores &r)
{
    std::string s = "{";
    bool first = true;
    auto put = [&](const char *n, const std::optional<double> &v) {
        if (!v) return; // skip_serializing_if = "Option::is_none"
        s += (first ? "\"" : ",\"") + std::string(n) + "\":" + json_number(*v);
        first = false;
    };
    put("psnr", r.psnr); put("ssim", r.ssim); put("msssim", r.msssim); put("ssimulacra2", r.ssimulacra2);
    put("xpsnr_y", r.xpsnr_y); put("xpsnr_u", r.xpsnr_u); put("xpsnr_v", r.xpsnr_v);
    put("motion", r.motion); put("motion2", r.motion2);
    put("vif_scale0", r.vif_scale[0]); put("vif_scale1", r.vif_scale[1]); put("vif_scale2", r.vif_scale[2]); put("vif_scale3", r.vif_scale[3]);
    put("vif", r.vif);
    put("adm2", r.adm2);
    put("adm_scale0", r.adm_scale[0]); put("adm_scale1", r.adm_scale[1]); put("adm_scale2", r.adm_scale[2]); put("adm_scale3", r.adm_scale[3]);
    put("scene_score", r.scene_score);
    if (r.scene_cut) { s += (first ? "\"" : ",\"") + std::string("scene_cut\":") + (*r.scene_cut ? "1" : "0"); first = false; }
    static const char *const cn[5] = {"cambi_scale0", "cambi_scale1", "cambi_scale2", "cambi_scale3", "cambi_scale4"};
    static const char *const rn[5] = {"cambi_ref_scale0", "cambi_ref_scale1", "cambi_ref_scale2", "cambi_ref_scale3", "cambi_ref_scale4"};
    put("cambi", r.cambi);
    for (int k = 0; k < 5; ++k) put(cn[k], r.cambi_scale[k]);
    put("cambi_ref", r.cambi_ref);
    for (int k = 0; k < 5; ++k) put(rn[k], r.cambi_ref_scale[k]);
    put("flip", r.flip); put("flip_min", r.flip_min); put("flip_max", r.flip_max);
    for (int k = 0; k < 8; ++k) put(kYuvNames[k], r.yuv[k]);
    for (int k = 0; k < 2; ++k) put(kHvsNames[k], r.hvs[k]);
    for (int k = 0; k < 2; ++k) put(kCiedeNames[k], r.ciede[k]);
    put("si", r.si); put("ti", r.ti);
    for (int k = 0; k < 2; ++k) put(kGmsdNames[k], r.gmsd[k]);
    put("haarpsi", r.haarpsi);
    for (int k = 0; k < 2; ++k) put(kItpNames[k], r.deitp[k]);
    put("mdsi", r.mdsi);
    return s + "}";
}

} // namespace

std::string stats_debug_pretty(const Stats &s)
{
    std::string out = "Stats {\n";
    for (const Named &f : stat_fields(s)) out += "    " + std::string(f.name) + ": " + debug(f.value) + ",\n";
    return out + "}";
}

std::string stats_json(const Stats &s, int indent, bool pretty)
{
    std::string out = "{";
    const std::string pad((size_t)indent + 2, ' ');
    bool first = true;
    for (const Named &f : stat_fields(s)) {
        if (!first) out += ",";
        if (pretty) out += "\n" + pad;
        out += "\"" + std::string(f.name) + "\":" + (pretty ? " " : "") + json_number(f.value);
        first = false;
    }
    if (pretty) out += "\n" + std::string((size_t)indent, ' ');
    return out + "}";
}

void output_prepare(Output o, const Metrics &m, std::ostream &os)
{
    if (o == Output::CSV) csv_header(m.psnr, m.ssim, m.msssim, m.ssimulacra2, os, m.xpsnr, m.motion, m.vif, m.adm, m.scenes, m.cambi, m.cambi && m.cambi_ref, m.flip, m.psnr_yuv, m.ssim_yuv,
                                     m.psnr_hvs, m.psnr_hvs_m, m.ciede, m.siti, m.gmsd, m.haarpsi, m.deitp, m.mdsi);
}

void output_single_score(Output o, const FrameScores &r, std::ostream &os)
{
    if (o == Output::JsonLines) os << frame_scores_json(r) << "\n";
    else if (o == Output::CSV) {
        const std::optional<double> v5[5] = {r.vif_scale[0], r.vif_scale[1], r.vif_scale[2], r.vif_scale[3], r.vif};
        const std::optional<double> a5[5] = {r.adm2, r.adm_scale[0], r.adm_scale[1], r.adm_scale[2], r.adm_scale[3]};
        const std::optional<double> c6[6] = {r.cambi, r.cambi_scale[0], r.cambi_scale[1], r.cambi_scale[2], r.cambi_scale[3], r.cambi_scale[4]};
        const std::optional<double> r6[6] = {r.cambi_ref, r.cambi_ref_scale[0], r.cambi_ref_scale[1], r.cambi_ref_scale[2], r.cambi_ref_scale[3], r.cambi_ref_scale[4]};
        const std::optional<double> f3[3] = {r.flip, r.flip_min, r.flip_max};
        csv_row(r.psnr, r.ssim, r.msssim, r.ssimulacra2, os, r.xpsnr_y, r.xpsnr_u, r.xpsnr_v, r.motion, r.motion2, v5, a5, r.scene_score, r.scene_cut, c6, r6, f3, r.yuv, r.hvs, r.ciede, r.si, r.ti, r.gmsd, r.haarpsi, r.deitp, r.mdsi);
    }
}

void output_results(Output o, const MetricsResults &r, std::ostream &os)
{
    switch (o) {
    case Output::Default:
        if (r.psnr) os << "PSNR: " << stats_debug_pretty(r.psnr->stats) << "\n";
        if (r.ssim) os << "SSIM: " << stats_debug_pretty(r.ssim->stats) << "\n";
        if (r.msssim) os << "MSSSIM: " << stats_debug_pretty(r.msssim->stats) << "\n";
        if (r.ssimulacra2) os << "SSIMULACRA2: " << stats_debug_pretty(r.ssimulacra2->stats) << "\n";
        if (r.xpsnr_y) {
            os << "XPSNR_Y: " << stats_debug_pretty(r.xpsnr_y->stats) << "\n";
            os << "XPSNR_U: " << stats_debug_pretty(r.xpsnr_u->stats) << "\n";
            os << "XPSNR_V: " << stats_debug_pretty(r.xpsnr_v->stats) << "\n";
            os << "XPSNR (sequence): y " << debug(*r.xpsnr_y->sequence) << ", u " << debug(*r.xpsnr_u->sequence) << ", v "
               << debug(*r.xpsnr_v->sequence) << "\n";
        }
        if (r.motion) os << "MOTION: " << stats_debug_pretty(r.motion->stats) << "\n";
        if (r.motion2) os << "MOTION2: " << stats_debug_pretty(r.motion2->stats) << "\n";
        if (r.vif) {
            for (int k = 0; k < 4; ++k) os << "VIF_SCALE" << k << ": " << stats_debug_pretty(r.vif_scale[k]->stats) << "\n";
            os << "VIF: " << stats_debug_pretty(r.vif->stats) << "\n";
        }
        if (r.adm2) {
            os << "ADM2: " << stats_debug_pretty(r.adm2->stats) << "\n";
            for (int k = 0; k < 4; ++k) os << "ADM_SCALE" << k << ": " << stats_debug_pretty(r.adm_scale[k]->stats) << "\n";
        }
        if (r.scene_score) {
            os << "SCENE_SCORE: " << stats_debug_pretty(r.scene_score->stats) << "\n";
            os << "SCENE_STARTS: " << index_list(r.scene_starts, ", ") << "\n";
        }
        if (r.cambi) {
            os << "CAMBI: " << stats_debug_pretty(r.cambi->stats) << "\n";
            for (int k = 0; k < 5; ++k) os << "CAMBI_SCALE" << k << ": " << stats_debug_pretty(r.cambi_scale[k]->stats) << "\n";
        }
        if (r.cambi_ref) {
            os << "CAMBI_REF: " << stats_debug_pretty(r.cambi_ref->stats) << "\n";
            for (int k = 0; k < 5; ++k) os << "CAMBI_REF_SCALE" << k << ": " << stats_debug_pretty(r.cambi_ref_scale[k]->stats) << "\n";
        }
        if (r.flip) {
            os << "FLIP: " << stats_debug_pretty(r.flip->stats) << "\n";
            os << "FLIP_MIN: " << stats_debug_pretty(r.flip_min->stats) << "\n";
            os << "FLIP_MAX: " << stats_debug_pretty(r.flip_max->stats) << "\n";
        }
        for (int g = 0; g < 2; ++g) { // psnr_y .. psnr_avg, then ssim_y .. ssim_all, each with its sequence line
            if (!r.yuv[4 * g]) continue;
            for (int k = 4 * g; k < 4 * g + 4; ++k) {
                std::string n = kYuvNames[k];
                for (char &c : n) c = (char)toupper((unsigned char)c);
                os << n << ": " << stats_debug_pretty(r.yuv[k]->stats) << "\n";
            }
            os << (g ? "SSIM-YUV (sequence): y " : "PSNR-YUV (sequence): y ") << debug(*r.yuv[4 * g]->sequence) << ", u " << debug(*r.yuv[4 * g + 1]->sequence)
               << ", v " << debug(*r.yuv[4 * g + 2]->sequence) << (g ? ", all " : ", avg ") << debug(*r.yuv[4 * g + 3]->sequence) << "\n";
        }
        for (int k = 0; k < 2; ++k) { // psnr_hvs, psnr_hvs_m, each with its sequence line
            if (!r.hvs[k]) continue;
            os << (k ? "PSNR_HVS_M: " : "PSNR_HVS: ") << stats_debug_pretty(r.hvs[k]->stats) << "\n";
            os << (k ? "PSNR-HVS-M (sequence): " : "PSNR-HVS (sequence): ") << debug(*r.hvs[k]->sequence) << "\n";
        }
        for (int k = 0; k < 2; ++k) { // ciede2000, ciede2000_de, each with its sequence line
            if (!r.ciede[k]) continue;
            os << (k ? "CIEDE2000_DE: " : "CIEDE2000: ") << stats_debug_pretty(r.ciede[k]->stats) << "\n";
            os << (k ? "CIEDE2000 mean dE00 (sequence): " : "CIEDE2000 (sequence): ") << debug(*r.ciede[k]->sequence) << "\n";
        }
        if (r.si) { // ti's statistics: the frames after the first; the sequence values are the maxima
            os << "SI: " << stats_debug_pretty(r.si->stats) << "\n";
            os << "TI: " << stats_debug_pretty(r.ti->stats) << "\n";
            os << "SI / TI (sequence): si " << debug(*r.si->sequence) << ", ti " << debug(*r.ti->sequence) << "\n";
        }
        for (int k = 0; k < 2; ++k) { // gmsd, gmsm, each with its sequence line: pooled over all positions of all pairs
            if (!r.gmsd[k]) continue;
            os << (k ? "GMSM: " : "GMSD: ") << stats_debug_pretty(r.gmsd[k]->stats) << "\n";
            os << (k ? "GMSM (sequence): " : "GMSD (sequence): ") << debug(*r.gmsd[k]->sequence) << "\n";
        }
        if (r.haarpsi) { // with its sequence line: from the summed Q and WS of all pairs
            os << "HaarPSI: " << stats_debug_pretty(r.haarpsi->stats) << "\n";
            os << "HaarPSI (sequence): " << debug(*r.haarpsi->sequence) << "\n";
        }
        for (int k = 0; k < 2; ++k) { // deitp, deitp_max, each with its sequence line
            if (!r.deitp[k]) continue;
            os << (k ? "DEITP_MAX: " : "DEITP: ") << stats_debug_pretty(r.deitp[k]->stats) << "\n";
            os << (k ? "dE ITP max (sequence): " : "dE ITP mean (sequence): ") << debug(*r.deitp[k]->sequence) << "\n";
        }
        if (r.mdsi) { // the sequence value is the mean of the pairs' values
            os << "MDSI: " << stats_debug_pretty(r.mdsi->stats) << "\n";
            os << "MDSI (sequence): " << debug(*r.mdsi->sequence) << "\n";
        }
        break;
    case Output::Json: { // serde_json::to_string_pretty: two-space indent, `"key": value`
        os << "{\n  \"frame_count\": " << r.frame_count;
        auto put = [&](const char *n, const std::optional<MetricAggregate> &a) {
            if (!a) return;
            os << ",\n  \"" << n << "\": {\n    \"scores\": [";
            for (size_t i = 0; i < a->scores.size(); ++i) os << (i ? ",\n      " : "\n      ") << json_number(a->scores[i]);
            os << (a->scores.empty() ? "]" : "\n    ]") << ",\n    \"stats\": " << stats_json(a->stats, 4, true);
            if (a->sequence) os << ",\n    \"sequence\": " << json_number(*a->sequence);
            os << "\n  }";
        };
        put("psnr", r.psnr); put("ssim", r.ssim); put("msssim", r.msssim); put("ssimulacra2", r.ssimulacra2);
        put("xpsnr_y", r.xpsnr_y); put("xpsnr_u", r.xpsnr_u); put("xpsnr_v", r.xpsnr_v);
        put("motion", r.motion); put("motion2", r.motion2);
        put("vif_scale0", r.vif_scale[0]); put("vif_scale1", r.vif_scale[1]); put("vif_scale2", r.vif_scale[2]); put("vif_scale3", r.vif_scale[3]);
        put("vif", r.vif);
        put("adm2", r.adm2);
        put("adm_scale0", r.adm_scale[0]); put("adm_scale1", r.adm_scale[1]); put("adm_scale2", r.adm_scale[2]); put("adm_scale3", r.adm_scale[3]);
        put("scene_score", r.scene_score);
        if (r.scene_score) os << ",\n  \"scene_starts\": " << index_list(r.scene_starts, ", ");
        {
            static const char *const cn[5] = {"cambi_scale0", "cambi_scale1", "cambi_scale2", "cambi_scale3", "cambi_scale4"};
            static const char *const rn[5] = {"cambi_ref_scale0", "cambi_ref_scale1", "cambi_ref_scale2", "cambi_ref_scale3", "cambi_ref_scale4"};
            put("cambi", r.cambi);
            for (int k = 0; k < 5; ++k) put(cn[k], r.cambi_scale[k]);
            put("cambi_ref", r.cambi_ref);
            for (int k = 0; k < 5; ++k) put(rn[k], r.cambi_ref_scale[k]);
        }
        put("flip", r.flip); put("flip_min", r.flip_min); put("flip_max", r.flip_max);
        for (int k = 0; k < 8; ++k) put(kYuvNames[k], r.yuv[k]);
        for (int k = 0; k < 2; ++k) put(kHvsNames[k], r.hvs[k]);
        for (int k = 0; k < 2; ++k) put(kCiedeNames[k], r.ciede[k]);
        put("si", r.si); put("ti", r.ti);
        for (int k = 0; k < 2; ++k) put(kGmsdNames[k], r.gmsd[k]);
        put("haarpsi", r.haarpsi);
        for (int k = 0; k < 2; ++k) put(kItpNames[k], r.deitp[k]);
        put("mdsi", r.mdsi);
        os << "\n}\n";
        break;
    }
    case Output::JsonLines: {
        const MetricsStats s = MetricsStats::from(r);
        os << "{\"frame_count\":" << s.frame_count;
        auto put = [&](const char *n, const std::optional<Stats> &st) { if (st) os << ",\"" << n << "\":" << stats_json(*st, 0, false); };
        put("psnr", s.psnr); put("ssim", s.ssim); put("msssim", s.msssim); put("ssimulacra2", s.ssimulacra2);
        auto put_x = [&](const char *n, const std::optional<MetricAggregate> &a) { // the stats, then "sequence"
            if (!a) return;
            const std::string st = stats_json(a->stats, 0, false);
            os << ",\"" << n << "\":" << st.substr(0, st.size() - 1) << ",\"sequence\":" << json_number(*a->sequence) << "}";
        };
        put_x("xpsnr_y", r.xpsnr_y); put_x("xpsnr_u", r.xpsnr_u); put_x("xpsnr_v", r.xpsnr_v);
        if (r.motion) put("motion", r.motion->stats);
        if (r.motion2) put("motion2", r.motion2->stats);
        if (r.vif) {
            static const char *const names[4] = {"vif_scale0", "vif_scale1", "vif_scale2", "vif_scale3"};
            for (int k = 0; k < 4; ++k) put(names[k], r.vif_scale[k]->stats);
            put("vif", r.vif->stats);
        }
        if (r.adm2) {
            static const char *const names[4] = {"adm_scale0", "adm_scale1", "adm_scale2", "adm_scale3"};
            put("adm2", r.adm2->stats);
            for (int k = 0; k < 4; ++k) put(names[k], r.adm_scale[k]->stats);
        }
        if (r.scene_score) {
            put("scene_score", r.scene_score->stats);
            os << ",\"scene_starts\":" << index_list(r.scene_starts, ",");
        }
        if (r.cambi) {
            static const char *const names[5] = {"cambi_scale0", "cambi_scale1", "cambi_scale2", "cambi_scale3", "cambi_scale4"};
            put("cambi", r.cambi->stats);
            for (int k = 0; k < 5; ++k) put(names[k], r.cambi_scale[k]->stats);
        }
        if (r.cambi_ref) {
            static const char *const names[5] = {"cambi_ref_scale0", "cambi_ref_scale1", "cambi_ref_scale2", "cambi_ref_scale3", "cambi_ref_scale4"};
            put("cambi_ref", r.cambi_ref->stats);
            for (int k = 0; k < 5; ++k) put(names[k], r.cambi_ref_scale[k]->stats);
        }
        if (r.flip) { put("flip", r.flip->stats); put("flip_min", r.flip_min->stats); put("flip_max", r.flip_max->stats); }
        for (int k = 0; k < 8; ++k) put_x(kYuvNames[k], r.yuv[k]);
        for (int k = 0; k < 2; ++k) put_x(kHvsNames[k], r.hvs[k]);
        for (int k = 0; k < 2; ++k) put_x(kCiedeNames[k], r.ciede[k]);
        put_x("si", r.si); put_x("ti", r.ti);
        for (int k = 0; k < 2; ++k) put_x(kGmsdNames[k], r.gmsd[k]);
        put_x("haarpsi", r.haarpsi);
        for (int k = 0; k < 2; ++k) put_x(kItpNames[k], r.deitp[k]);
        put_x("mdsi", r.mdsi);
        os << "}\n";
        break;
    }
    case Output::CSV:
        csv_header((bool)r.psnr, (bool)r.ssim, (bool)r.msssim, (bool)r.ssimulacra2, os, (bool)r.xpsnr_y, (bool)r.motion, (bool)r.vif, (bool)r.adm2, (bool)r.scene_score, (bool)r.cambi, (bool)r.cambi_ref, (bool)r.flip, (bool)r.yuv[0], (bool)r.yuv[4],
                   (bool)r.hvs[0], (bool)r.hvs[1], (bool)r.ciede[0], (bool)r.si, (bool)r.gmsd[0], (bool)r.haarpsi, (bool)r.deitp[0], (bool)r.mdsi);
        for (size_t i = 0, starts = 0; i < r.frame_count; ++i) {
            auto at = [&](const std::optional<MetricAggregate> &a) { return a ? std::optional<double>(a->scores[i]) : std::nullopt; };
            const std::optional<double> v5[5] = {at(r.vif_scale[0]), at(r.vif_scale[1]), at(r.vif_scale[2]), at(r.vif_scale[3]), at(r.vif)};
            const std::optional<double> a5[5] = {at(r.adm2), at(r.adm_scale[0]), at(r.adm_scale[1]), at(r.adm_scale[2]), at(r.adm_scale[3])};
            const std::optional<double> c6[6] = {at(r.cambi), at(r.cambi_scale[0]), at(r.cambi_scale[1]), at(r.cambi_scale[2]), at(r.cambi_scale[3]), at(r.cambi_scale[4])};
            const std::optional<double> r6[6] = {at(r.cambi_ref), at(r.cambi_ref_scale[0]), at(r.cambi_ref_scale[1]), at(r.cambi_ref_scale[2]), at(r.cambi_ref_scale[3]), at(r.cambi_ref_scale[4])};
            const std::optional<double> f3[3] = {at(r.flip), at(r.flip_min), at(r.flip_max)};
            const std::optional<double> h2[2] = {at(r.hvs[0]), at(r.hvs[1])};
            const std::optional<double> e2[2] = {at(r.ciede[0]), at(r.ciede[1])};
            const std::optional<double> t2[2] = {at(r.deitp[0]), at(r.deitp[1])};
            const std::optional<double> g2[2] = {at(r.gmsd[0]), at(r.gmsd[1])};
            const std::optional<double> y8[8] = {at(r.yuv[0]), at(r.yuv[1]), at(r.yuv[2]), at(r.yuv[3]), at(r.yuv[4]), at(r.yuv[5]), at(r.yuv[6]), at(r.yuv[7])};
            csv_row(at(r.psnr), at(r.ssim), at(r.msssim), at(r.ssimulacra2), os, at(r.xpsnr_y), at(r.xpsnr_u), at(r.xpsnr_v), at(r.motion), at(r.motion2), v5, a5,
                    at(r.scene_score), r.scene_score ? std::optional<bool>(i > 0 && starts < r.scene_starts.size() && r.scene_starts[starts] == i) : std::nullopt, c6, r6, f3, y8, h2, e2,
                    at(r.si), at(r.ti), g2, at(r.haarpsi), t2, at(r.mdsi));
            if (starts < r.scene_starts.size() && r.scene_starts[starts] == i) ++starts; // (frame 0 starts the first scene and is no cut)
        }
        break;
    }
}

} // namespace tm_host
