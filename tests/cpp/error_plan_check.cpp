// The host half of rtgl_error_estimate (raytracer.glsl_amd/csrc/rt_error_plan.hpp) as a stand-alone program: the defaults, the record's
// bounds, the snapshot's life against a transcription of tests/error_mirror.py's Estimator over a scripted history, the three factors bit
// for bit, and the footprint functions against rt_spread_plan's copies; with the argument `replay`, the call's answers to the records and
// states of standard input (tests/cpp/post_replay.hpp).  Built by its test with the address and undefined-behaviour sanitizers
// (tests/test_post_plans.py).
#include "../../raytracer.glsl_amd/csrc/rt_error_plan.hpp"
#include "../../raytracer.glsl_amd/csrc/rt_spread_plan.hpp"
#include "post_replay.hpp"

using namespace rt_error_plan;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static int replay()
{
    const char *who = "rtgl_error_estimate";
    bool tiled = false;
    int width = 0, height = 0;
    Snapshot s;
    for (post_replay::Line line; post_replay::next(line);) {
        if (line.verb == "state") {
            const auto &n = line.n;
            s = Snapshot{};
            tiled = n.at(0) != 0; s.rendered = n.at(1) != 0; s.fn = (int32_t)n.at(2); s.fm = (int32_t)n.at(3); s.first = (int32_t)n.at(4);
            s.snap_epoch = n.at(5) ? s.epoch : s.epoch - 1; width = (int)n.at(6); height = (int)n.at(7);
            continue;
        }
        if (line.verb != who) return 2;
        Params p = default_params();      // the order of rtgl_amd.hip: the record, the tiled refusal, the accumulation and the picture
        post_replay::take(line, p);
        if (post_replay::refuse(kInvalid, who, invalid(p))) continue;
        if (tiled) { std::puts("tiled"); continue; }
        const Refusal no = refused(s, p, width, height);
        if (post_replay::refuse(no.code, who, no.why)) continue;
        const Plan q = plan(s, p);
        std::printf("0 %d %d %d\n", q.usable ? 1 : 0, (int)q.frames_now, (int)q.frames_snapshot);
        taken(s, p, q.keep);
    }
    return 0;
}

// tests/error_mirror.py, class Estimator, without the pictures
struct Mirror {
    long epoch = 1, snap_epoch = 0, fm = 0, first = 0, fn = -1;
    void drop() { epoch += 1; }
    void frame(long frames, bool reset) { if (reset) drop(); fn = frames; }
    bool refuses(long first_frames) const { return fn < 0 || fn + 1 - first_frames < 1; }
    bool usable = false, kept = false;
    void call(long first_frames, bool keep_flag)
    {
        usable = snap_epoch == epoch && fn > fm && first_frames == first;
        kept = usable && keep_flag;
        if (!kept) { fm = fn; first = first_frames; snap_epoch = epoch; }
    }
};

int main(int argc, char **argv)
{
    if (argc > 1 && !std::strcmp(argv[1], "replay")) return replay();
    // defaults: the numbers of host.py's ERROR_DEFAULTS and of the header's text
    const Params d = default_params();
    CHECK(d.threshold == 0.05f && d.floor == 0.01f && d.quantile_permille == 950u && d.first_frames == 1 && d.flags == 0u && !invalid(d));
    for (uint32_t r : d.reserved) CHECK(r == 0u);
    for (uint32_t q = 0; q < 1100; ++q) { Params p = d; p.quantile_permille = q; CHECK(!invalid(p) == (q >= 1 && q <= 1000)); }
    { Params p = d; p.first_frames = 0; CHECK(!invalid(p)); p.first_frames = -1; CHECK(invalid(p)); p = d; p.flags = 1; CHECK(!invalid(p)); p.flags = 2; CHECK(invalid(p)); }
    { Params p = d; p.threshold = 1e-45f; CHECK(!invalid(p)); p.threshold = 0.0f; CHECK(invalid(p)); p = d; p.floor = -0.0f; CHECK(invalid(p)); }
    // refusals: a state first, then the two invalid ones
    {
        Snapshot s;
        CHECK(refused(s, d, 32, 32).code == kState && refused(s, d, 65536, 65536).code == kState);
        rendered_frame(s, 2, false);
        Params p = d; p.first_frames = 2; CHECK(!refused(s, p, 32, 32).why); p.first_frames = 3; CHECK(refused(s, p, 32, 32).code == kInvalid);
        CHECK(!refused(s, d, 65535, 65535).why && !refused(s, d, 65536, 65535).why && refused(s, d, 65536, 65536).code == kInvalid);
        p.first_frames = 0x7FFFFFFF; CHECK(refused(s, p, 32, 32).why); rendered_frame(s, 0x7FFFFFFF, false); CHECK(!refused(s, p, 32, 32).why && !refused(s, d, 32, 32).why);
    }
    // a scripted history of frames, drops and estimates: the decisions of the mirror's Estimator
    {
        Snapshot s;
        Mirror m;
        uint32_t rng = 12345u;
        auto pick = [&](uint32_t n) { rng = rng * 1664525u + 1013904223u; return (rng >> 8) % n; };
        long frames = 0, estimates = 0, used = 0, kept = 0;
        for (int step = 0; step < 20000; ++step) {
            const uint32_t what = pick(10);
            if (what < 4) {                                                 // a frame, now and then a reset frame or a jump of the count
                const bool reset = pick(8) == 0;
                frames = pick(16) == 0 ? (long)pick(50) : frames + 1;
                rendered_frame(s, (int32_t)frames, reset); m.frame(frames, reset);
            } else if (what == 4) { drop(s); m.drop(); }
            else {
                Params p = d; p.first_frames = (int32_t)pick(3); p.flags = pick(2);
                const bool no = refused(s, p, 64, 48).why != nullptr;
                CHECK(no == m.refuses(p.first_frames));
                if (no) continue;
                const Plan q = plan(s, p);
                taken(s, p, q.keep);
                m.call(p.first_frames, p.flags != 0);
                CHECK(q.usable == m.usable && q.keep == m.kept && s.fm == m.fm && s.first == m.first && (s.snap_epoch == s.epoch) == (m.snap_epoch == m.epoch));
                CHECK(q.usable ? (q.frames_now == s.fn && q.frames_snapshot < q.frames_now && q.c > 0.0f) : (q.g_n == 0.0f && q.g_m == 0.0f && q.c == 0.0f && q.frames_now == 0));
                ++estimates; used += q.usable; kept += q.keep;
            }
        }
        CHECK(estimates > 5000 && used > 500 && kept > 100 && used - kept > 100);      // the script reaches every decision
    }
    // the factors, bit for bit: tests/error_mirror.py's scales() for (frames now, the snapshot's, first_frames)
    {
        const struct { int32_t fn, fm, first; float g_n, g_m, c; } cases[] = {
            {2, 1, 1, 0x1.8p+0f, 0x1p+1f, 0x1p+0f}, {3, 2, 1, 0x1.555556p+0f, 0x1.8p+0f, 0x1p+1f}, {17, 16, 1, 0x1.0f0f1p+0f, 0x1.1p+0f, 0x1p+4f},
            {100, 7, 3, 0x1.07d634p+0f, 0x1.99999ap+0f, 0x1.b86e1cp-5f}, {1000003, 999, 0, 0x1p+0f, 0x1p+0f, 0x1.0667c6p-10f}, {6, 5, 5, 0x1.cp+1f, 0x1.8p+2f, 0x1p+0f}};
        for (const auto &k : cases) {
            Snapshot s;
            Params p = d; p.first_frames = k.first;
            rendered_frame(s, k.fm, false); taken(s, p, false); rendered_frame(s, k.fn, false);
            const Plan q = plan(s, p);
            CHECK(q.usable && !q.keep && q.frames_now == k.fn && q.frames_snapshot == k.fm);
            CHECK(!std::memcmp(&q.g_n, &k.g_n, 4) && !std::memcmp(&q.g_m, &k.g_m, 4) && !std::memcmp(&q.c, &k.c, 4));
        }
    }
    // the footprint, the tiles and the sizes: rt_spread_plan keeps copies of its own
    for (int w : {-3, 0, 1, 7, 8, 15, 16, 17, 70, 1080, 1920, 65535, 65536, 0x7FFFFFFF})
        for (int h : {-3, 0, 1, 7, 8, 15, 16, 17, 53, 1080, 65535, 65536, 0x7FFFFFFF}) {
            CHECK(footprint_side(w) == rt_spread_plan::footprint_side(w) && tiles_along(w) == rt_spread_plan::tiles_along(w));
            CHECK(footprint(w, h) == rt_spread_plan::footprint(w, h) && footprint_fits(w, h) == rt_spread_plan::footprint_fits(w, h));
            CHECK(record_bytes(w, h) == rt_spread_plan::record_bytes(w, h));
        }
    CHECK(kTile == rt_spread_plan::kTile && kSummaryBytes == rt_spread_plan::kSummaryBytes && kRecordBytes == rt_spread_plan::kRecordBytes);
    CHECK(footprint(70, 53) == 64 * 48 && tiles_along(17) == 2 && record_bytes(1920, 1080) == 120u * 68u * 16u && snapshot_bytes(1920, 1080) == 2073600u * 4u);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("error_plan_check: ok\n");
    return 0;
}
