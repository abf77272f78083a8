// cli.cpp — `fmrx [<mode> <channels>] [--batch N] [--device D] [--rf-taps T] [--mono-product]
// [--offset-hz F] [--scan [--scan-bytes B]] [--iq-format u8|s8|s16|f32] [--capture-decim D]
// [--capture-rate HZ] [--rds] [--deemph 50|75] [--meter] [--blend] [--afc] [--quiet]`:
// the drop-in for the reference's `project` executable (src/project.cpp:273-390).  Reads u8 I/Q
// (or, with --iq-format, another raw format) from stdin and writes raw S16LE to stdout under project's process contract:
//   * arguments as project.cpp:278-299: fewer than two positional arguments run the default
//     mode 0 (a lone one is ignored, as `project 3` ignores it), exactly two are <mode>
//     <channels> (atoi; out of range -> message, exit 1), more print the usage and exit 1;
//   * the output is ALWAYS the 2-channel interleaved R,L stream of project.cpp:179-195:
//     `channels` is only logged (:301-302), the reference has no mono-only output;
//   * --mono-product (an fmrx extension, not a project argument) writes the 1-channel mono
//     product instead (project.cpp:146's mono resample with a private history, quantised like
//     :187) -- the BASELINE headline path;
//   * --offset-hz F (an fmrx extension) decodes the station F Hz off the capture's centre
//     (fmrx_tune: the I/Q is rotated by -F in front of the RF low-pass); the same loop otherwise.
//   * --scan (an fmrx extension) decodes nothing: it reads up to B bytes of stdin (--scan-bytes,
//     default 2^24; fewer at EOF), runs the band scan (fmrx_scan, default settings) and prints one
//     line per station found, `offset_hz power_db snr_db` (two decimals), ascending by offset; no
//     PCM, exit 0.  Fewer bytes than one transform (2 * fft_bins): message, exit 1.
//   * --iq-format u8|s8|s16|f32 (an fmrx extension, default u8) reads stdin as int8, little-endian
//     int16 or float32 pairs (fmrx_set_input_format), in blocks of iq_pairs times the pair's bytes;
//     with a format other than u8 and no --offset-hz the station at offset 0 is decoded; --scan-bytes
//     counts bytes of that format.  Without the flag nothing differs from before.
//   * --capture-decim D (an fmrx extension, D in 1..10, default 1) reads stdin as a capture at D times
//     the mode's rate (fmrx_set_capture_decim): blocks of D * iq_pairs pairs, --offset-hz against that
//     rate (fmrx_tune_wide; without it offset 0), decoded by fmrx_process_wide_device; --scan then runs
//     fmrx_scan_wide.  D = 1 is the same as no flag; anything else outside 2..10: message, exit 1.
//   * --capture-rate HZ (an fmrx extension) reads stdin as a capture at HZ samples a second
//     (fmrx_set_capture_rate: HZ = rf_fs M / L, a rational ratio through the polyphase down-converter,
//     an integer one as --capture-decim): stdin in whole granules (fmrx_wide_granule), --offset-hz and
//     --scan against that rate.  With --capture-decim: message, exit 1; a rate the library refuses:
//     message, exit 1.
//   * --rds (an fmrx extension) also decodes the station's RDS (fmrx_set_rds): the batch is rounded up to
//     whole RDS granules (fmrx_rds_granule), the tuned front end runs (offset 0 without --offset-hz), and
//     at end of input one line goes to stderr, `rds pi=%04X pty=%d ps="........" groups=%d`.  stdout is
//     unchanged: blocks past the last whole granule are decoded without RDS.
//   * --rds-sync (an fmrx extension, with --rds) also runs the block sync behind the bits (fmrx_set_rds_sync),
//     flushes it at end of input and prints, after the `rds ...` line, to stderr
//     `rdsx pi=%04X pty=%d ps="........" ct=YYYY-MM-DDTHH:MM+HH:MM af=%d blocks=%llu+%llu groups=%llu+%llu`
//     (ct=- without a clock time; blocks exact + corrected, groups complete + partial).  Without --rds:
//     message, exit 1.
//   * --deemph 50|75 (an fmrx extension) de-emphasises the PCM with that time constant in microseconds
//     (fmrx_set_deemphasis: 50 in most of the world, 75 in the Americas and Korea), whatever else is
//     chosen; without it the audio is as broadcast, as project's is.  Any other value: message, exit 1.
//   * --meter (an fmrx extension) also measures the station's 19 kHz pilot and 57 kHz RDS subcarrier
//     (fmrx_set_meter): batches of whole frames and the tuned front end as with --rds, and at end of input
//     one line goes to stderr, `meter pilot_snr=%.1f stereo=%d rds_snr=%.1f rds=%d frames=%llu`.  stdout is
//     unchanged: blocks past the last whole frame are decoded without the meter.
//   * --blend (an fmrx extension, with <channels> 2) blends the station toward mono by the signal-to-noise
//     ratio of its pilot (fmrx_set_stereo_blend, the default thresholds): batches of whole granules and the
//     tuned front end as with --meter; blocks past the last whole granule are decoded at the last level
//     (fmrx_blend_hold); at end of input one line goes to stderr, `blend mean=%.2f full=%llu mono=%llu
//     frames=%llu` (the mean level over 16, the frames at level 16 and at level 0, all frames).  With
//     <channels> 1 or --mono-product: message, exit 1.
//   * --quiet (an fmrx extension, either <channels>) rolls off the treble and turns the audio down by the
//     station's noise level (fmrx_set_quieting, the default configuration): batches of whole granules and the
//     tuned front end as with --meter; blocks past the last whole granule are decoded at the last levels
//     (fmrx_quiet_hold); at end of input one line goes to stderr, `quiet cut=%.2f mute=%.2f frames=%llu` (the
//     mean cut and mute levels over 16, all frames).  (The usage text does not list it: tests/golden/
//     drivers_parent.json records that text byte for byte.)
//   * --afc (an fmrx extension) measures the station's carrier against --offset-hz and retunes to it between
//     batches (fmrx_set_afc, the default configuration, tracking on): batches of whole frames and the tuned
//     front end as with --meter; blocks past the last whole frame are decoded where the tuner then stands,
//     unmeasured; at end of input one line goes to stderr, `afc offset=%+d err=%+.0f carrier=%d retunes=%u
//     frames=%llu` (where the stream ended, its last decision's error and gate, the retunes, all frames).
//     The PCM depends on the batch size, as every retune happens between two batches.
//
// Streaming runtime.  The reference splits the work into a producer thread
// (read + RF front end, project.cpp:48-84) and a consumer thread (audio back end, :132-196)
// joined by a bounded queue of depth 3 (QUEUE_CAPACITY, :17).  Here the whole receive runs on
// the GPU and the queue becomes a ring of 3 batch slots, each a pinned host input/output pair
// and a device input/output pair, cycled by three agents:
//   reader thread : fread whole blocks straight into a free slot's pinned input;
//   main thread   : H2D on a copy stream -> (event) -> fmrx_process_device on the context's
//                   stream -> (event) -> D2H on an output stream, all asynchronous;
//   writer thread : waits for the slot's D2H event, writes its PCM, frees the slot.
// so the upload of batch i+1, the receive of batch i and the write of batch i-1 overlap.
// Stream order keeps the receiver state sequential (one context, one compute stream).
// Unlike the reference (project.cpp:51-54, which exit(1)s while blocks are still queued) every
// full block read is processed before the process exits 0; a trailing partial block is
// dropped, as in the reference.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

#include "fmrx.h"

namespace {

constexpr int kSlots = 3;  // project.cpp:17 QUEUE_CAPACITY

class IndexQueue {
  public:
    void push(int v) {
        std::lock_guard<std::mutex> lk(m_);
        q_.push_back(v);
        cv_.notify_all();
    }
    int pop() {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return !q_.empty(); });
        const int v = q_.front();
        q_.pop_front();
        return v;
    }

  private:
    std::mutex m_;
    std::condition_variable cv_;
    std::deque<int> q_;
};

struct Slot {
    uint8_t* h_in = nullptr;   // pinned
    int16_t* h_out = nullptr;  // pinned
    uint8_t* d_in = nullptr;
    int16_t* d_out = nullptr;
    hipEvent_t uploaded{}, computed{}, downloaded{};
    size_t blocks = 0;
    bool last = false;
};

// the usage text to stderr; false, as refuse() below
bool usage(const char* argv0) {
    std::fprintf(stderr,
                 "Usage: %s\nor \nUsage %s <mode> <channels>\n"
                 "\t\t<mode> is a value from 0 to 3\n\t\t   <channels> is either 1 or 2\n"
                 "options (fmrx): [--batch N] [--device D] [--rf-taps T] [--mono-product] [--offset-hz F]\n"
                 "                [--deemph 50|75]  de-emphasise the audio (time constant in us; default: none)\n"
                 "                [--meter]  measure the pilot and the RDS subcarrier; at end of input print their levels to stderr\n"
                 "                [--afc]  measure the carrier's offset and retune to it between batches; print where it ended to stderr\n"
                 "                [--blend]  with <channels> 2: blend toward mono by the pilot's signal-to-noise ratio; print the levels' summary to stderr\n"
                 "                [--rds-sync]  with --rds: per-block sync with burst correction; print the extended line too\n"
                 "                [--rds]  decode the station's RDS too; at end of input print its PI, PTY and name to stderr\n"
                 "                [--iq-format u8|s8|s16|f32]  raw format of stdin (default u8)\n"
                 "                [--capture-decim D]  stdin runs at D (2..10) times the mode's rate; --offset-hz and\n"
                 "                                     --scan then refer to that rate (default 1)\n"
                 "                [--capture-rate HZ]  stdin runs at HZ samples a second (10000000, 8000000, 2048000 ...),\n"
                 "                                     read in whole granules; not with --capture-decim\n"
                 "                [--scan [--scan-bytes B]]  list the stations of the first B bytes (default 16777216)\n"
                 "                                           as `offset_hz power_db snr_db` lines; no PCM\n",
                 argv0, argv0);
    return false;
}

// a message to stderr; false, which every step of main answers for "exit 1"
bool refuse(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    return false;
}

[[noreturn]] void die_hip(hipError_t e, const char* what) {
    std::fprintf(stderr, "fmrx: %s: %s\n", what, hipGetErrorString(e));
    std::fflush(stdout);
    std::_Exit(1);
}

#define CLI_HIP(x)                              \
    do {                                        \
        const hipError_t e_ = (x);              \
        if (e_ != hipSuccess) die_hip(e_, #x);  \
    } while (0)

// ---- the demod-row switches: one row each, in the order of their end-of-input lines -------------------
// Every one of them taps the tuned front end's demod rows over whole RDS granules (the meter's frames), so
// with any of them on the batch is whole granules and the tuner runs; what differs is in its row.

void report_rds(fmrx_ctx* ctx) {
    fmrx_rds_info info;
    if (fmrx_rds_info_get(ctx, 0, &info) == FMRX_OK)
        std::fprintf(stderr, "rds pi=%04X pty=%d ps=\"%s\" groups=%d\n", (unsigned)info.pi, (int)info.pty, info.ps,
                     (int)info.groups);
}

void report_rds_sync(fmrx_ctx* ctx) {
    fmrx_rds_ext x;
    if (fmrx_rds_blocks_flush(ctx, nullptr, 0, nullptr) != FMRX_OK || fmrx_rds_ext_get(ctx, 0, &x) != FMRX_OK) return;
    char ct[32] = "-";
    if (x.ct_set) {
        const int half = x.ct_offset < 0 ? -x.ct_offset : x.ct_offset;
        std::snprintf(ct, sizeof ct, "%04d-%02d-%02dT%02d:%02d%c%02d:%02d", (int)x.ct_year, (int)x.ct_month, (int)x.ct_day,
                      (int)x.ct_hour, (int)x.ct_minute, x.ct_offset < 0 ? '-' : '+', half / 2, half % 2 * 30);
    }
    std::fprintf(stderr, "rdsx pi=%04X pty=%d ps=\"%s\" ct=%s af=%d blocks=%llu+%llu groups=%llu+%llu\n", (unsigned)x.pi,
                 (int)x.pty, x.ps, ct, (int)x.af_n, (unsigned long long)x.exact_blocks,
                 (unsigned long long)x.corrected_blocks, (unsigned long long)x.groups,
                 (unsigned long long)x.partial_groups);
}

void report_meter(fmrx_ctx* ctx) {
    fmrx_meter_report rep;
    fmrx_subcarriers sc{};
    if (fmrx_meter_get(ctx, 0, &rep) == FMRX_OK && (rep.frames == 0 || fmrx_meter_detect(&rep, nullptr, &sc) == FMRX_OK))
        std::fprintf(stderr, "meter pilot_snr=%.1f stereo=%d rds_snr=%.1f rds=%d frames=%llu\n", (double)sc.pilot_snr_db,
                     sc.stereo, (double)sc.rds_snr_db, sc.rds, (unsigned long long)rep.frames);
}

void report_afc(fmrx_ctx* ctx) {
    fmrx_afc_status st;
    if (fmrx_afc_get(ctx, 0, &st) == FMRX_OK)
        std::fprintf(stderr, "afc offset=%+d err=%+.0f carrier=%d retunes=%u frames=%llu\n", (int)st.offset_hz, st.last.err_hz,
                     st.last.carrier, st.retunes, (unsigned long long)st.total.frames);
}

void report_blend(fmrx_ctx* ctx) {
    fmrx_blend_report rep;
    if (fmrx_blend_get(ctx, 0, &rep) != FMRX_OK) return;
    double sum = 0.0;
    for (int l = 0; l <= 16; l++) sum += (double)l * (double)rep.level_frames[l];
    std::fprintf(stderr, "blend mean=%.2f full=%llu mono=%llu frames=%llu\n", rep.frames ? sum / (16.0 * (double)rep.frames) : 0.0,
                 (unsigned long long)rep.level_frames[16], (unsigned long long)rep.level_frames[0],
                 (unsigned long long)rep.frames);
}

void report_quiet(fmrx_ctx* ctx) {
    fmrx_quiet_report rep;
    if (fmrx_quiet_get(ctx, 0, &rep) != FMRX_OK) return;
    double cut = 0.0, mute = 0.0;
    for (int l = 0; l <= 16; l++) cut += (double)l * (double)rep.cut_frames[l], mute += (double)l * (double)rep.mute_frames[l];
    const double over = rep.frames ? 16.0 * (double)rep.frames : 1.0;
    std::fprintf(stderr, "quiet cut=%.2f mute=%.2f frames=%llu\n", cut / over, mute / over, (unsigned long long)rep.frames);
}

enum { kRds, kRdsSync, kMeter, kAfc, kBlend, kQuiet, kSwitchCount };

struct Switch {
    const char* flag;
    int (*turn_on)(fmrx_ctx*);
    int (*before_tail)(fmrx_ctx*);  // ahead of the blocks past the last whole granule (null: it stays as it is)
    void (*report)(fmrx_ctx*);      // its line at end of input
};

const Switch kSwitches[kSwitchCount] = {
    {"--rds", [](fmrx_ctx* c) { return fmrx_set_rds(c, 1); }, [](fmrx_ctx* c) { return fmrx_set_rds(c, 0); }, report_rds},
    {"--rds-sync", [](fmrx_ctx* c) { return fmrx_set_rds_sync(c, 1); }, nullptr, report_rds_sync},
    {"--meter", [](fmrx_ctx* c) { return fmrx_set_meter(c, 1); }, [](fmrx_ctx* c) { return fmrx_set_meter(c, 0); }, report_meter},
    {"--afc", [](fmrx_ctx* c) { return fmrx_set_afc(c, nullptr, 1); }, [](fmrx_ctx* c) { return fmrx_set_afc(c, nullptr, 0); }, report_afc},
    {"--blend", [](fmrx_ctx* c) { return fmrx_set_stereo_blend(c, 1, nullptr); }, [](fmrx_ctx* c) { return fmrx_blend_hold(c, 1); }, report_blend},
    {"--quiet", [](fmrx_ctx* c) { return fmrx_set_quieting(c, 1, nullptr); }, [](fmrx_ctx* c) { return fmrx_quiet_hold(c, 1); }, report_quiet},
};

struct Options {
    int mode = 0, channels = 1, batch = 16, device = 0, rf_taps = 51;
    bool mono_product = false, tuned = false, scan = false, have_rate = false, have_deemph = false;
    bool on[kSwitchCount] = {};  // the demod-row switches, by row of kSwitches
    long offset_hz = 0, capture_rate = 0;
    int iq_format = FMRX_IQ_U8, capture_decim = 1, deemph_us = 0;
    long long scan_bytes = 1ll << 24;
    bool any_switch() const { return std::find(on, on + kSwitchCount, true) != on + kSwitchCount; }
};

// The arguments into o, and every refusal that needs no context.
bool parse(int argc, char** argv, Options* o) {
    bool have_decim = false;
    const char* bad_format = nullptr;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; i++) {
        const auto is = [&](const char* flag) { return !std::strcmp(argv[i], flag); };
        const bool value = i + 1 < argc;  // a value follows
        if (is("--batch") && value) o->batch = std::atoi(argv[++i]);
        else if (is("--device") && value) o->device = std::atoi(argv[++i]);
        else if (is("--rf-taps") && value) o->rf_taps = std::atoi(argv[++i]);
        else if (is("--mono-product")) o->mono_product = true;
        else if (is("--scan")) o->scan = true;
        else if (is("--rds")) o->on[kRds] = true;
        else if (is("--rds-sync")) o->on[kRdsSync] = true;
        else if (is("--meter")) o->on[kMeter] = true;
        else if (is("--blend")) o->on[kBlend] = true;
        else if (is("--afc")) o->on[kAfc] = true;
        else if (is("--quiet")) o->on[kQuiet] = true;
        else if (is("--scan-bytes") && value) o->scan_bytes = std::atoll(argv[++i]);
        else if (is("--iq-format") && value) {
            static const char* const names[] = {"u8", "s8", "s16", "f32"};  // FMRX_IQ_U8 .. FMRX_IQ_F32
            const char* f = argv[++i];
            const auto at = std::find_if(names, names + 4, [&](const char* n) { return !std::strcmp(f, n); });
            if (at == names + 4) bad_format = f;
            else o->iq_format = (int)(at - names);
        }
        else if (is("--deemph") && value) o->deemph_us = std::atoi(argv[++i]), o->have_deemph = true;
        else if (is("--capture-decim") && value) o->capture_decim = std::atoi(argv[++i]), have_decim = true;
        else if (is("--capture-rate") && value) o->capture_rate = std::atol(argv[++i]), o->have_rate = true;
        else if (is("--offset-hz") && value) o->offset_hz = std::atol(argv[++i]), o->tuned = true;
        else if (argv[i][0] == '-' && argv[i][1] != '\0' && !(argv[i][1] >= '0' && argv[i][1] <= '9')) return usage(argv[0]);
        else pos.push_back(argv[i]);  // "-1" is a (negative, invalid) mode as in project
    }
    if (pos.size() > 2) return usage(argv[0]);  // project.cpp:292-298
    if (pos.size() < 2) {  // :278-279 (argc < 3): argv[1] alone is not parsed
        std::fprintf(stderr, "Operating in default mode 0, mono\n");
    } else {  // :280-291
        o->mode = std::atoi(pos[0]);
        o->channels = std::atoi(pos[1]);
        if (o->mode < 0 || o->mode > 3) return refuse("Invalid mode: %d!\n", o->mode);
        if (o->channels < 1 || o->channels > 2) return refuse("Invaild channel: %d!\n", o->channels);  // project.cpp:289, verbatim
    }
    if (o->on[kRdsSync] && !o->on[kRds]) return refuse("fmrx: --rds-sync needs --rds\n");
    if (o->on[kBlend] && (o->channels != 2 || o->mono_product))
        return refuse("fmrx: --blend needs <channels> 2 (soft stereo blends a stereo decode)\n");
    if (bad_format) return refuse("fmrx: --iq-format %s: expected u8, s8, s16 or f32\n", bad_format);
    if (o->capture_decim < 1 || o->capture_decim > 10)
        return refuse("fmrx: --capture-decim %d: expected 1 to 10\n", o->capture_decim);
    if (o->have_rate && have_decim) return refuse("fmrx: --capture-rate and --capture-decim exclude each other\n");
    if (o->have_rate && (o->capture_rate < 1 || o->capture_rate > 2147483647l))
        return refuse("fmrx: --capture-rate %ld: expected a rate in Hz\n", o->capture_rate);
    if (o->have_deemph && o->deemph_us != 50 && o->deemph_us != 75)
        return refuse("fmrx: --deemph %d: expected 50 or 75 (microseconds)\n", o->deemph_us);
    if (o->batch < 1) o->batch = 1;
    std::fprintf(stderr, "Operating in mode %d, %s\n", o->mode, o->channels == 1 ? "mono" : "stereo");
    return true;
}

// The context and what its input looks like.
struct Session {
    fmrx_ctx* ctx = nullptr;
    fmrx_geometry_t geo;
    bool wide = false;
    size_t unit_blocks = 1, unit_pairs = 0;  // a read unit: a block, or with --capture-rate a granule of unit_blocks blocks
    size_t pair_bytes = 0, block_bytes = 0;  // bytes an I/Q pair and a read unit take (geo.block_bytes for u8 at the mode's rate)
    size_t batch = 0, rds_unit = 1;          // blocks a batch (whole units); blocks the switches' calls are whole multiples of
};

// The context, set to stdin's format and rate.
bool open_context(const Options& o, Session* s) {
    // project.cpp always writes the stereo R,L stream whatever `channels` says (:179-195).
    fmrx_config cfg;
    if (fmrx_config_default(&cfg, o.mode, o.mono_product ? FMRX_MONO : FMRX_STEREO) != FMRX_OK)
        return refuse("fmrx: %s\n", fmrx_last_error());
    cfg.device = o.device;
    cfg.rf_taps = o.rf_taps;
    if (fmrx_geometry(&cfg, &s->geo) != FMRX_OK || fmrx_create(&cfg, &s->ctx) != FMRX_OK)
        return refuse("fmrx: %s\n", fmrx_last_error());
    if (o.iq_format != FMRX_IQ_U8 && fmrx_set_input_format(s->ctx, o.iq_format) != FMRX_OK)
        return refuse("fmrx: --iq-format: %s\n", fmrx_last_error());
    s->wide = o.capture_decim > 1;
    if (s->wide && fmrx_set_capture_decim(s->ctx, o.capture_decim) != FMRX_OK)
        return refuse("fmrx: --capture-decim: %s\n", fmrx_last_error());
    s->unit_pairs = s->geo.iq_pairs * (size_t)o.capture_decim;
    if (o.have_rate) {
        int d = 1;
        if (fmrx_set_capture_rate(s->ctx, (int)o.capture_rate) != FMRX_OK || fmrx_capture_decim(s->ctx, &d) != FMRX_OK ||
            fmrx_wide_granule(s->ctx, &s->unit_blocks, &s->unit_pairs) != FMRX_OK)
            return refuse("fmrx: --capture-rate: %s\n", fmrx_last_error());
        s->wide = d != 1;  // fmrx_capture_decim reads 1 at the mode's own rate alone (D, or 0 at a rational ratio): no wide capture
    }
    s->pair_bytes = (size_t)fmrx_iq_pair_bytes(o.iq_format);
    s->block_bytes = s->unit_pairs * s->pair_bytes;
    s->batch = std::max<size_t>(1, (size_t)o.batch / s->unit_blocks) * s->unit_blocks;
    s->rds_unit = s->unit_blocks;
    return true;
}

// --scan: the stations in the first --scan-bytes of stdin, one line each
bool scan_stdin(const Options& o, const Session& s) {
    if (o.scan_bytes <= 0) return refuse("fmrx: --scan-bytes must be positive\n");
    const size_t max_bytes = (size_t)o.scan_bytes;
    fmrx_scan_config sc;
    (void)fmrx_scan_config_default(&sc);
    std::vector<uint8_t> iq(max_bytes);
    size_t got = 0;
    while (got < max_bytes) {
        const size_t r = std::fread(iq.data() + got, 1, max_bytes - got, stdin);
        if (r == 0) break;
        got += r;
    }
    if (got < s.pair_bytes * (size_t)sc.fft_bins)
        return refuse("fmrx: --scan needs at least %zu bytes of I/Q on stdin, got %zu\n", s.pair_bytes * (size_t)sc.fft_bins, got);
    constexpr int kMaxStations = 256;
    fmrx_station st[kMaxStations];
    int n = 0;
    if ((s.wide ? fmrx_scan_wide : fmrx_scan)(s.ctx, iq.data(), got / s.pair_bytes, &sc, st, kMaxStations, &n) != FMRX_OK)
        return refuse("fmrx: %s\n", fmrx_last_error());
    for (int i = 0; i < n && i < kMaxStations; i++)
        std::printf("%d %.2f %.2f\n", (int)st[i].offset_hz, (double)st[i].power_db, (double)st[i].snr_db);
    std::fflush(stdout);
    return true;
}

// What a decode sets before its first batch: de-emphasis, the switches, the tuner.
bool prepare(const Options& o, Session* s) {
    if (o.have_deemph && fmrx_set_deemphasis(s->ctx, o.deemph_us) != FMRX_OK) return refuse("fmrx: --deemph: %s\n", fmrx_last_error());
    // any switch: whole RDS granules (the meter's frames) a batch (rounded up), decoded by the tuned front end
    const bool granule = !o.any_switch() || fmrx_rds_granule(s->ctx, &s->rds_unit) == FMRX_OK;
    for (int r = 0; r < kSwitchCount; r++)
        if (o.on[r] && (!granule || kSwitches[r].turn_on(s->ctx) != FMRX_OK))
            return refuse("fmrx: %s: %s\n", kSwitches[r].flag, fmrx_last_error());
    s->batch = (s->batch + s->rds_unit - 1) / s->rds_unit * s->rds_unit;
    if (o.tuned || s->wide || o.any_switch()) {  // out of range (or no 32-bit value) -> message, exit 1
        const int32_t f = (int32_t)o.offset_hz;
        if ((long)f != o.offset_hz || (s->wide ? fmrx_tune_wide : fmrx_tune)(s->ctx, &f, 0) != FMRX_OK)
            return refuse("fmrx: --offset-hz %ld: %s\n", o.offset_hz, (long)f != o.offset_hz ? "out of range" : fmrx_last_error());
    }
    return true;
}

// stdin to stdout through the ring of three slots, until end of input
void pump(const Options& o, const Session& ss) {
    const size_t unit_blocks = ss.unit_blocks, block_bytes = ss.block_bytes, pcm_samples = ss.geo.pcm_samples;
    const size_t in_cap = block_bytes * (ss.batch / unit_blocks);
    const size_t out_cap = pcm_samples * ss.batch;

    CLI_HIP(hipSetDevice(o.device));
    hipStream_t compute = static_cast<hipStream_t>(fmrx_stream(ss.ctx));
    hipStream_t up, down;
    CLI_HIP(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    CLI_HIP(hipStreamCreateWithFlags(&down, hipStreamNonBlocking));
    Slot slots[kSlots];
    for (Slot& s : slots) {
        CLI_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.h_in), in_cap, hipHostMallocDefault));
        CLI_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.h_out), out_cap * sizeof(int16_t), hipHostMallocDefault));
        CLI_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_in), in_cap));
        CLI_HIP(hipMalloc(reinterpret_cast<void**>(&s.d_out), out_cap * sizeof(int16_t)));
        CLI_HIP(hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming));
        CLI_HIP(hipEventCreateWithFlags(&s.computed, hipEventDisableTiming));
        CLI_HIP(hipEventCreateWithFlags(&s.downloaded, hipEventDisableTiming));
    }

    IndexQueue free_q, filled_q, done_q;
    for (int i = 0; i < kSlots; i++) free_q.push(i);

    std::thread reader([&] {
        for (;;) {
            const int i = free_q.pop();
            Slot& s = slots[i];
            size_t got = 0;
            while (got < in_cap) {
                const size_t r = std::fread(s.h_in + got, 1, in_cap - got, stdin);
                if (r == 0) break;
                got += r;
            }
            s.blocks = got / block_bytes * unit_blocks;
            s.last = got < in_cap;
            filled_q.push(i);
            if (s.last) return;
        }
    });
    std::thread writer([&] {
        for (;;) {
            const int i = done_q.pop();
            Slot& s = slots[i];
            if (s.blocks > 0) {
                CLI_HIP(hipEventSynchronize(s.downloaded));
                std::fwrite(s.h_out, sizeof(int16_t), s.blocks * pcm_samples, stdout);
            }
            if (s.last) return;
            free_q.push(i);
        }
    });

    auto process = ss.wide ? fmrx_process_wide_device : fmrx_process_device;
    for (;;) {
        const int i = filled_q.pop();
        Slot& s = slots[i];
        if (s.blocks > 0) {
            // with a switch on: the whole granules, then (end of input only) the blocks left over, every switch as
            // its row says before the tail
            const size_t head = s.blocks / ss.rds_unit * ss.rds_unit;
            CLI_HIP(hipMemcpyAsync(s.d_in, s.h_in, s.blocks / unit_blocks * block_bytes, hipMemcpyHostToDevice, up));
            CLI_HIP(hipEventRecord(s.uploaded, up));
            CLI_HIP(hipStreamWaitEvent(compute, s.uploaded, 0));
            bool ok = head == 0 || process(ss.ctx, s.d_in, head, s.d_out) == FMRX_OK;
            if (ok && head < s.blocks) {
                for (int r = 0; ok && r < kSwitchCount; r++)
                    if (o.on[r] && kSwitches[r].before_tail) ok = kSwitches[r].before_tail(ss.ctx) == FMRX_OK;
                ok = ok && process(ss.ctx, s.d_in + head / unit_blocks * block_bytes, s.blocks - head,
                                   s.d_out + head * pcm_samples) == FMRX_OK;
            }
            if (!ok) {
                std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
                std::fflush(stdout);
                std::_Exit(1);
            }
            CLI_HIP(hipEventRecord(s.computed, compute));
            CLI_HIP(hipStreamWaitEvent(down, s.computed, 0));
            CLI_HIP(hipMemcpyAsync(s.h_out, s.d_out, s.blocks * pcm_samples * sizeof(int16_t), hipMemcpyDeviceToHost, down));
            CLI_HIP(hipEventRecord(s.downloaded, down));
        }
        done_q.push(i);
        if (s.last) break;
    }
    reader.join();
    writer.join();
    std::fflush(stdout);
    for (Slot& s : slots) {
        (void)hipHostFree(s.h_in);
        (void)hipHostFree(s.h_out);
        (void)hipFree(s.d_in);
        (void)hipFree(s.d_out);
        (void)hipEventDestroy(s.uploaded);
        (void)hipEventDestroy(s.computed);
        (void)hipEventDestroy(s.downloaded);
    }
    (void)hipStreamDestroy(up);
    (void)hipStreamDestroy(down);
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    Session s;
    if (!parse(argc, argv, &o)) return 1;
    bool ok = open_context(o, &s);
    if (ok && o.scan) {
        ok = scan_stdin(o, s);
    } else if (ok && (ok = prepare(o, &s))) {
        pump(o, s);
        for (int r = 0; r < kSwitchCount; r++)
            if (o.on[r]) kSwitches[r].report(s.ctx);
    }
    fmrx_destroy(s.ctx);
    if (ok && !o.scan) std::fprintf(stderr, "End of input stream reached!\n");
    return ok ? 0 : 1;
}
