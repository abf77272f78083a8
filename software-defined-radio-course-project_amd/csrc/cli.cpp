// cli.cpp — `fmrx [<mode> <channels>] [--batch N] [--device D] [--rf-taps T] [--mono-product]
// [--offset-hz F] [--scan [--scan-bytes B]] [--iq-format u8|s8|s16|f32] [--capture-decim D]
// [--capture-rate HZ] [--rds] [--deemph 50|75] [--meter] [--blend] [--afc]`:
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

void usage(const char* argv0) {
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
}

[[noreturn]] void die_hip(hipError_t e, const char* what) {
    std::fprintf(stderr, "fmrx: %s: %s\n", what, hipGetErrorString(e));
    std::fflush(stdout);
    std::_Exit(1);
}

// --scan: the stations in the first max_bytes of stdin, one line each
int scan_stdin(fmrx_ctx* ctx, size_t max_bytes, size_t pair_bytes, bool wide) {
    fmrx_scan_config sc;
    (void)fmrx_scan_config_default(&sc);
    std::vector<uint8_t> iq(max_bytes);
    size_t got = 0;
    while (got < max_bytes) {
        const size_t r = std::fread(iq.data() + got, 1, max_bytes - got, stdin);
        if (r == 0) break;
        got += r;
    }
    if (got < pair_bytes * (size_t)sc.fft_bins) {
        std::fprintf(stderr, "fmrx: --scan needs at least %zu bytes of I/Q on stdin, got %zu\n",
                     pair_bytes * (size_t)sc.fft_bins, got);
        return 1;
    }
    constexpr int kMaxStations = 256;
    fmrx_station st[kMaxStations];
    int n = 0;
    if ((wide ? fmrx_scan_wide : fmrx_scan)(ctx, iq.data(), got / pair_bytes, &sc, st, kMaxStations, &n) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
        return 1;
    }
    for (int i = 0; i < n && i < kMaxStations; i++)
        std::printf("%d %.2f %.2f\n", (int)st[i].offset_hz, (double)st[i].power_db, (double)st[i].snr_db);
    std::fflush(stdout);
    return 0;
}

#define CLI_HIP(x)                              \
    do {                                        \
        const hipError_t e_ = (x);              \
        if (e_ != hipSuccess) die_hip(e_, #x);  \
    } while (0)

}  // namespace

int main(int argc, char** argv) {
    int mode = 0, channels = 1, batch = 16, device = 0, rf_taps = 51;
    bool mono_product = false, tuned = false, scan = false, rds = false, rds_sync = false, meter = false, blend = false, afc = false;
    long offset_hz = 0;
    int iq_format = FMRX_IQ_U8, capture_decim = 1, deemph_us = 0;
    long capture_rate = 0;
    bool have_decim = false, have_rate = false, have_deemph = false;
    const char* bad_format = nullptr;
    long long scan_bytes = 1ll << 24;
    std::vector<const char*> pos;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--batch") && i + 1 < argc) batch = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--device") && i + 1 < argc) device = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--rf-taps") && i + 1 < argc) rf_taps = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--mono-product")) mono_product = true;
        else if (!std::strcmp(argv[i], "--scan")) scan = true;
        else if (!std::strcmp(argv[i], "--rds")) rds = true;
        else if (!std::strcmp(argv[i], "--rds-sync")) rds_sync = true;
        else if (!std::strcmp(argv[i], "--meter")) meter = true;
        else if (!std::strcmp(argv[i], "--blend")) blend = true;
        else if (!std::strcmp(argv[i], "--afc")) afc = true;
        else if (!std::strcmp(argv[i], "--scan-bytes") && i + 1 < argc) scan_bytes = std::atoll(argv[++i]);
        else if (!std::strcmp(argv[i], "--iq-format") && i + 1 < argc) {
            const char* f = argv[++i];
            if (!std::strcmp(f, "u8")) iq_format = FMRX_IQ_U8;
            else if (!std::strcmp(f, "s8")) iq_format = FMRX_IQ_S8;
            else if (!std::strcmp(f, "s16")) iq_format = FMRX_IQ_S16;
            else if (!std::strcmp(f, "f32")) iq_format = FMRX_IQ_F32;
            else bad_format = f;
        }
        else if (!std::strcmp(argv[i], "--deemph") && i + 1 < argc) {
            deemph_us = std::atoi(argv[++i]);
            have_deemph = true;
        }
        else if (!std::strcmp(argv[i], "--capture-decim") && i + 1 < argc) {
            capture_decim = std::atoi(argv[++i]);
            have_decim = true;
        }
        else if (!std::strcmp(argv[i], "--capture-rate") && i + 1 < argc) {
            capture_rate = std::atol(argv[++i]);
            have_rate = true;
        }
        else if (!std::strcmp(argv[i], "--offset-hz") && i + 1 < argc) {
            offset_hz = std::atol(argv[++i]);
            tuned = true;
        }
        else if (argv[i][0] == '-' && argv[i][1] != '\0' && !(argv[i][1] >= '0' && argv[i][1] <= '9')) {
            usage(argv[0]);
            return 1;
        } else pos.push_back(argv[i]);  // "-1" is a (negative, invalid) mode as in project
    }
    if (pos.size() < 2) {  // project.cpp:278-279 (argc < 3): argv[1] alone is not parsed
        std::fprintf(stderr, "Operating in default mode 0, mono\n");
    } else if (pos.size() == 2) {  // :280-291
        mode = std::atoi(pos[0]);
        channels = std::atoi(pos[1]);
        if (mode < 0 || mode > 3) { std::fprintf(stderr, "Invalid mode: %d!\n", mode); return 1; }
        if (channels < 1 || channels > 2) { std::fprintf(stderr, "Invaild channel: %d!\n", channels); return 1; }  // project.cpp:289, verbatim
    } else {  // :292-298
        usage(argv[0]);
        return 1;
    }
    if (rds_sync && !rds) {
        std::fprintf(stderr, "fmrx: --rds-sync needs --rds\n");
        return 1;
    }
    if (blend && (channels != 2 || mono_product)) {
        std::fprintf(stderr, "fmrx: --blend needs <channels> 2 (soft stereo blends a stereo decode)\n");
        return 1;
    }
    if (bad_format) {
        std::fprintf(stderr, "fmrx: --iq-format %s: expected u8, s8, s16 or f32\n", bad_format);
        return 1;
    }
    if (capture_decim < 1 || capture_decim > 10) {
        std::fprintf(stderr, "fmrx: --capture-decim %d: expected 1 to 10\n", capture_decim);
        return 1;
    }
    if (have_rate && have_decim) {
        std::fprintf(stderr, "fmrx: --capture-rate and --capture-decim exclude each other\n");
        return 1;
    }
    if (have_rate && (capture_rate < 1 || capture_rate > 2147483647l)) {
        std::fprintf(stderr, "fmrx: --capture-rate %ld: expected a rate in Hz\n", capture_rate);
        return 1;
    }
    if (have_deemph && deemph_us != 50 && deemph_us != 75) {
        std::fprintf(stderr, "fmrx: --deemph %d: expected 50 or 75 (microseconds)\n", deemph_us);
        return 1;
    }
    bool wide = capture_decim > 1;
    if (batch < 1) batch = 1;
    std::fprintf(stderr, "Operating in mode %d, %s\n", mode, channels == 1 ? "mono" : "stereo");

    // project.cpp always writes the stereo R,L stream whatever `channels` says (:179-195).
    const int out_channels = mono_product ? FMRX_MONO : FMRX_STEREO;
    fmrx_config cfg;
    if (fmrx_config_default(&cfg, mode, out_channels) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
        return 1;
    }
    cfg.device = device;
    cfg.rf_taps = rf_taps;
    fmrx_geometry_t geo;
    fmrx_ctx* ctx = nullptr;
    if (fmrx_geometry(&cfg, &geo) != FMRX_OK || fmrx_create(&cfg, &ctx) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
        return 1;
    }
    if (iq_format != FMRX_IQ_U8 && fmrx_set_input_format(ctx, iq_format) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: --iq-format: %s\n", fmrx_last_error());
        fmrx_destroy(ctx);
        return 1;
    }
    if (wide && fmrx_set_capture_decim(ctx, capture_decim) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: --capture-decim: %s\n", fmrx_last_error());
        fmrx_destroy(ctx);
        return 1;
    }
    // what one read unit is: a block, or with --capture-rate a granule of unit_blocks blocks
    size_t unit_blocks = 1, unit_pairs = geo.iq_pairs * (size_t)capture_decim;
    if (have_rate) {
        int d = 1;
        if (fmrx_set_capture_rate(ctx, (int)capture_rate) != FMRX_OK || fmrx_capture_decim(ctx, &d) != FMRX_OK ||
            fmrx_wide_granule(ctx, &unit_blocks, &unit_pairs) != FMRX_OK) {
            std::fprintf(stderr, "fmrx: --capture-rate: %s\n", fmrx_last_error());
            fmrx_destroy(ctx);
            return 1;
        }
        wide = d != 1;  // fmrx_capture_decim reads 1 at the mode's own rate alone (D, or 0 at a rational ratio): no wide capture
    }
    const size_t pair_bytes = (size_t)fmrx_iq_pair_bytes(iq_format);
    const size_t block_bytes = unit_pairs * pair_bytes;  // bytes a read unit; geo.block_bytes for u8 at the mode's rate
    batch = (int)(std::max<size_t>(1, (size_t)batch / unit_blocks) * unit_blocks);  // whole units
    if (scan) {
        const int rc = scan_bytes > 0 ? scan_stdin(ctx, (size_t)scan_bytes, pair_bytes, wide) : 1;
        if (scan_bytes <= 0) std::fprintf(stderr, "fmrx: --scan-bytes must be positive\n");
        fmrx_destroy(ctx);
        return rc;
    }
    if (have_deemph && fmrx_set_deemphasis(ctx, deemph_us) != FMRX_OK) {
        std::fprintf(stderr, "fmrx: --deemph: %s\n", fmrx_last_error());
        fmrx_destroy(ctx);
        return 1;
    }
    // --rds, --meter: whole RDS granules (the meter's frames) a batch (rounded up), decoded by the tuned front end
    size_t rds_unit = unit_blocks;
    if (rds || meter || blend || afc) {
        if (fmrx_rds_granule(ctx, &rds_unit) != FMRX_OK || (rds && fmrx_set_rds(ctx, 1) != FMRX_OK) ||
            (rds_sync && fmrx_set_rds_sync(ctx, 1) != FMRX_OK) ||
            (meter && fmrx_set_meter(ctx, 1) != FMRX_OK) || (blend && fmrx_set_stereo_blend(ctx, 1, nullptr) != FMRX_OK) ||
            (afc && fmrx_set_afc(ctx, nullptr, 1) != FMRX_OK)) {
            std::fprintf(stderr, "fmrx: %s: %s\n", rds ? "--rds" : meter ? "--meter" : blend ? "--blend" : "--afc", fmrx_last_error());
            fmrx_destroy(ctx);
            return 1;
        }
        batch = (int)(((size_t)batch + rds_unit - 1) / rds_unit * rds_unit);
    }
    if (tuned || wide || rds || meter || blend || afc) {  // out of range (or no 32-bit value) -> message, exit 1
        const int32_t f = (int32_t)offset_hz;
        if ((long)f != offset_hz || (wide ? fmrx_tune_wide : fmrx_tune)(ctx, &f, 0) != FMRX_OK) {
            std::fprintf(stderr, "fmrx: --offset-hz %ld: %s\n", offset_hz,
                         (long)f != offset_hz ? "out of range" : fmrx_last_error());
            fmrx_destroy(ctx);
            return 1;
        }
    }
    const size_t in_cap = block_bytes * ((size_t)batch / unit_blocks);
    const size_t out_cap = geo.pcm_samples * (size_t)batch;

    CLI_HIP(hipSetDevice(device));
    hipStream_t compute = static_cast<hipStream_t>(fmrx_stream(ctx));
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
                std::fwrite(s.h_out, sizeof(int16_t), s.blocks * geo.pcm_samples, stdout);
            }
            if (s.last) return;
            free_q.push(i);
        }
    });

    auto process = wide ? fmrx_process_wide_device : fmrx_process_device;
    for (;;) {
        const int i = filled_q.pop();
        Slot& s = slots[i];
        if (s.blocks > 0) {
            // with --rds, --meter or --blend: the whole granules, then (end of input only) the blocks left over without
            // RDS and meter, blended at the last level
            const size_t head = s.blocks / rds_unit * rds_unit;
            CLI_HIP(hipMemcpyAsync(s.d_in, s.h_in, s.blocks / unit_blocks * block_bytes, hipMemcpyHostToDevice, up));
            CLI_HIP(hipEventRecord(s.uploaded, up));
            CLI_HIP(hipStreamWaitEvent(compute, s.uploaded, 0));
            if ((head > 0 && process(ctx, s.d_in, head, s.d_out) != FMRX_OK) ||
                (head < s.blocks && (fmrx_set_rds(ctx, 0) != FMRX_OK || fmrx_set_meter(ctx, 0) != FMRX_OK ||
                                     (afc && fmrx_set_afc(ctx, nullptr, 0) != FMRX_OK) ||
                                     (blend && fmrx_blend_hold(ctx, 1) != FMRX_OK) ||
                                     process(ctx, s.d_in + head / unit_blocks * block_bytes, s.blocks - head,
                                             s.d_out + head * geo.pcm_samples) != FMRX_OK))) {
                std::fprintf(stderr, "fmrx: %s\n", fmrx_last_error());
                std::fflush(stdout);
                std::_Exit(1);
            }
            CLI_HIP(hipEventRecord(s.computed, compute));
            CLI_HIP(hipStreamWaitEvent(down, s.computed, 0));
            CLI_HIP(hipMemcpyAsync(s.h_out, s.d_out, s.blocks * geo.pcm_samples * sizeof(int16_t),
                                   hipMemcpyDeviceToHost, down));
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
    if (rds) {
        fmrx_rds_info info;
        if (fmrx_rds_info_get(ctx, 0, &info) == FMRX_OK)
            std::fprintf(stderr, "rds pi=%04X pty=%d ps=\"%s\" groups=%d\n", (unsigned)info.pi, (int)info.pty, info.ps,
                         (int)info.groups);
    }
    if (rds_sync) {
        fmrx_rds_ext x;
        if (fmrx_rds_blocks_flush(ctx, nullptr, 0, nullptr) == FMRX_OK && fmrx_rds_ext_get(ctx, 0, &x) == FMRX_OK) {
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
    }
    if (meter) {
        fmrx_meter_report rep;
        fmrx_subcarriers sc{};
        if (fmrx_meter_get(ctx, 0, &rep) == FMRX_OK && (rep.frames == 0 || fmrx_meter_detect(&rep, nullptr, &sc) == FMRX_OK))
            std::fprintf(stderr, "meter pilot_snr=%.1f stereo=%d rds_snr=%.1f rds=%d frames=%llu\n", (double)sc.pilot_snr_db,
                         sc.stereo, (double)sc.rds_snr_db, sc.rds, (unsigned long long)rep.frames);
    }
    if (afc) {
        fmrx_afc_status st;
        if (fmrx_afc_get(ctx, 0, &st) == FMRX_OK)
            std::fprintf(stderr, "afc offset=%+d err=%+.0f carrier=%d retunes=%u frames=%llu\n", (int)st.offset_hz, st.last.err_hz,
                         st.last.carrier, st.retunes, (unsigned long long)st.total.frames);
    }
    if (blend) {
        fmrx_blend_report rep;
        if (fmrx_blend_get(ctx, 0, &rep) == FMRX_OK) {
            double sum = 0.0;
            for (int l = 0; l <= 16; l++) sum += (double)l * (double)rep.level_frames[l];
            std::fprintf(stderr, "blend mean=%.2f full=%llu mono=%llu frames=%llu\n", rep.frames ? sum / (16.0 * (double)rep.frames) : 0.0,
                         (unsigned long long)rep.level_frames[16], (unsigned long long)rep.level_frames[0],
                         (unsigned long long)rep.frames);
        }
    }
    fmrx_destroy(ctx);
    std::fprintf(stderr, "End of input stream reached!\n");
    return 0;
}
