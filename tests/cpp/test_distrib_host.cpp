// test_distrib_host.cpp -- the host mirror's device route for the waterfall feed (cubicsdr_amd/host/HipPipeline.h: DeviceFFTDataDistributor,
// FFTVisualDataThread::setDeviceRoute, SDRPostThread::setVisualReadback, SpectrumVisualProcessor::processLines; WaterfallPanel::stepFrom),
// driven by tests/test_distrib_host.py.
//   ./test_distrib_host gpu <raw_cs16.bin> <nb> <sample_rate> <demod_offset>
//        nb blocks at <sample_rate> (2.4 MS/s: 4 channels; 480 kS/s: the single-channel branch) from a raw CS16 source through RawStreamReblocker
//        + the raw DeviceIngest -> SDRPostThread -> "IQDataOutput" -> FFTVisualDataThread, run twice on the same samples: the default host route
//        (read-back, FFTDataDistributor, one process() per line) and the device route with both switches on.
//        1. The thread as it stands (30 lines/s of 2 * 2048 samples: a line every other block): the waterfall frames both routes distribute, with
//           their ceilings and floors, and the textures of a panel fed from them (device route: stepFrom, HBM to HBM) must be identical bit for bit.
//        2. A busy cadence (600 lines/s at fftSize 512, ten lines per block) over the first 8 blocks: the same number of frames, block by block, and
//           the same pacing state.  The frames themselves are NOT compared here: csdr_spec_process_distrib hands a push's lines over as ONE
//           csdr_spec_process call, whose floor / ceiling trackers evaluate their recurrence in closed form over the frames of a call
//           (kernels_spec.hpp, spec_trackers: equal to the serial loop to about 1e-15 relative, not to the bit) -- a property of batched
//           csdr_spec_process that exists without the distributor.  With at most one line per push, as in 1., both routes make the same calls.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <thread>

#include "../../cubicsdr_amd/host/WaterfallPanel.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

static std::vector<unsigned char> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// a device that hands out a recorded stream in reads of at most maxElems samples
struct RecordedSource : RawIQStreamSource {
    const std::vector<unsigned char> &bytes;
    size_t bps, pos = 0;
    RecordedSource(const std::vector<unsigned char> &b, size_t bps_) : bytes(b), bps(bps_) {}
    int readStream(void *buff, int maxElems) override {
        const size_t left = bytes.size() / bps - pos, n = std::min(left, (size_t)maxElems);
        std::memcpy(buff, bytes.data() + pos * bps, n * bps);
        pos += n;
        return (int)n;
    }
};

// (the thread's host distributor, for its pacing state)
struct VisualThread : FFTVisualDataThread {
    using FFTVisualDataThread::FFTVisualDataThread;
    FFTDataDistributor &hostDistributor() { return fftDistrib; }
};

struct RouteOutput {
    std::vector<std::vector<float>> frames;
    std::vector<double> ceilings, floors;
    std::vector<unsigned char> tex[2];
    std::vector<int> framesPerPump;
    int ofs[2] = {-1, -1};
    int blocksInHbmOnly = 0, blocksWithHostSamples = 0, pumpsWithSeveralFrames = 0;
    double accum = 0.0;
    size_t buffered = 0;
};

static RouteOutput run_route(csdr_ctx *ctx, const std::vector<unsigned char> &raw, int nb, long long fs, long long demodOffset, bool deviceRoute, int lps, int fftSize) {
    const long long center = 100000000;
    const BlockGeometry geo = BlockGeometry::forRate(fs);
    const int block = geo.elems, mtu = std::min(16384, block / 2 + 1), wfLines = 16;
    RouteOutput o;
    csdr_iq_format fmt{};
    fmt.format = CSDR_IQ_CS16; fmt.full_scale = 32768.0; fmt.offset = 0.0f;
    RawStreamReblocker rb(fmt, ctx);
    rb.setSampleRate(fs); rb.setFrequency(center); rb.setMTU(mtu);
    DeviceIngest ingest(ctx, block + mtu, fmt, 4);
    rb.bindIngest(&ingest);
    RecordedSource dev(raw, 4);
    std::atomic_bool stopping{false};

    DemodulatorMgr mgr(4);
    SDRPostThread post(ctx, &mgr);
    post.setVisualReadback(!deviceRoute);
    auto in = std::make_shared<SDRThreadIQDataQueue>();
    in->set_max_num_items(4);
    post.setInputQueue("IQDataInput", in);
    auto iqOut = std::make_shared<DemodulatorThreadInputQueue>(), iqTap = std::make_shared<DemodulatorThreadInputQueue>();
    iqOut->set_max_num_items(4); iqTap->set_max_num_items(4);
    post.setOutputQueue("IQDataOutput", iqOut);
    post.setOutputQueue("IQVisualDataOutput", iqTap);          // the same block object, for a look at where its samples live
    VisualThread fft(ctx);
    auto fftOut = std::make_shared<SpectrumVisualDataQueue>();
    fft.setInputQueue("IQDataInput", iqOut);
    fft.setOutputQueue("FFTDataOutput", fftOut);
    fft.setDeviceRoute(deviceRoute, 64);
    WaterfallPanel panel(ctx);
    panel.setup(fftSize, wfLines);
    int steppedInHbm = 0;
    if (deviceRoute) fft.onDeviceLines = [&](SpectrumVisualProcessor &proc, int n) { if (panel.stepFrom(proc, 0, n)) steppedInHbm += n; };
    fft.bind();
    if (fftSize != DEFAULT_FFT_SIZE) fft.getProcessor()->setFFTSize(fftSize);      // takes effect inside the first process(), as in the application
    if (lps != DEFAULT_WATERFALL_LPS) fft.setLinesPerSecond(lps);
    auto d = mgr.newThread();
    d->setDemodulatorType("NBFM");
    d->setFrequency(center + demodOffset);
    std::thread tp(&IOThread::threadMain, &post);
    SpectrumVisualDataPtr sv;
    DemodulatorThreadIQDataPtr tap;
    for (int b = 0; b < nb; ++b) {
        CHECK(rb.readStream(dev, in, stopping) > 0);
        while (post.blocksProcessed.load() <= b) std::this_thread::sleep_for(std::chrono::milliseconds(1));
        while (iqTap->try_pop(tap)) {
            if (tap->data.empty() && tap->deviceData) ++o.blocksInHbmOnly; else ++o.blocksWithHostSamples;
        }
        tap.reset();
        fft.pumpOnce();
        int got = 0;
        while (fftOut->try_pop(sv)) {
            o.frames.push_back(sv->spectrum_points); o.ceilings.push_back(sv->fft_ceiling); o.floors.push_back(sv->fft_floor);
            if (!deviceRoute) { panel.setPoints(sv->spectrum_points); panel.step(); }
            ++got;
        }
        if (got) panel.update();
        o.pumpsWithSeveralFrames += got > 1;
        o.framesPerPump.push_back(got);
    }
    CHECK(post.errlog.errorCount() == 0 && fft.getProcessor()->errlog.errorCount() == 0 && panel.errlog.errorCount() == 0);
    if (deviceRoute) {
        CHECK(fft.deviceDistributor() && fft.deviceDistributor()->errlog.errorCount() == 0);
        CHECK(steppedInHbm == (int)o.frames.size());
        if (fft.deviceDistributor()) { o.accum = fft.deviceDistributor()->lineRateAccumulator(); o.buffered = fft.deviceDistributor()->buffered(); }
    } else {
        CHECK(!fft.deviceDistributor());
        o.accum = fft.hostDistributor().lineRateAccumulator(); o.buffered = fft.hostDistributor().buffered();
    }
    for (int j = 0; j < 2; ++j) { CHECK(panel.fetchIndex(j, o.tex[j])); o.ofs[j] = panel.getOffset(j); }
    post.terminate();
    tp.join();
    return o;
}

static int run_gpu(const char *rawPath, int nb, long long fs, long long demodOffset) {
    const BlockGeometry geo = BlockGeometry::forRate(fs);
    const std::vector<unsigned char> raw = slurp(rawPath);
    CHECK(raw.size() >= ((size_t)(nb + 1) * geo.elems + 16384) * 4);
    csdr_ctx *ctx = nullptr;
    csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
    {
        // 1. the thread as it stands
        const RouteOutput a = run_route(ctx, raw, nb, fs, demodOffset, false, DEFAULT_WATERFALL_LPS, DEFAULT_FFT_SIZE);
        const RouteOutput b = run_route(ctx, raw, nb, fs, demodOffset, true, DEFAULT_WATERFALL_LPS, DEFAULT_FFT_SIZE);
        CHECK(!a.frames.empty() && a.frames.size() == b.frames.size() && a.framesPerPump == b.framesPerPump);
        for (size_t k = 0; k < a.frames.size() && k < b.frames.size(); ++k) {
            CHECK(!a.frames[k].empty() && a.frames[k].size() == b.frames[k].size() && !std::memcmp(a.frames[k].data(), b.frames[k].data(), a.frames[k].size() * sizeof(float)));
            CHECK(a.ceilings[k] == b.ceilings[k] && a.floors[k] == b.floors[k]);
        }
        for (int j = 0; j < 2; ++j) CHECK(!a.tex[j].empty() && a.tex[j] == b.tex[j] && a.ofs[j] == b.ofs[j] && a.ofs[j] >= 0);
        CHECK(a.accum == b.accum && a.buffered == b.buffered && a.pumpsWithSeveralFrames == 0);
        // where the samples of the visual blocks lived: the default route always has them on the host; with both switches on a channelized
        // block is never downloaded (the single-channel branch hands on the DC-corrected block it read back, whatever the switches say)
        CHECK(a.blocksInHbmOnly == 0 && a.blocksWithHostSamples == nb);
        if (geo.channels > 1) CHECK(b.blocksInHbmOnly == nb && b.blocksWithHostSamples == 0);
        else CHECK(b.blocksWithHostSamples == nb);
        std::printf("FRAMES %zu default %zu device several_per_pump %d channels %d hbm_only %d\n", a.frames.size(), b.frames.size(), b.pumpsWithSeveralFrames, geo.channels, b.blocksInHbmOnly);
        // 2. ten lines per block
        const RouteOutput c = run_route(ctx, raw, 8, fs, demodOffset, false, 600, 512), d = run_route(ctx, raw, 8, fs, demodOffset, true, 600, 512);
        CHECK(c.frames.size() >= 50 && c.framesPerPump == d.framesPerPump && c.accum == d.accum && c.buffered == d.buffered && d.pumpsWithSeveralFrames >= 7);
        std::printf("BUSY %zu default %zu device several_per_pump %d accum %.17g buffered %zu\n", c.frames.size(), d.frames.size(), d.pumpsWithSeveralFrames, d.accum, d.buffered);
    }
    csdr_ctx_destroy(ctx);
    std::printf(g_fail ? "distrib host gpu FAILED (%d)\n" : "distrib host gpu ok\n", g_fail);
    return g_fail ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 5 && !std::strcmp(argv[1], "gpu")) return run_gpu(argv[2], std::atoi(argv[3]), std::atoll(argv[4]), std::atoll(argv[5]));
    std::printf("usage: see the head of this file\n");
    return 2;
}
