// test_raw_ingest_host.cpp -- the host mirror's native-format ingest (cubicsdr_amd/host/Adapters.h RawIQStreamSource, RawStreamReblocker, the raw
// DeviceIngest, convertRawIQ), driven by tests/test_raw_ingest_host.py.
//   ./test_raw_ingest_host cpu <raw.bin> <expected.bin> <format> <full_scale> <offset> <mtu> <swap_on_read> <swap_off_read>
//        the raw stream through RawStreamReblocker without an ingest (host fall-back): blocks of 800 samples from reads of <mtu>, the I/Q option
//        switched on from read <swap_on_read> and off again from read <swap_off_read>, then a saturated consumer; every block's `data` must equal
//        the expected CF32 stream (the numpy conversion the test wrote) bit for bit
//   ./test_raw_ingest_host gpu <raw_cs16.bin> <cf32.bin> <nb> <sample_rate> <demod_offset>
//        nb blocks at <sample_rate> (2.4 MS/s: 4 channels; 480 kS/s: the single-channel branch): the CS16 stream through RawStreamReblocker + the raw
//        DeviceIngest -> SDRPostThread with "IQDataOutput" bound to the waterfall's FFTDataDistributor -> NBFM audio, waterfall lines and frames,
//        against the same samples fed as CF32 blocks; all three must be identical
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <thread>

#include "../../cubicsdr_amd/host/HipPipeline.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

static std::vector<unsigned char> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

// a device that hands out a recorded stream in reads of at most maxElems samples; `onRead` runs inside every read (a user action in mid-block)
struct RecordedSource : RawIQStreamSource {
    const std::vector<unsigned char> &bytes;
    size_t bps, pos = 0;
    int reads = 0;
    std::function<void(int)> onRead;
    RecordedSource(const std::vector<unsigned char> &b, size_t bps_) : bytes(b), bps(bps_) {}
    int readStream(void *buff, int maxElems) override {
        const size_t left = bytes.size() / bps - pos, n = std::min(left, (size_t)maxElems);
        std::memcpy(buff, bytes.data() + pos * bps, n * bps);
        pos += n;
        if (onRead) onRead(reads);
        ++reads;
        return (int)n;
    }
};

static int run_cpu(char **a) {
    const std::vector<unsigned char> raw = slurp(a[0]), want = slurp(a[1]);
    csdr_iq_format fmt{};
    fmt.format = std::atoi(a[2]); fmt.full_scale = std::atof(a[3]); fmt.offset = (float)std::atof(a[4]);
    const int mtu = std::atoi(a[5]), swapOn = std::atoi(a[6]), swapOff = std::atoi(a[7]);
    const size_t bps = iqSampleBytes(fmt.format);
    CHECK(bps > 0 && !raw.empty() && want.size() == raw.size() / bps * 8);
    RawStreamReblocker rb(fmt);
    rb.setSampleRate(48000); rb.setFrequency(100000000); rb.setMTU(mtu);
    const int block = rb.getNumElems();
    CHECK(block == 800 && rb.getNumChannels() == 1);
    CHECK(!rb.setScale(0.0, fmt.offset) && !rb.setScale(-1.0, fmt.offset) && !rb.setScale(std::nan(""), fmt.offset) && !rb.setScale(fmt.full_scale, std::nanf("")));
    CHECK((fmt.format == CSDR_IQ_CU8) == rb.setScale(fmt.full_scale, fmt.offset + 1.0f));      // an offset only where the format has one
    CHECK(rb.setScale(fmt.full_scale, fmt.offset));
    RecordedSource dev(raw, bps);
    dev.onRead = [&](int r) { if (r + 1 == swapOn) rb.setIQSwap(true); if (r + 1 == swapOff) rb.setIQSwap(false); };   // takes effect at the next read
    std::atomic_bool stopping{false};
    auto q = std::make_shared<SDRThreadIQDataQueue>();                  // room for one block
    auto same = [&](const SDRThreadIQDataPtr &blk, int index) {
        CHECK(blk && blk->data.size() == (size_t)block && blk->numSamples() == (size_t)block && blk->rawSamples == (size_t)block);
        CHECK(!blk->deviceData && !blk->iqSwapPending && blk->sampleRate == 48000 && blk->numChannels == 1);
        if (blk && blk->data.size() == (size_t)block) CHECK(!std::memcmp(blk->data.data(), want.data() + (size_t)index * block * 8, (size_t)block * 8));
    };
    SDRThreadIQDataPtr blk;
    for (int b = 0; b < 4; ++b) {
        CHECK(rb.readStream(dev, q, stopping) > 0);
        CHECK(q->try_pop(blk));
        same(blk, b);
        CHECK(rb.pendingOverflow() == ((b + 1) * block + mtu - 1) / mtu * mtu - (b + 1) * block);     // the surplus of the last read, in samples
    }
    blk.reset();
    // a saturated consumer loses the block; the stream goes on from where the lost block ended
    CHECK(rb.readStream(dev, q, stopping) > 0);                          // block 4 waits in the queue
    CHECK(rb.readStream(dev, q, stopping) == 0);                         // block 5 is read and lost
    CHECK(q->try_pop(blk));
    same(blk, 4);
    blk.reset();
    CHECK(rb.readStream(dev, q, stopping) > 0);
    CHECK(q->try_pop(blk));
    same(blk, 6);
    CHECK(dev.reads > swapOff);
    std::printf(g_fail ? "raw ingest host FAILED (%d)\n" : "raw ingest host test ok\n", g_fail);
    return g_fail ? 1 : 0;
}

// What nb blocks through SDRPostThread give: the NBFM audio, and -- with "IQDataOutput" bound, as CubicSDR binds it -- the waterfall: the lines
// FFTDataDistributor cuts from the full-rate blocks and the frames SpectrumVisualProcessor makes of them.  The distributor and its processor are
// wired as FFTVisualDataThread wires them but pumped here after every block, so that which lines go out does not depend on thread timing.
struct PipelineOutput {
    std::vector<std::vector<float>> audio;
    std::vector<std::vector<liquid_float_complex_t>> lines;
    std::vector<std::vector<float>> frames;
};
static bool sameBytes(const void *a, const void *b, size_t n) { return !std::memcmp(a, b, n); }

static PipelineOutput run_pipeline(csdr_ctx *ctx, int nb, long long demodOffset, const std::function<void(int, const SDRThreadIQDataQueuePtr &)> &feed) {
    PipelineOutput o;
    DemodulatorMgr mgr(4);
    SDRPostThread post(ctx, &mgr);
    auto in = std::make_shared<SDRThreadIQDataQueue>();
    in->set_max_num_items(4);
    post.setInputQueue("IQDataInput", in);
    auto iqOut = std::make_shared<DemodulatorThreadInputQueue>();
    iqOut->set_max_num_items(4);
    post.setOutputQueue("IQDataOutput", iqOut);
    FFTDataDistributor distrib;
    SpectrumVisualProcessor wproc(ctx);
    auto fftQueue = std::make_shared<DemodulatorThreadInputQueue>(), lineTap = std::make_shared<DemodulatorThreadInputQueue>();
    auto fftOut = std::make_shared<SpectrumVisualDataQueue>();
    fftQueue->set_max_num_items(100); lineTap->set_max_num_items(1000); fftOut->set_max_num_items(1000);
    distrib.setInput(iqOut);
    distrib.attachOutput(fftQueue);
    distrib.attachOutput(lineTap);
    wproc.setInput(fftQueue);
    wproc.attachOutput(fftOut);
    wproc.setup(512);
    const int want = wproc.getDesiredInputSize();                                   // the line length FFTVisualDataThread asks the distributor for
    CHECK(want > 0);
    distrib.setFFTSize(want > 0 ? (unsigned)want : 1024u);
    distrib.setLinesPerSecond(600);
    auto d = mgr.newThread();
    d->setDemodulatorType("NBFM");
    d->setFrequency(100000000 + demodOffset);
    std::thread tp(&IOThread::threadMain, &post);
    SpectrumVisualDataPtr sv;
    for (int b = 0; b < nb; ++b) {
        feed(b, in);
        while (post.blocksProcessed.load() <= b) std::this_thread::sleep_for(std::chrono::milliseconds(1));
        distrib.run();
        for (int guard = 0; guard < 1000 && !wproc.isInputEmpty(); ++guard) {      // (the processor takes an input only while its output queue is empty)
            wproc.run();
            while (fftOut->try_pop(sv)) o.frames.push_back(sv->spectrum_points);
        }
    }
    CHECK(post.errlog.errorCount() == 0 && wproc.errlog.errorCount() == 0);
    auto aq = d->getAudioOutputQueue();
    AudioThreadInputPtr ati;
    while (aq->try_pop(ati)) o.audio.push_back(ati->data);
    DemodulatorThreadIQDataPtr line;
    while (lineTap->try_pop(line)) o.lines.push_back(line->data);
    post.terminate();
    tp.join();
    return o;
}

static int run_gpu(const char *rawPath, const char *cfPath, int nb, long long fs, long long demodOffset) {
    const long long center = 100000000;
    const BlockGeometry geo = BlockGeometry::forRate(fs);
    const int block = geo.elems, mtu = std::min(16384, block / 2 + 1);
    const std::vector<unsigned char> raw = slurp(rawPath), cf = slurp(cfPath);
    CHECK(raw.size() >= ((size_t)(nb + 1) * block + mtu) * 4 && cf.size() == raw.size() * 2);
    csdr_ctx *ctx = nullptr;
    csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
    {
        csdr_iq_format fmt{};
        fmt.format = CSDR_IQ_CS16; fmt.full_scale = 32768.0; fmt.offset = 0.0f;
        RawStreamReblocker rb(fmt, ctx);
        rb.setSampleRate(fs); rb.setFrequency(center); rb.setMTU(mtu);
        CHECK(rb.getNumElems() == block && rb.getNumChannels() == geo.channels);
        CHECK(!rb.setScale(0.0, 0.0f) && !rb.setScale(32768.0, 1.0f) && rb.setScale(32768.0, 0.0f));
        DeviceIngest ingest(ctx, block + mtu, fmt, 4);
        rb.bindIngest(&ingest);
        RecordedSource dev(raw, 4);
        std::atomic_bool stopping{false};
        int inHbm = 0;
        auto a = run_pipeline(ctx, nb, demodOffset, [&](int, const SDRThreadIQDataQueuePtr &in) { CHECK(rb.readStream(dev, in, stopping) > 0); });
        {   // the blocks really went through the device copy, and carry no host samples
            auto probe = std::make_shared<SDRThreadIQDataQueue>();
            CHECK(rb.readStream(dev, probe, stopping) > 0);
            SDRThreadIQDataPtr blk;
            CHECK(probe->try_pop(blk) && blk->data.empty() && blk->numSamples() == (size_t)block && blk->rawSamples == (size_t)block);
            if (blk && blk->deviceData && blk->deviceSamples == (size_t)block) ++inHbm;
        }
        CHECK(inHbm == 1);
        auto b = run_pipeline(ctx, nb, demodOffset, [&](int k, const SDRThreadIQDataQueuePtr &in) {
            auto blk = std::make_shared<SDRThreadIQData>();
            blk->frequency = center; blk->sampleRate = fs; blk->numChannels = geo.channels;
            blk->data.resize(block);
            std::memcpy(blk->data.data(), cf.data() + (size_t)k * block * 8, (size_t)block * 8);
            CHECK(in->push(blk));
        });
        CHECK((int)a.audio.size() == nb && a.audio.size() == b.audio.size());
        size_t total = 0;
        for (size_t k = 0; k < a.audio.size() && k < b.audio.size(); ++k) {
            CHECK(a.audio[k].size() == b.audio[k].size() && !a.audio[k].empty());
            if (a.audio[k].size() == b.audio[k].size()) CHECK(sameBytes(a.audio[k].data(), b.audio[k].data(), a.audio[k].size() * sizeof(float)));
            total += a.audio[k].size();
        }
        // the waterfall of the raw feed is the CF32 feed's: the same lines (the samples the distributor cut) and the same frames
        CHECK(!a.lines.empty() && a.lines.size() == b.lines.size() && !a.frames.empty() && a.frames.size() == b.frames.size());
        for (size_t k = 0; k < a.lines.size() && k < b.lines.size(); ++k)
            CHECK(!a.lines[k].empty() && a.lines[k].size() == b.lines[k].size() && sameBytes(a.lines[k].data(), b.lines[k].data(), a.lines[k].size() * 8));
        for (size_t k = 0; k < a.frames.size() && k < b.frames.size(); ++k)
            CHECK(!a.frames[k].empty() && a.frames[k].size() == b.frames[k].size() && sameBytes(a.frames[k].data(), b.frames[k].data(), a.frames[k].size() * sizeof(float)));
        std::printf("AUDIO %zu blocks %zu samples\n", a.audio.size(), total);
        std::printf("WATERFALL %zu lines %zu frames channels %d\n", a.lines.size(), a.frames.size(), geo.channels);
    }
    csdr_ctx_destroy(ctx);
    std::printf(g_fail ? "raw ingest host gpu FAILED (%d)\n" : "raw ingest host gpu ok\n", g_fail);
    return g_fail ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 6 && !std::strcmp(argv[1], "gpu")) return run_gpu(argv[2], argv[3], std::atoi(argv[4]), std::atoll(argv[5]), std::atoll(argv[6]));
    if (argc > 9 && !std::strcmp(argv[1], "cpu")) return run_cpu(argv + 2);
    std::printf("usage: see the head of this file\n");
    return 2;
}
