// test_waterfall_host.cpp -- the host mirror's waterfall (cubicsdr_amd/host/WaterfallPanel.h: WaterfallPanel, WaterfallFeed), driven by
// tests/test_waterfall_host.py.
//   ./test_waterfall_host cpu <frames.bin> <plan.txt> <out_prefix> <fft_size> <lines> <lps>
//        a host panel (no context) behind the pacing rule: plan.txt holds one turn per line, "<elapsed seconds> <entries pushed before the turn ...>",
//        an entry being a frame index of frames.bin ((x, y) pairs), -1 for a null entry, -2 for a frame of the wrong size.  Writes both textures and the
//        picture (five-stop gradient given as <r g b> triples in the plan's first line) to <out_prefix>.tex0 / .tex1 / .rgba and prints the state;
//        the Python test compares all of it with its numpy model.
//   ./test_waterfall_host gpu <iq.bin> <n_blocks> <block_len> <sample_rate> <fft_size> <lines>
//        blocks of IQ through FFTVisualDataThread's distributor and processor, pumped as its run() pumps them; every frame that comes out is stepped
//        twice: HBM to HBM with stepFrom() into a device panel, and from the fetched SpectrumVisualData into a device panel AND a host panel.
//        The three panels must hold the same textures, offsets and picture.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/WaterfallPanel.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

template <typename T> static std::vector<T> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(b.size() / sizeof(T));
    std::memcpy(v.data(), b.data(), v.size() * sizeof(T));
    return v;
}
static void dump(const std::string &path, const std::vector<unsigned char> &v) { std::ofstream(path, std::ios::binary).write((const char *)v.data(), (std::streamsize)v.size()); }

static int run_cpu(const char *framesPath, const char *planPath, const std::string &prefix, unsigned fft, int lines, int lps) {
    const std::vector<float> frames = slurp<float>(framesPath);
    const size_t per = (size_t)fft * 2;
    CHECK(!frames.empty() && frames.size() % per == 0);
    WaterfallPanel panel;                                           // no context: the host arithmetic
    CHECK(!panel.onDevice());
    panel.setup(fft, lines);
    WaterfallFeed feed;
    feed.linesPerSecond = lps;
    SpectrumVisualDataQueue q;
    q.set_max_num_items(1000);
    std::ifstream plan(planPath);
    std::string ln;
    std::getline(plan, ln);
    {
        std::istringstream is(ln);
        std::vector<float> stops;
        float c;
        while (is >> c) stops.push_back(c);
        CHECK(stops.size() >= 6 && panel.setGradient(stops));
        CHECK(!panel.setGradient(std::vector<float>(3, 0.5f)));     // one stop is refused
    }
    int turns = 0, updates = 0;
    while (std::getline(plan, ln)) {
        std::istringstream is(ln);
        double elapsed;
        if (!(is >> elapsed)) continue;
        long e;
        while (is >> e) {
            SpectrumVisualDataPtr v;
            if (e >= 0) { v = std::make_shared<SpectrumVisualData>(); v->spectrum_points.assign(frames.begin() + (size_t)e * per, frames.begin() + (size_t)(e + 1) * per); }
            else if (e == -2) { v = std::make_shared<SpectrumVisualData>(); v->spectrum_points.assign(10, 0.5f); }
            CHECK(q.push(v));
        }
        if (feed.processInputQueue(elapsed, q, panel, fft)) ++updates;
        ++turns;
    }
    std::vector<unsigned char> t0, t1, pic;
    CHECK(panel.fetchIndex(0, t0) && panel.fetchIndex(1, t1) && panel.fetchRGBA(0, lines, pic));
    dump(prefix + ".tex0", t0); dump(prefix + ".tex1", t1); dump(prefix + ".rgba", pic);
    std::printf("STATE turns %d updates %d stepped %ld ofs0 %d ofs1 %d buffered %d queued %zu lpsIndex %.17g\n", turns, updates, feed.stepped, panel.getOffset(0),
                panel.getOffset(1), panel.getLinesBuffered(), q.size(), feed.lpsIndex);
    std::printf(g_fail ? "waterfall host FAILED (%d)\n" : "waterfall host test ok\n", g_fail);
    return g_fail ? 1 : 0;
}

// FFTVisualDataThread with its loop body callable from the test: what run() does per tick, without the sleep, so that the lines that go out do not
// depend on thread timing
class PumpedFFTVisualDataThread : public FFTVisualDataThread {
public:
    explicit PumpedFFTVisualDataThread(csdr_ctx *ctx) : FFTVisualDataThread(ctx) {}
    void wire(unsigned fft) {
        in = std::make_shared<DemodulatorThreadInputQueue>();
        out = std::make_shared<SpectrumVisualDataQueue>();
        in->set_max_num_items(8); out->set_max_num_items(100); fftQueue->set_max_num_items(100);
        setInputQueue("IQDataInput", in);
        setOutputQueue("FFTDataOutput", out);
        fftDistrib.setInput(in);
        fftDistrib.attachOutput(fftQueue);
        wproc.setInput(fftQueue);
        wproc.attachOutput(out);
        wproc.setup(fft);
    }
    // one tick; `onFrame` runs right behind every frame the processor made, on this thread
    template <typename Fn> void tick(Fn onFrame) {
        const int want = wproc.getDesiredInputSize();
        fftDistrib.setFFTSize(want ? (unsigned)want : DEFAULT_FFT_SIZE * 2);
        if (lpsChanged.load()) { fftDistrib.setLinesPerSecond((unsigned)linesPerSecond.load()); lpsChanged.store(false); }
        fftDistrib.run();
        SpectrumVisualDataPtr sv;
        for (int guard = 0; guard < 1000 && !wproc.isInputEmpty(); ++guard) {
            wproc.run();
            while (out->try_pop(sv)) onFrame(wproc, sv);
        }
    }
    DemodulatorThreadInputQueuePtr in;
    SpectrumVisualDataQueuePtr out;
};

static int run_gpu(const char *iqPath, int nb, int block, long long fs, unsigned fft, int lines) {
    const std::vector<liquid_float_complex_t> iq = slurp<liquid_float_complex_t>(iqPath);
    CHECK(iq.size() >= (size_t)nb * block);
    csdr_ctx *ctx = nullptr;
    csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
    {
        PumpedFFTVisualDataThread th(ctx);
        th.wire(fft);
        th.setLinesPerSecond(600);
        th.getProcessor()->setHideDC(true);
        th.getProcessor()->setCenterFrequency(100000000);
        th.getProcessor()->setBandwidth((long)fs);
        WaterfallPanel hbm(ctx, 64), viaHost(ctx, 64), host;
        const std::vector<float> stops = {0.0f, 0.0f, 0.2f, 0.1f, 0.9f, 1.2f, 1.0f, 1.0f, -0.1f, 1.0f, 0.3f, 0.3f};
        WaterfallPanel *all[3] = {&hbm, &viaHost, &host};
        for (auto *p : all) { p->setup(fft, lines); CHECK(p->setGradient(stops)); p->step(); p->update(); }      // (the first step is dropped; the update makes the textures)
        int frames = 0, updates = 0;
        for (int b = 0; b < nb; ++b) {
            auto blk = std::make_shared<DemodulatorThreadIQData>();
            blk->frequency = 100000000; blk->sampleRate = fs;
            blk->data.assign(iq.begin() + (size_t)b * block, iq.begin() + (size_t)(b + 1) * block);
            CHECK(th.in->push(blk));
            int got = 0;
            th.tick([&](SpectrumVisualProcessor &proc, const SpectrumVisualDataPtr &sv) {
                CHECK(sv && sv->spectrum_points.size() == (size_t)fft * 2);
                CHECK(hbm.stepFrom(proc));
                viaHost.setPoints(sv->spectrum_points); viaHost.step();
                host.setPoints(sv->spectrum_points); host.step();
                ++got;
            });
            frames += got;
            if (got && (b % 3 == 2 || hbm.getLinesBuffered() > 40)) { for (auto *p : all) p->update(); ++updates; }
        }
        for (auto *p : all) p->update();
        CHECK(frames > lines && updates >= 3);                       // the ring went round
        CHECK(th.getProcessor()->errlog.errorCount() == 0);
        std::vector<unsigned char> want, got, wantPic, gotPic;
        for (auto *p : all) CHECK(p->errlog.errorCount() == 0 && p->getLinesBuffered() == 0 && p->getOffset(0) == host.getOffset(0) && p->getOffset(1) == host.getOffset(1));
        CHECK(host.fetchRGBA(1, lines - 1, wantPic));
        for (int j = 0; j < 2; ++j) {
            CHECK(host.fetchIndex(j, want));
            size_t distinct = 0;
            { bool seen[256] = {false}; for (unsigned char c : want) if (!seen[c]) { seen[c] = true; ++distinct; } }
            CHECK(distinct > 8);
            for (auto *p : {&hbm, &viaHost}) { CHECK(p->fetchIndex(j, got)); CHECK(got == want); }
        }
        for (auto *p : {&hbm, &viaHost}) { CHECK(p->fetchRGBA(1, lines - 1, gotPic)); CHECK(gotPic == wantPic); }
        std::printf("WATERFALL frames %d updates %d offset %d\n", frames, updates, host.getOffset(0));
    }
    csdr_ctx_destroy(ctx);
    std::printf(g_fail ? "waterfall host gpu FAILED (%d)\n" : "waterfall host gpu ok\n", g_fail);
    return g_fail ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 7 && !std::strcmp(argv[1], "gpu")) return run_gpu(argv[2], std::atoi(argv[3]), std::atoi(argv[4]), std::atoll(argv[5]), (unsigned)std::atoi(argv[6]), std::atoi(argv[7]));
    if (argc > 7 && !std::strcmp(argv[1], "cpu")) return run_cpu(argv[2], argv[3], argv[4], (unsigned)std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]));
    std::printf("usage: see the head of this file\n");
    return 2;
}
