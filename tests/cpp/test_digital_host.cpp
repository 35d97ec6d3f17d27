// test_digital_host.cpp -- the host mirror's digital lab (cubicsdr_amd/host/ModemDigital.h, HipPipeline.h), driven by tests/test_digital_host.py.
//   ./test_digital_host cpu                      : registry (opt-in registration, names, default rates), settings round trip, DemodulatorInstance extras
//   ./test_digital_host gpu <blocks.bin> <nb>    : nb blocks of 40000 complex-float samples at 2.4 MS/s, M = 4, through SDRPostThread with an FSK and a
//                                                  QPSK demodulator; prints the FSK console text and the QPSK lock after every block
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>
#include <thread>

#include "../../cubicsdr_amd/host/HipPipeline.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

struct TextOutput : ModemDigitalOutput {
    std::string text;
    int writes = 0, shows = 0;
    void write(std::string outp) override { text += outp; ++writes; }
    void write(char outc) override { text += outc; ++writes; }
    void Show() override { ++shows; }
    void Hide() override {}
    void Close() override {}
};

static int run_cpu() {
    CHECK(Modem::getFactories().size() == 9);                        // registerBuiltins() alone: the nine analog modems
    CHECK(Modem::makeModem("PSK") == nullptr);
    Modem::registerDigitalLab();
    Modem::registerDigitalLab();                                      // (once)
    auto f = Modem::getFactories();
    CHECK(f.size() == 17);
    for (const char *n : {"ASK", "BPSK", "DPSK", "OOK", "PSK", "QAM", "QPSK"}) CHECK(f.count(n) == 1 && Modem::getModemDefaultSampleRate(n) == 200000);
    CHECK(f.count("FSK") == 1 && Modem::getModemDefaultSampleRate("FSK") == 19200);
    for (const char *n : {"APSK", "SQAM", "ST", "GMSK"}) CHECK(f.count(n) == 0);
    for (auto &kv : f) {
        std::unique_ptr<Modem> m(Modem::makeModem(kv.first));
        CHECK(m && m->getName() == kv.first);
        const std::set<std::string> digital = {"ASK", "BPSK", "DPSK", "FSK", "OOK", "PSK", "QAM", "QPSK"};
        if (digital.count(kv.first)) CHECK(m->getType() == "digital" && m->csdrModemId() == CSDR_MODEM_DIGITAL);
        else CHECK(m->getType() == "analog");
    }
    // cons settings (ModemPSK.cpp:39-94 and alike)
    for (const char *n : {"PSK", "DPSK", "ASK", "QAM"}) {
        std::unique_ptr<Modem> m(Modem::makeModem(n));
        auto args = m->getSettings();
        const bool qam = !std::strcmp(n, "QAM");
        CHECK(args.size() == 1 && args[0].key == "cons" && args[0].name == "Constellation" && args[0].options.size() == (qam ? 7u : 8u));
        CHECK(args[0].options.front() == (qam ? "4" : "2") && args[0].options.back() == "256");
        CHECK(m->readSetting("cons") == (qam ? "4" : "2"));
        m->writeSetting("cons", "64");
        CHECK(m->readSetting("cons") == "64" && m->readSettings()["cons"] == "64" && !m->shouldRebuildKit());
        auto *md = dynamic_cast<ModemDigital *>(m.get());
        CHECK(md && md->csdrDigitalCons() == 64 && md->csdrDigitalParams().cons == 64);
        CHECK(m->checkSampleRate(100, 48000) == MIN_BANDWIDTH && m->checkSampleRate(200000, 48000) == 200000);
    }
    for (const char *n : {"BPSK", "QPSK", "OOK"}) { std::unique_ptr<Modem> m(Modem::makeModem(n)); CHECK(m->getSettings().empty()); }
    {   // FSK: bps / sps / bw, every write asks for a rebuild (ModemFSK.cpp:78-90), checkSampleRate :19-28
        std::unique_ptr<Modem> m(Modem::makeModem("FSK"));
        CHECK(m->readSetting("bps") == "1" && m->readSetting("sps") == "9600" && m->readSetting("bw") == std::to_string(0.45f));
        CHECK(m->getSettings().size() == 3 && m->getDefaultSampleRate() == 19200);
        CHECK(m->checkSampleRate(19200, 48000) == 19200);
        m->writeSetting("bps", "4");
        CHECK(m->shouldRebuildKit() && m->readSetting("bps") == "4");
        CHECK(m->checkSampleRate(19200, 48000) == 2 * 4 * 9600);
        m->clearRebuildKit();
        m->writeSetting("sps", "1200"); m->writeSetting("bw", "0.3");
        CHECK(m->shouldRebuildKit() && m->readSetting("sps") == "1200" && m->readSetting("bw") == std::to_string(0.3f));
        auto p = dynamic_cast<ModemDigital *>(m.get())->csdrDigitalParams();
        CHECK(p.kind == CSDR_DIGITAL_FSK && p.bps == 4 && p.sps == 1200 && p.bw == 0.3f);
        uint32_t s[4] = {0, 10, 15, 3};
        CHECK(ModemFSK::hexText(s, 4) == "0af3");
    }
    {   // DemodulatorInstance: lock and output (DemodulatorInstance.h:85-86, 132)
        DemodulatorMgr mgr(2);
        auto d = mgr.newThread();
        TextOutput out;
        d->setOutput(&out);
        CHECK(d->getOutput() == &out && d->getDemodulatorLock() == 0);
        d->setDemodulatorType("PSK");
        CHECK(d->getModemType() == "digital" && d->getBandwidth() == 200000);
        d->setDemodulatorLock(true);
        CHECK(d->getDemodulatorLock() == 1);
        d->writeModemSetting("cons", "8");
        CHECK(d->readModemSetting("cons") == "8");
        d->setDemodulatorType("NBFM");
        CHECK(d->getDemodulatorLock() == 0 && d->getOutput() == &out);
    }
    std::printf(g_fail ? "digital host test FAILED (%d)\n" : "digital host test ok\n", g_fail);
    return g_fail ? 1 : 0;
}

static int run_gpu(const char *path, int nb) {
    Modem::registerDigitalLab();
    const long long fs = 2400000, center = 100000000;
    const int block = 40000;
    std::ifstream fin(path, std::ios::binary);
    std::vector<liquid_float_complex_t> all((size_t)nb * block);
    fin.read((char *)all.data(), (std::streamsize)(all.size() * sizeof(liquid_float_complex_t)));
    CHECK(fin.good());
    csdr_ctx *ctx = nullptr;
    csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
    {
        DemodulatorMgr mgr(4);
        SDRPostThread post(ctx, &mgr);
        auto in = std::make_shared<SDRThreadIQDataQueue>();
        in->set_max_num_items(4);
        post.setInputQueue("IQDataInput", in);
        auto fsk = mgr.newThread();
        fsk->setDemodulatorType("FSK");
        fsk->setFrequency(center + 620000);                 // (tests/test_digital_host.py: F_FSK, F_QPSK)
        TextOutput out;
        fsk->setOutput(&out);
        auto qpsk = mgr.newThread();
        qpsk->setDemodulatorType("QPSK");
        qpsk->setFrequency(center - 550000);
        auto vis = std::make_shared<DemodulatorThreadOutputQueue>();
        vis->set_max_num_items(4);
        qpsk->setVisualOutputQueue(vis);
        std::thread tp(&IOThread::threadMain, &post);
        for (int b = 0; b < nb; ++b) {
            auto blk = std::make_shared<SDRThreadIQData>();
            blk->frequency = center; blk->sampleRate = fs; blk->numChannels = 4;
            blk->data.assign(all.begin() + (long)b * block, all.begin() + (long)(b + 1) * block);
            CHECK(in->push(blk));
            while (post.blocksProcessed.load() <= b) std::this_thread::sleep_for(std::chrono::milliseconds(1));
            std::printf("LOCK %d %d\n", b, qpsk->getDemodulatorLock());
            std::printf("FSKLOCK %d %d\n", b, fsk->getDemodulatorLock());
            std::printf("LEVEL %d %.3f\n", b, (double)qpsk->getSignalLevel());
        }
        AudioThreadInputPtr f;
        int frames = 0;
        while (vis->try_pop(f)) {          // the constellation frame (DemodulatorThread.cpp:256-267): n floats = the first n / 2 samples, interleaved
            ++frames;
            CHECK(f->type == 2 && f->channels == 2 && f->sampleRate == 200000 && !f->data.empty());
            std::printf("SCOPE %zu\n", f->data.size());
        }
        CHECK(frames >= 1);
        CHECK(post.errlog.errorCount() == 0);
        std::printf("TEXT %s\n", out.text.c_str());
        std::printf("WRITES %d\n", out.writes);
        post.terminate();
        tp.join();
    }
    csdr_ctx_destroy(ctx);
    std::printf(g_fail ? "digital host gpu FAILED (%d)\n" : "digital host gpu ok\n", g_fail);
    return g_fail ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 3 && !std::strcmp(argv[1], "gpu")) return run_gpu(argv[2], std::atoi(argv[3]));
    return run_cpu();
}
