// test_gmsk_host.cpp -- the host mirror's GMSK (cubicsdr_amd/host/ModemDigital.h ModemGMSK, Modem::registerDigitalGMSK), driven by
// tests/test_gmsk_host.py.
//   ./test_gmsk_host lab   : registerDigitalLab() alone still registers its 17 factories, without GMSK
//   ./test_gmsk_host gmsk  : registerDigitalGMSK(): the factory, its settings (ModemGMSK.cpp:35-68), rates and rebuild requests
//   ./test_gmsk_host gpu <blocks.bin> <nb> <sw> : nb blocks of 40000 complex-float samples at 2.4 MS/s, M = 4, through SDRPostThread with a GMSK
//                                                 demodulator whose "sps" is set to 8 before block sw; prints its console text, the text's length
//                                                 and the lock after every block
#include <chrono>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <thread>

#include "../../cubicsdr_amd/host/HipPipeline.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

static int run_lab() {
    Modem::registerDigitalLab();
    auto f = Modem::getFactories();
    CHECK(f.size() == 17 && f.count("GMSK") == 0);
    if (!g_fail) std::printf("gmsk host test ok\n");
    return g_fail ? 1 : 0;
}

static int run_gmsk() {
    Modem::registerDigitalGMSK();
    Modem::registerDigitalGMSK();                                     // (once)
    CHECK(Modem::getFactories().size() == 10 && Modem::getFactories().count("GMSK") == 1 && Modem::getModemDefaultSampleRate("GMSK") == 19200);
    Modem::registerDigitalLab();
    CHECK(Modem::getFactories().size() == 18);
    std::unique_ptr<Modem> m(Modem::makeModem("GMSK"));
    CHECK(m && m->getName() == "GMSK" && m->getType() == "digital" && m->csdrModemId() == CSDR_MODEM_DIGITAL);
    CHECK(m->getDefaultSampleRate() == 19200);
    CHECK(m->checkSampleRate(100, 48000) == MIN_BANDWIDTH && m->checkSampleRate(19200, 48000) == 19200);
    auto args = m->getSettings();
    CHECK(args.size() == 3);
    if (args.size() == 3) {
        CHECK(args[0].key == "fdelay" && args[0].name == "Filter delay" && args[0].units == "samples" && args[0].value == "3");
        CHECK(args[0].type == ModemArgInfo::Type::INT && args[0].range.minimum() == 1 && args[0].range.maximum() == 128);
        CHECK(args[1].key == "sps" && args[1].name == "Samples / symbol" && args[1].units == "samples/symbol" && args[1].value == "4");
        CHECK(args[1].type == ModemArgInfo::Type::INT && args[1].range.minimum() == 2 && args[1].range.maximum() == 512);
        CHECK(args[2].key == "ebf" && args[2].name == "Excess bandwidth" && args[2].value == std::to_string(0.3f));
        CHECK(args[2].type == ModemArgInfo::Type::FLOAT && args[2].range.minimum() == 0.1 && args[2].range.maximum() == 0.49);
    }
    auto *md = dynamic_cast<ModemDigital *>(m.get());
    CHECK(md != nullptr);
    csdr_digital_params p = md->csdrDigitalParams();
    CHECK(p.kind == CSDR_DIGITAL_GMSK && p.sps == 4 && p.fdelay == 3 && p.bw == 0.3f);
    for (const char *key : {"fdelay", "sps", "ebf"}) {
        CHECK(!m->shouldRebuildKit());
        m->writeSetting(key, std::strcmp(key, "ebf") ? "16" : "0.25");
        CHECK(m->shouldRebuildKit());                                  // every write asks for a rebuild (ModemGMSK.cpp:70-81)
        m->clearRebuildKit();
    }
    p = md->csdrDigitalParams();
    CHECK(p.sps == 16 && p.fdelay == 16 && p.bw == 0.25f);
    CHECK(m->readSetting("sps") == "16" && m->readSetting("fdelay") == "16" && m->readSetting("ebf") == std::to_string(0.25f));
    if (!g_fail) std::printf("gmsk host test ok\n");
    return g_fail ? 1 : 0;
}

struct TextOutput : ModemDigitalOutput {
    std::string text;
    int writes = 0;
    void write(std::string outp) override { text += outp; ++writes; }
    void write(char outc) override { text += outc; ++writes; }
    void Show() override {}
    void Hide() override {}
    void Close() override {}
};

static int run_gpu(const char *path, int nb, int sw) {
    Modem::registerDigitalLab();
    Modem::registerDigitalGMSK();
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
        auto g = mgr.newThread();
        g->setDemodulatorType("GMSK");
        g->setFrequency(center + 430000);                    // (tests/test_gmsk_host.py: F_GMSK)
        TextOutput out;
        g->setOutput(&out);
        std::thread tp(&IOThread::threadMain, &post);
        for (int b = 0; b < nb; ++b) {
            if (b == sw) g->writeModemSetting("sps", "8");     // a rebuild: a fresh gmskdem, an empty inputBuffer
            auto blk = std::make_shared<SDRThreadIQData>();
            blk->frequency = center; blk->sampleRate = fs; blk->numChannels = 4;
            blk->data.assign(all.begin() + (long)b * block, all.begin() + (long)(b + 1) * block);
            CHECK(in->push(blk));
            while (post.blocksProcessed.load() <= b) std::this_thread::sleep_for(std::chrono::milliseconds(1));
            std::printf("LOCK %d %d\n", b, g->getDemodulatorLock());
            std::printf("TEXTLEN %d %zu\n", b, out.text.size());
        }
        CHECK(post.errlog.errorCount() == 0);
        std::printf("TEXT %s\n", out.text.c_str());
        std::printf("WRITES %d\n", out.writes);
        post.terminate();
        tp.join();
    }
    csdr_ctx_destroy(ctx);
    std::printf(g_fail ? "gmsk host gpu FAILED (%d)\n" : "gmsk host gpu ok\n", g_fail);
    return g_fail ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 4 && !std::strcmp(argv[1], "gpu")) return run_gpu(argv[2], std::atoi(argv[3]), std::atoi(argv[4]));
    if (argc > 1 && !std::strcmp(argv[1], "lab")) return run_lab();
    return run_gmsk();
}
