// test_table_host.cpp -- the host mirror's table-driven modems (ModemAPSK / ModemSQAM / ModemST of cubicsdr_amd/host/ModemDigital.h, registered by
// Modem::registerDigitalTables with a ConstellationSource), driven by tests/test_table_host.py.
//   ./test_table_host cpu                              : the registry with a formula-built source (names, default rates, settings, opt-in only, the other
//                                                        registration calls unchanged), a failing source
//   ./test_table_host gpu <blocks.bin> <nb> <tables>   : nb blocks of 40000 complex-float samples at 2.4 MS/s, M = 4, through SDRPostThread with an APSK
//                                                        and an ST instance whose points come from the file <tables> (records: int32 name length, name,
//                                                        int32 cons, 2 cons floats); APSK's cons is written to 16 before block 3; prints every block's
//                                                        lock and symbols
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <thread>

#include "../../cubicsdr_amd/host/HipPipeline.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

// constellations of the right shape from formulas (no table of anybody's): APSK as 4 + 12 ... points on rings, SQAM as a grid folded into the four
// quadrants in the order the fold needs, ST as a square grid
static int g_asked = 0;
static bool formula_source(const std::string &name, int cons, std::vector<float> &pts) {
    ++g_asked;
    pts.clear();
    if (name == "APSK") {
        const int inner = cons >= 16 ? 4 : 1, outer = cons - inner;      // two rings: 1 + (cons - 1) or 4 + (cons - 4)
        for (int i = 0; i < inner; ++i) { const double a = 2 * M_PI * i / inner; const double r = inner == 1 ? 0.0 : 0.4; pts.push_back((float)(r * std::cos(a))); pts.push_back((float)(r * std::sin(a))); }
        for (int i = 0; i < outer; ++i) { const double a = 2 * M_PI * i / outer; pts.push_back((float)std::cos(a)); pts.push_back((float)std::sin(a)); }
        return true;
    }
    if (name == "SQAM") {
        const int m = cons / 4;
        std::vector<float> q;
        for (int i = 0; i < m; ++i) { q.push_back(0.1f + 0.2f * (float)(i % 8)); q.push_back(0.1f + 0.2f * (float)(i / 8)); }
        const float sx[4] = {1, 1, -1, -1}, sy[4] = {1, -1, 1, -1};
        for (int k = 0; k < 4; ++k) for (int i = 0; i < m; ++i) { pts.push_back(sx[k] * q[2 * i]); pts.push_back(sy[k] * q[2 * i + 1]); }
        return true;
    }
    if (name == "ST") {
        for (int i = 0; i < cons; ++i) { pts.push_back(-0.75f + 0.5f * (float)(i % 4)); pts.push_back(-0.75f + 0.5f * (float)(i / 4)); }
        return true;
    }
    return false;
}

static int run_cpu() {
    CHECK(Modem::getFactories().size() == 9);                        // registerBuiltins() alone
    Modem::registerDigitalLab();
    Modem::registerDigitalGMSK();
    CHECK(Modem::getFactories().size() == 18);                       // the other two registration calls: what they were
    for (const char *n : {"APSK", "SQAM", "ST"}) CHECK(Modem::getFactories().count(n) == 0 && Modem::makeModem(n) == nullptr);
    // a source that fails registers nothing; one that fails for one name leaves that name out
    CHECK(Modem::registerDigitalTables([](const std::string &, int, std::vector<float> &) { return false; }) == 0);
    CHECK(Modem::registerDigitalTables(ConstellationSource()) == 0);
    CHECK(Modem::getFactories().size() == 18);
    CHECK(Modem::registerDigitalTables([](const std::string &n, int c, std::vector<float> &p) { return n == "ST" && formula_source(n, c, p); }) == 1);
    CHECK(Modem::getFactories().size() == 19 && Modem::getFactories().count("ST") == 1 && Modem::getFactories().count("APSK") == 0);
    // an APSK "table" that is no set of rings is refused by the design: the name stays out
    CHECK(Modem::registerDigitalTables([](const std::string &n, int c, std::vector<float> &p) { return n == "APSK" && formula_source("ST", c, p); }) == 0);
    g_asked = 0;
    CHECK(Modem::registerDigitalTables(formula_source) == 2);
    CHECK(g_asked == 7 + 2);                                         // every table once, up front; ST was there already
    CHECK(Modem::registerDigitalTables(formula_source) == 0 && g_asked == 9);
    auto f = Modem::getFactories();
    CHECK(f.size() == 21);
    for (const char *n : {"APSK", "SQAM", "ST"}) {
        CHECK(f.count(n) == 1 && Modem::getModemDefaultSampleRate(n) == 200000);
        std::unique_ptr<Modem> m(Modem::makeModem(n));
        CHECK(m && m->getName() == n && m->getType() == "digital" && m->csdrModemId() == CSDR_MODEM_DIGITAL && m->getDefaultSampleRate() == 200000);
        CHECK(m->checkSampleRate(100, 48000) == MIN_BANDWIDTH && m->checkSampleRate(200000, 48000) == 200000);
        auto *mt = dynamic_cast<ModemDigitalTableBase *>(m.get());
        CHECK(mt && mt->csdrDigitalParams().kind == CSDR_DIGITAL_TABLE);
    }
    {
        std::unique_ptr<Modem> m(Modem::makeModem("APSK"));
        auto args = m->getSettings();
        CHECK(args.size() == 1 && args[0].key == "cons" && args[0].name == "Constellation" && args[0].description == "Modem Constellation Pattern");
        CHECK(args[0].options == (std::vector<std::string>{"4", "8", "16", "32", "64", "128", "256"}) && args[0].value == "4");
        CHECK(m->readSetting("cons") == "4");
        auto *mt = dynamic_cast<ModemDigitalTableBase *>(m.get());
        const auto &t = mt->csdrTables();
        CHECK(t.size() == 7 && t[0].n_points == 4 && t[6].n_points == 256 && t[2].rule == CSDR_TABLE_RINGS && t[2].n_rings == 2 && t[2].ring_size[0] == 4 && t[2].ring_size[1] == 12);
        CHECK(t[2].sensitivity == 0.005f && t[0].n_rings == 2 && t[0].ring_size[0] == 1 && t[0].ring_radius[0] == 0.0f);
        m->writeSetting("cons", "64");
        CHECK(m->readSetting("cons") == "64" && mt->csdrDigitalCons() == 64 && mt->csdrDigitalParams().cons == 64 && !m->shouldRebuildKit());      // a pointer move, not a rebuild
        m->writeSetting("cons", "48");
        CHECK(m->readSetting("cons") == "48" && mt->csdrDigitalCons() == 64);
        CHECK(&mt->csdrTables() == &dynamic_cast<ModemDigitalTableBase *>(std::unique_ptr<Modem>(Modem::makeModem("APSK")).get())->csdrTables());   // created once, shared
    }
    {
        std::unique_ptr<Modem> m(Modem::makeModem("SQAM"));
        auto args = m->getSettings();
        CHECK(args.size() == 1 && args[0].key == "cons" && args[0].options == (std::vector<std::string>{"32", "128"}) && m->readSetting("cons") == "32");
        auto *mt = dynamic_cast<ModemDigitalTableBase *>(m.get());
        CHECK(mt->csdrTables().size() == 2 && mt->csdrTables()[0].rule == CSDR_TABLE_QUADRANT && mt->csdrTables()[1].n_points == 128);
        m->writeSetting("cons", "128");
        CHECK(mt->csdrDigitalCons() == 128 && !m->shouldRebuildKit());
    }
    {
        std::unique_ptr<Modem> m(Modem::makeModem("ST"));
        CHECK(m->getSettings().empty() && m->readSetting("cons") == "" && m->readSettings().empty());
        auto *mt = dynamic_cast<ModemDigitalTableBase *>(m.get());
        m->writeSetting("cons", "4");
        CHECK(mt->csdrTables().size() == 1 && mt->csdrTables()[0].rule == CSDR_TABLE_NEAREST && mt->csdrTables()[0].n_points == 16 && mt->csdrDigitalCons() == 16);
    }
    {
        DemodulatorMgr mgr(2);
        auto d = mgr.newThread();
        d->setDemodulatorType("APSK");
        CHECK(d->getModemType() == "digital" && d->getBandwidth() == 200000 && d->getDemodulatorLock() == 0);
        d->writeModemSetting("cons", "16");
        CHECK(d->readModemSetting("cons") == "16");
    }
    std::printf(g_fail ? "table host test FAILED (%d)\n" : "table host test ok\n", g_fail);
    return g_fail ? 1 : 0;
}

static std::map<std::pair<std::string, int>, std::vector<float>> g_file;
static bool file_source(const std::string &name, int cons, std::vector<float> &pts) {
    auto it = g_file.find({name, cons});
    if (it == g_file.end()) return false;
    pts = it->second;
    return true;
}

static int run_gpu(const char *path, int nb, const char *tables) {
    {
        std::ifstream ft(tables, std::ios::binary);
        for (;;) {
            int32_t len = 0, cons = 0;
            if (!ft.read((char *)&len, 4) || len < 1 || len > 16) break;
            std::string name((size_t)len, ' ');
            ft.read(&name[0], len);
            ft.read((char *)&cons, 4);
            std::vector<float> p((size_t)2 * cons);
            ft.read((char *)p.data(), (std::streamsize)(p.size() * sizeof(float)));
            if (!ft.good()) break;
            g_file[{name, cons}] = p;
        }
    }
    CHECK(Modem::registerDigitalTables(file_source) == 2);              // APSK and ST; the file holds no SQAM
    CHECK(Modem::makeModem("SQAM") == nullptr);
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
        auto apsk = mgr.newThread();
        apsk->setDemodulatorType("APSK");
        apsk->setFrequency(center + 620000);                 // (tests/test_table_host.py: F_APSK, F_ST)
        auto st = mgr.newThread();
        st->setDemodulatorType("ST");
        st->setFrequency(center - 550000);
        auto vis = std::make_shared<DemodulatorThreadOutputQueue>();
        vis->set_max_num_items(4);
        st->setVisualOutputQueue(vis);
        std::thread tp(&IOThread::threadMain, &post);
        std::vector<uint32_t> sym(1 << 16);
        for (int b = 0; b < nb; ++b) {
            if (b == 3) apsk->writeModemSetting("cons", "16");
            auto blk = std::make_shared<SDRThreadIQData>();
            blk->frequency = center; blk->sampleRate = fs; blk->numChannels = 4;
            blk->data.assign(all.begin() + (long)b * block, all.begin() + (long)(b + 1) * block);
            CHECK(in->push(blk));
            while (post.blocksProcessed.load() <= b) std::this_thread::sleep_for(std::chrono::milliseconds(1));
            std::printf("LOCK %d %d %d\n", b, apsk->getDemodulatorLock(), st->getDemodulatorLock());
            for (auto &d : {apsk, st}) {
                int n = 0;
                CHECK(post.bank() && csdr_bank_fetch_symbols(post.bank(), d->slot(), sym.data(), (int)sym.size(), &n) == CSDR_OK);
                std::printf("SYM %d %d", b, d->slot());
                for (int i = 0; i < n; ++i) std::printf(" %u", sym[i]);
                std::printf("\n");
            }
        }
        AudioThreadInputPtr f;
        int frames = 0;
        while (vis->try_pop(f)) {          // the constellation frame (DemodulatorThread.cpp:256-267)
            ++frames;
            CHECK(f->type == 2 && f->channels == 2 && f->sampleRate == 200000 && !f->data.empty());
        }
        CHECK(frames >= 1);
        CHECK(post.errlog.errorCount() == 0);
        std::printf("SLOTS %d %d\n", apsk->slot(), st->slot());
        post.terminate();
        tp.join();
    }
    csdr_ctx_destroy(ctx);
    std::printf(g_fail ? "table host gpu FAILED (%d)\n" : "table host gpu ok\n", g_fail);
    return g_fail ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc > 4 && !std::strcmp(argv[1], "gpu")) return run_gpu(argv[2], std::atoi(argv[3]), argv[4]);
    return run_cpu();
}
