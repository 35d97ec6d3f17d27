// test_tracebank_host.cpp -- DemodTraceBank (cubicsdr_amd/host/DemodTraces.h), driven by tests/test_tracebank_host.py.
//   ./test_tracebank_host cpu <floats.bin> <plan.txt> <out.bin>
//        a host bank (no context).  plan.txt, one command per line:
//          "colors <16 bytes>"                                  bg RGBA, line, hold, axis_major, axis_minor RGB
//          "render <width> <height> <atlas_cols> <kind> <n> <layout> <has_hold> ..."    one render; every item takes its floats from floats.bin in the
//                                                                        order named (points, then hold); n 0 is an empty tile.  Appends the picture.
//          "badrender ..."                                               a render that must fail with one logged error
//        The Python test compares out.bin with what tests/trace_oracle.py gives, byte for byte.
//   ./test_tracebank_host gpu <floats.bin> <plan.txt>
//        the same plan into a device bank and a host bank: every picture of the two is the same bytes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/DemodTraces.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

static std::vector<float> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<float> v(b.size() / sizeof(float));
    std::memcpy(v.data(), b.data(), v.size() * sizeof(float));
    return v;
}

static int run(std::vector<DemodTraceBank *> banks, const char *floatsPath, const char *planPath, const char *outPath) {
    const std::vector<float> all = slurp(floatsPath);
    CHECK(!all.empty());
    for (auto *b : banks) {
        CHECK(!b->setup(0, 16) && !b->setup(16, 0) && !b->setup((1 << 20) + 1, 16) && !b->setup(16, (1 << 21) + 1));
        CHECK(b->errlog.errorCount() == 4);
        CHECK(b->setup(16, 1 << 16));
    }
    std::ofstream out;
    if (outPath) out.open(outPath, std::ios::binary);
    std::ifstream plan(planPath);
    std::string ln;
    size_t next = 0;
    int pictures = 0, refused = 0;
    while (std::getline(plan, ln)) {
        std::istringstream is(ln);
        std::string cmd;
        if (!(is >> cmd)) continue;
        if (cmd == "colors") {
            int v[16];
            for (int &x : v) is >> x;
            DemodTraceBank::Colors c;
            for (int k = 0; k < 4; ++k) c.bg[k] = (unsigned char)v[k];
            for (int k = 0; k < 3; ++k) { c.line[k] = (unsigned char)v[4 + k]; c.hold[k] = (unsigned char)v[7 + k]; c.axisMajor[k] = (unsigned char)v[10 + k]; c.axisMinor[k] = (unsigned char)v[13 + k]; }
            for (auto *b : banks) b->setColors(c);
        } else if (cmd == "render" || cmd == "badrender") {
            int w = 0, h = 0, cols = 0, kind = 0, n = 0, layout = 0, hasHold = 0;
            is >> w >> h >> cols;
            std::vector<DemodTraceBank::Item> items;
            while (is >> kind >> n >> layout >> hasHold) {
                const size_t nf = n <= 0 ? 0 : (kind == CSDR_TRACE_SCOPE_XY ? (size_t)n : (size_t)n * (size_t)(layout == 1 ? 2 : 1));
                DemodTraceBank::Item it{kind, nf ? all.data() + next : nullptr, nullptr, n, layout, 0};
                next += nf;
                if (hasHold) { it.hold = all.data() + next; next += nf; }
                items.push_back(it);
            }
            CHECK(next <= all.size());
            std::vector<unsigned char> p0, p;
            if (cmd == "badrender") {
                for (auto *b : banks) { const long long e = b->errlog.errorCount(); CHECK(!b->render(items, w, h, cols, p) && b->errlog.errorCount() == e + 1); }
                ++refused;
                continue;
            }
            CHECK(banks[0]->render(items, w, h, cols, p0));
            for (size_t k = 1; k < banks.size(); ++k) { CHECK(banks[k]->render(items, w, h, cols, p)); CHECK(p == p0); }
            if (out.is_open()) out.write((const char *)p0.data(), (std::streamsize)p0.size());
            ++pictures;
        } else CHECK(!"unknown command");
    }
    CHECK(next == all.size());
    std::printf("DONE pictures %d refused %d banks %zu\n", pictures, refused, banks.size());
    return g_fail;
}

int main(int argc, char **argv) {
    if (argc > 4 && !std::strcmp(argv[1], "cpu")) {
        DemodTraceBank host(nullptr);
        CHECK(!host.onDevice());
        run({&host}, argv[2], argv[3], argv[4]);
        std::printf(g_fail ? "tracebank host FAILED (%d)\n" : "tracebank host test ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    if (argc > 3 && !std::strcmp(argv[1], "gpu")) {
        csdr_ctx *ctx = nullptr;
        csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
        {
            DemodTraceBank dev(ctx), host(nullptr);
            CHECK(dev.onDevice());
            run({&dev, &host}, argv[2], argv[3], nullptr);
        }
        csdr_ctx_destroy(ctx);
        std::printf(g_fail ? "tracebank host gpu FAILED (%d)\n" : "tracebank host gpu ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    std::printf("usage: see the head of this file\n");
    return 2;
}
