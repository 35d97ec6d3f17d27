// test_wfbank_host.cpp -- DemodWaterfallBank (cubicsdr_amd/host/DemodWaterfalls.h), driven by tests/test_wfbank_host.py.
//   ./test_wfbank_host cpu <floats.bin> <plan.txt> <out.bin> <fft_size> <lines> <slots> <max_pending>
//        a host bank (no context).  plan.txt, one command per line:
//          "step <slot> <n_floats> <n_lines> ..."    one step call; every item takes n_floats * n_lines floats from floats.bin in the order named,
//                                                    n_floats 0 is a line without points (NULL)
//          "refuse <slot> <n_floats> <n_lines> ..."  a step call that must fail with one logged error and take nothing (its floats are skipped)
//          "update" / "reset <slot>" / "gradient <n_colors>" (3 n floats from floats.bin)
//          "state"                                   appends per slot: int32 lines_buffered, offset 0, offset 1, then both textures where they exist
//          "render <mode> <width> <height> <atlas_cols> <slot> ..."     appends the picture
//          "badrender ..."                           a render that must fail with one logged error
//        The Python test compares out.bin with what its models give, byte for byte.
//   ./test_wfbank_host gpu <floats.bin> <plan.txt> <fft_size> <lines> <slots> <max_pending>
//        the same plan into a device bank and a host bank: every state and every picture of the two are the same bytes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/DemodWaterfalls.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

static std::vector<float> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<float> v(b.size() / sizeof(float));
    std::memcpy(v.data(), b.data(), v.size() * sizeof(float));
    return v;
}

static void put(std::vector<unsigned char> &dst, const void *p, size_t n) { dst.insert(dst.end(), (const unsigned char *)p, (const unsigned char *)p + n); }

static std::vector<unsigned char> state_of(DemodWaterfallBank &b, int slots) {
    std::vector<unsigned char> out, tex;
    for (int s = 0; s < slots; ++s) {
        const int32_t head[3] = {b.getLinesBuffered(s), b.getOffset(s, 0), b.getOffset(s, 1)};
        put(out, head, sizeof head);
        const long long e = b.errlog.errorCount();
        for (int j = 0; j < 2; ++j) {
            if (head[1] >= 0) { CHECK(b.fetchIndex(s, j, tex)); put(out, tex.data(), tex.size()); }
            else CHECK(!b.fetchIndex(s, j, tex));
        }
        CHECK(b.onDevice() ? b.errlog.errorCount() == e + (head[1] >= 0 ? 0 : 2) : b.errlog.errorCount() == e);
    }
    return out;
}

static int run(std::vector<DemodWaterfallBank *> banks, const char *floatsPath, const char *planPath, const char *outPath, unsigned fft, int lines, int slots) {
    const std::vector<float> all = slurp(floatsPath);
    CHECK(!all.empty());
    for (auto *b : banks) {
        CHECK(!b->setup(1, lines, slots) && !b->setup(4097, lines, slots) && !b->setup(fft, 1, slots) && !b->setup(fft, lines, 0) && !b->setup(fft, lines, 4097));
        CHECK(b->errlog.errorCount() == 5);
        CHECK(b->setup(fft, lines, slots));
    }
    std::ofstream out;
    if (outPath) out.open(outPath, std::ios::binary);
    std::ifstream plan(planPath);
    std::string ln;
    size_t next = 0;
    int steps = 0, refused = 0, states = 0, pictures = 0;
    while (std::getline(plan, ln)) {
        std::istringstream is(ln);
        std::string cmd;
        if (!(is >> cmd)) continue;
        if (cmd == "update") { for (auto *b : banks) b->update(); }
        else if (cmd == "reset") { int s = 0; is >> s; for (auto *b : banks) CHECK(b->resetSlot(s)); }
        else if (cmd == "gradient") {
            int n = 0; is >> n;
            std::vector<float> stops(all.begin() + (long)next, all.begin() + (long)(next + 3 * (size_t)n));
            next += 3 * (size_t)n;
            for (auto *b : banks) CHECK(b->setGradient(stops));
        } else if (cmd == "step" || cmd == "refuse") {
            std::vector<DemodWaterfallBank::Item> items;
            size_t at = next;
            int s = 0, nf = 0, nl = 0;
            long long lines_in = 0;
            while (is >> s >> nf >> nl) { items.push_back(DemodWaterfallBank::Item{s, nf > 0 ? all.data() + at : nullptr, nf, nl}); at += (size_t)nf * (size_t)nl; lines_in += nl; }
            CHECK(at <= all.size());
            next = at;
            std::vector<int> t0, t;
            if (cmd == "refuse") {
                for (auto *b : banks) {
                    const long long e = b->errlog.errorCount();
                    CHECK(!b->step(items, &t) && b->errlog.errorCount() == e + 1);
                    for (int v : t) CHECK(v == 0);
                }
                ++refused;
                continue;
            }
            ++steps;
            CHECK(banks[0]->step(items, &t0));
            for (size_t k = 1; k < banks.size(); ++k) { CHECK(banks[k]->step(items, &t)); CHECK(t == t0); }
            if (out.is_open()) { const int32_t n = (int32_t)t0.size(); out.write((const char *)&n, 4); out.write((const char *)t0.data(), (std::streamsize)(t0.size() * sizeof(int))); }
        } else if (cmd == "state") {
            const std::vector<unsigned char> s0 = state_of(*banks[0], slots);
            for (size_t k = 1; k < banks.size(); ++k) CHECK(state_of(*banks[k], slots) == s0);
            if (out.is_open()) out.write((const char *)s0.data(), (std::streamsize)s0.size());
            ++states;
        } else if (cmd == "render" || cmd == "badrender") {
            int mode = 0, w = 0, h = 0, cols = 0, s = 0;
            is >> mode >> w >> h >> cols;
            std::vector<int> list;
            while (is >> s) list.push_back(s);
            std::vector<unsigned char> p0, p;
            if (cmd == "badrender") {
                for (auto *b : banks) { const long long e = b->errlog.errorCount(); CHECK(!b->renderView(list, w, h, mode, cols, p) && b->errlog.errorCount() == e + 1); }
                ++refused;
                continue;
            }
            CHECK(banks[0]->renderView(list, w, h, mode, cols, p0));
            for (size_t k = 1; k < banks.size(); ++k) { CHECK(banks[k]->renderView(list, w, h, mode, cols, p)); CHECK(p == p0); }
            if (out.is_open()) out.write((const char *)p0.data(), (std::streamsize)p0.size());
            ++pictures;
        } else CHECK(!"unknown command");
    }
    CHECK(next == all.size());
    std::printf("DONE steps %d refused %d states %d pictures %d banks %zu\n", steps, refused, states, pictures, banks.size());
    return g_fail;
}

int main(int argc, char **argv) {
    if (argc > 8 && !std::strcmp(argv[1], "cpu")) {
        DemodWaterfallBank host(nullptr, std::atoi(argv[8]));
        CHECK(!host.onDevice());
        run({&host}, argv[2], argv[3], argv[4], (unsigned)std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]));
        std::printf(g_fail ? "wfbank host FAILED (%d)\n" : "wfbank host test ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    if (argc > 7 && !std::strcmp(argv[1], "gpu")) {
        csdr_ctx *ctx = nullptr;
        csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
        {
            DemodWaterfallBank dev(ctx, std::atoi(argv[7])), host(nullptr, std::atoi(argv[7]));
            CHECK(dev.onDevice());
            run({&dev, &host}, argv[2], argv[3], nullptr, (unsigned)std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
        }
        csdr_ctx_destroy(ctx);
        std::printf(g_fail ? "wfbank host gpu FAILED (%d)\n" : "wfbank host gpu ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    std::printf("usage: see the head of this file\n");
    return 2;
}
