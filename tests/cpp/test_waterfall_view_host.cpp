// test_waterfall_view_host.cpp -- WaterfallPanel::renderView (cubicsdr_amd/host/WaterfallPanel.h), driven by tests/test_waterfall_view_host.py.
//   ./test_waterfall_view_host cpu <lines.bin> <plan.txt> <out_prefix> <fft_size> <lines>
//        a host panel (no context).  plan.txt, one command per line: "feed <n>" steps the next n lines of lines.bin (fft_size floats each) and
//        updates, "grad <r g b ...>" sets the gradient, "view <width> <height> <mode>" renders a view into <out_prefix>.<k>.rgba (k counts the views),
//        "refuse <width> <height> <mode>" expects renderView to fail with one logged error.  The Python test compares every picture with its
//        numpy model.
//   ./test_waterfall_view_host gpu <lines.bin> <plan.txt> <fft_size> <lines>
//        the same plan into a device panel and a host panel: every view must be the same bytes in both.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/WaterfallPanel.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

static std::vector<float> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<float> v(b.size() / sizeof(float));
    std::memcpy(v.data(), b.data(), v.size() * sizeof(float));
    return v;
}

static int run(std::vector<WaterfallPanel *> panels, const char *linesPath, const char *planPath, const std::string &prefix, unsigned fft, int lines) {
    const std::vector<float> all = slurp(linesPath);
    CHECK(!all.empty() && all.size() % fft == 0);
    for (auto *p : panels) {
        p->setup(fft, lines);
        std::vector<unsigned char> none(3, 7);
        CHECK(!p->renderView(16, 3, CSDR_WF_VIEW_PEAK, none));       // no textures yet
        p->step(); p->update();                                      // (the first step is dropped; the update makes the textures)
    }
    std::ifstream plan(planPath);
    std::string ln;
    size_t next = 0;
    int views = 0, refused = 0;
    while (std::getline(plan, ln)) {
        std::istringstream is(ln);
        std::string cmd;
        if (!(is >> cmd)) continue;
        if (cmd == "feed") {
            int n = 0;
            is >> n;
            CHECK(next + (size_t)n <= all.size() / fft);
            for (int k = 0; k < n; ++k, ++next) {
                std::vector<float> pts(all.begin() + next * fft, all.begin() + (next + 1) * fft);
                for (auto *p : panels) { p->setPoints(pts); p->step(); }
            }
            for (auto *p : panels) p->update();
        } else if (cmd == "grad") {
            std::vector<float> stops;
            float c;
            while (is >> c) stops.push_back(c);
            for (auto *p : panels) CHECK(p->setGradient(stops));
        } else if (cmd == "view" || cmd == "refuse") {
            int w = 0, h = 0, mode = 0;
            is >> w >> h >> mode;
            std::vector<unsigned char> first;
            for (size_t k = 0; k < panels.size(); ++k) {
                std::vector<unsigned char> pic;
                const size_t errors = panels[k]->errlog.errorCount();
                const bool ok = panels[k]->renderView(w, h, mode, pic);
                if (cmd == "refuse") { CHECK(!ok && panels[k]->errlog.errorCount() == errors + 1); continue; }
                CHECK(ok && pic.size() == (size_t)w * h * 4);
                if (k == 0) first = pic; else CHECK(pic == first);
            }
            if (cmd == "refuse") { ++refused; continue; }
            if (!prefix.empty()) std::ofstream(prefix + "." + std::to_string(views) + ".rgba", std::ios::binary).write((const char *)first.data(), (std::streamsize)first.size());
            ++views;
        } else CHECK(!"unknown command");
    }
    for (size_t k = 1; k < panels.size(); ++k) CHECK(panels[k]->getOffset(0) == panels[0]->getOffset(0));
    std::printf("VIEWS %d refused %d offset %d panels %zu\n", views, refused, panels[0]->getOffset(0), panels.size());
    return g_fail;
}

int main(int argc, char **argv) {
    if (argc > 6 && !std::strcmp(argv[1], "cpu")) {
        WaterfallPanel host;
        CHECK(!host.onDevice());
        run({&host}, argv[2], argv[3], argv[4], (unsigned)std::atoi(argv[5]), std::atoi(argv[6]));
        std::printf(g_fail ? "waterfall view host FAILED (%d)\n" : "waterfall view host test ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    if (argc > 5 && !std::strcmp(argv[1], "gpu")) {
        csdr_ctx *ctx = nullptr;
        csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
        {
            WaterfallPanel dev(ctx, 64), host;
            CHECK(dev.onDevice());
            run({&dev, &host}, argv[2], argv[3], "", (unsigned)std::atoi(argv[4]), std::atoi(argv[5]));
        }
        csdr_ctx_destroy(ctx);
        std::printf(g_fail ? "waterfall view host gpu FAILED (%d)\n" : "waterfall view host gpu ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    std::printf("usage: see the head of this file\n");
    return 2;
}
