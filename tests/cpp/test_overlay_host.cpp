// test_overlay_host.cpp -- DemodOverlayBank (cubicsdr_amd/host/DemodOverlays.h), driven by tests/test_overlay_host.py.
//   ./test_overlay_host cpu <bytes.bin> <plan.txt> <out.bin>
//        a host bank (no context).  plan.txt, one command per line; bytes.bin is consumed in the order named:
//          "font <w> <h>"                       the next w * h bytes are the coverage plane; "font 0 0" removes it
//          "glyphs <n> <8 ints> ..."            the glyph table of the text commands
//          "text <x> <y> <halign> <valign> <mode> <r> <g> <b> <a> <line_height> <string>"    csdr_design_text; appends the primitives (32 bytes each)
//          "compose <W> <H> <cols> <has_base> <n_tiles> <first count> ... <n_prims> <x y w h r g b a mode mask_x mask_y> ..."
//                                               one compose; with has_base the next rows * H * cols * W * 4 bytes are the base.  Appends the picture.
//          "badcompose ..."                     a compose that must fail with one logged error
//        The Python test compares out.bin with what tests/overlay_oracle.py gives, byte for byte.
//   ./test_overlay_host gpu <bytes.bin> <plan.txt>
//        the same plan into a device bank and a host bank: every picture of the two is the same bytes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/DemodOverlays.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

static std::vector<unsigned char> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int run(std::vector<DemodOverlayBank *> banks, const char *bytesPath, const char *planPath, const char *outPath) {
    const std::vector<unsigned char> all = slurp(bytesPath);
    CHECK(!all.empty());
    for (auto *b : banks) {
        CHECK(!b->setup(0, 16) && !b->setup(16, 0) && !b->setup((1 << 20) + 1, 16) && !b->setup(16, (1 << 22) + 1));
        CHECK(b->errlog.errorCount() == 4);
        CHECK(b->setup(16, 2048));
    }
    std::ofstream out;
    if (outPath) out.open(outPath, std::ios::binary);
    std::ifstream plan(planPath);
    std::string ln;
    size_t next = 0;
    int pictures = 0, refused = 0, texts = 0;
    std::vector<csdr_glyph> glyphs;
    while (std::getline(plan, ln)) {
        std::istringstream is(ln);
        std::string cmd;
        if (!(is >> cmd)) continue;
        if (cmd == "font") {
            int w = 0, h = 0;
            is >> w >> h;
            const size_t nb = (size_t)w * (size_t)h;
            CHECK(next + nb <= all.size());
            for (auto *b : banks) CHECK(b->setFont(nb ? all.data() + next : nullptr, w, h));
            next += nb;
        } else if (cmd == "glyphs") {
            int n = 0;
            is >> n;
            glyphs.assign((size_t)n, csdr_glyph{});
            for (auto &g : glyphs) is >> g.id >> g.x >> g.y >> g.w >> g.h >> g.xoffset >> g.yoffset >> g.xadvance;
        } else if (cmd == "text") {
            int x, y, ha, va, mode, c[4], lh;
            is >> x >> y >> ha >> va >> mode >> c[0] >> c[1] >> c[2] >> c[3] >> lh;
            std::string s;
            std::getline(is, s);
            if (!s.empty()) s.erase(0, 1);               // the one separating blank
            const unsigned char rgba[4] = {(unsigned char)c[0], (unsigned char)c[1], (unsigned char)c[2], (unsigned char)c[3]};
            std::vector<csdr_overlay_prim> prims;
            CHECK(banks[0]->text(glyphs, lh, s, x, y, ha, va, rgba, mode, prims));
            if (out.is_open() && !prims.empty()) out.write((const char *)prims.data(), (std::streamsize)(prims.size() * sizeof(csdr_overlay_prim)));
            ++texts;
        } else if (cmd == "compose" || cmd == "badcompose") {
            int w = 0, h = 0, cols = 0, hasBase = 0, nTiles = 0, nPrims = 0;
            is >> w >> h >> cols >> hasBase >> nTiles;
            std::vector<csdr_overlay_tile> tiles((size_t)std::max(nTiles, 0));
            for (auto &t : tiles) is >> t.first >> t.count;
            is >> nPrims;
            std::vector<csdr_overlay_prim> prims((size_t)std::max(nPrims, 0));
            for (auto &q : prims) {
                int c[4];
                is >> q.x >> q.y >> q.w >> q.h >> c[0] >> c[1] >> c[2] >> c[3] >> q.mode >> q.mask_x >> q.mask_y;
                for (int k = 0; k < 4; ++k) q.rgba[k] = (unsigned char)c[k];
            }
            CHECK(!is.fail());
            const unsigned char *base = nullptr;
            if (hasBase) {
                const size_t nb = cols > 0 ? (size_t)((nTiles + cols - 1) / cols) * (size_t)h * (size_t)cols * (size_t)w * 4 : 0;
                CHECK(next + nb <= all.size());
                base = all.data() + next;
                next += nb;
            }
            std::vector<unsigned char> p0, p;
            if (cmd == "badcompose") {
                for (auto *b : banks) { const long long e = b->errlog.errorCount(); CHECK(!b->compose(base, false, tiles, prims, w, h, cols, p) && b->errlog.errorCount() == e + 1); }
                ++refused;
                continue;
            }
            CHECK(banks[0]->compose(base, false, tiles, prims, w, h, cols, p0));
            for (size_t k = 1; k < banks.size(); ++k) { CHECK(banks[k]->compose(base, false, tiles, prims, w, h, cols, p)); CHECK(p == p0); }
            if (out.is_open()) out.write((const char *)p0.data(), (std::streamsize)p0.size());
            ++pictures;
        } else CHECK(!"unknown command");
    }
    CHECK(next == all.size());
    std::printf("DONE pictures %d refused %d texts %d banks %zu\n", pictures, refused, texts, banks.size());
    return g_fail;
}

int main(int argc, char **argv) {
    if (argc > 4 && !std::strcmp(argv[1], "cpu")) {
        DemodOverlayBank host(nullptr);
        CHECK(!host.onDevice());
        run({&host}, argv[2], argv[3], argv[4]);
        std::printf(g_fail ? "overlay host FAILED (%d)\n" : "overlay host test ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    if (argc > 3 && !std::strcmp(argv[1], "gpu")) {
        csdr_ctx *ctx = nullptr;
        csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
        {
            DemodOverlayBank dev(ctx), host(nullptr);
            CHECK(dev.onDevice());
            run({&dev, &host}, argv[2], argv[3], nullptr);
        }
        csdr_ctx_destroy(ctx);
        std::printf(g_fail ? "overlay host gpu FAILED (%d)\n" : "overlay host gpu ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    std::printf("usage: see the head of this file\n");
    return 2;
}
