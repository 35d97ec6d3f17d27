// test_specbank_host.cpp -- DemodSpectrumBank (cubicsdr_amd/host/DemodSpectra.h), driven by tests/test_specbank_host.py.
//   ./test_specbank_host cpu <iq.bin> <plan.txt> <out.bin> <fft_size> <slots> <max_frames>
//        a host bank (no context).  plan.txt, one command per line: "call <slot> <n> <slot> <n> ..." is one process() call whose items take their
//        samples from iq.bin in the order they are named (complex float32), "peak <0|1>" is setPeakHold, "reset <slot>" is resetSlot, "refuse <slot>
//        <n> ..." is a call that must fail with one logged error and change nothing (its samples are not consumed).  Every frame a call produces is
//        appended to out.bin: int32 slot, int32 hold, double fft_ceiling, double fft_floor, 2 * fft_size floats of points, and as many hold points
//        when hold is set.  The Python test compares every frame with its model.
//   ./test_specbank_host gpu <iq.bin> <plan.txt> <fft_size> <slots> <max_frames>
//        the same plan into a device bank and a host bank: every frame of the two within 1e-5 of the frame's largest point.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/DemodSpectra.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

static std::vector<liquid_float_complex_t> slurp(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<liquid_float_complex_t> v(b.size() / sizeof(liquid_float_complex_t));
    std::memcpy(v.data(), b.data(), v.size() * sizeof(liquid_float_complex_t));
    return v;
}

static bool close_enough(const std::vector<float> &a, const std::vector<float> &b) {
    if (a.size() != b.size()) return false;
    float peak = 0.f;
    for (float v : b) if (v == v && std::fabs(v) > peak) peak = std::fabs(v);
    for (size_t i = 0; i < a.size(); ++i) {
        if ((a[i] != a[i]) != (b[i] != b[i])) return false;
        if (a[i] == a[i] && std::fabs(a[i] - b[i]) > 1e-5f * peak) return false;
    }
    return true;
}

static int run(std::vector<DemodSpectrumBank *> banks, const char *iqPath, const char *planPath, const char *outPath, unsigned fft, int slots, int maxFrames) {
    const std::vector<liquid_float_complex_t> all = slurp(iqPath);
    CHECK(!all.empty());
    for (auto *b : banks) {
        CHECK(!b->setup(7, slots, maxFrames) && !b->setup(24, slots, maxFrames) && !b->setup(4096, slots, maxFrames) && !b->setup(fft, 0, maxFrames));
        CHECK(b->errlog.errorCount() == 4);
        CHECK(b->setup(fft, slots, maxFrames));
    }
    std::ofstream out;
    if (outPath) out.open(outPath, std::ios::binary);
    std::ifstream plan(planPath);
    std::string ln;
    size_t next = 0;
    int frames = 0, refused = 0, calls = 0;
    while (std::getline(plan, ln)) {
        std::istringstream is(ln);
        std::string cmd;
        if (!(is >> cmd)) continue;
        if (cmd == "peak") { int on = 0; is >> on; for (auto *b : banks) { b->setPeakHold(on != 0); CHECK(b->getPeakHold() == (on != 0)); } }
        else if (cmd == "reset") { int s = 0; is >> s; for (auto *b : banks) CHECK(b->resetSlot(s)); }
        else if (cmd == "call" || cmd == "refuse") {
            std::vector<DemodSpectrumBank::Item> items;
            size_t at = next;
            int s = 0, n = 0;
            while (is >> s >> n) { items.push_back(DemodSpectrumBank::Item{s, n > 0 ? all.data() + at : nullptr, n}); at += (size_t)(n > 0 ? n : 0); }
            CHECK(at <= all.size());
            if (cmd == "refuse") {
                for (auto *b : banks) { const long long e = b->errlog.errorCount(); CHECK(!b->process(items) && b->errlog.errorCount() == e + 1); }
                ++refused;
                continue;
            }
            next = at;
            ++calls;
            for (auto *b : banks) CHECK(b->process(items));
            for (int slot = 0; slot < slots; ++slot) {
                const int nf = banks[0]->frames(slot);
                for (size_t k = 1; k < banks.size(); ++k) CHECK(banks[k]->frames(slot) == nf);
                for (int j = 0; j < nf; ++j, ++frames) {
                    SpectrumVisualData d0;
                    CHECK(banks[0]->fetch(slot, j, d0) && d0.spectrum_points.size() == (size_t)fft * 2);
                    for (size_t k = 1; k < banks.size(); ++k) {
                        SpectrumVisualData d;
                        CHECK(banks[k]->fetch(slot, j, d));
                        CHECK(close_enough(d.spectrum_points, d0.spectrum_points) && close_enough(d.spectrum_hold_points, d0.spectrum_hold_points));
                        CHECK(std::fabs(d.fft_ceiling - d0.fft_ceiling) <= 1e-5 * std::fabs(d0.fft_ceiling) && std::fabs(d.fft_floor - d0.fft_floor) <= 1e-5 * std::fabs(d0.fft_ceiling));
                    }
                    if (out.is_open()) {
                        const int32_t head[2] = {slot, d0.spectrum_hold_points.empty() ? 0 : 1};
                        out.write((const char *)head, sizeof head);
                        out.write((const char *)&d0.fft_ceiling, sizeof(double));
                        out.write((const char *)&d0.fft_floor, sizeof(double));
                        out.write((const char *)d0.spectrum_points.data(), (std::streamsize)(d0.spectrum_points.size() * sizeof(float)));
                        if (head[1]) out.write((const char *)d0.spectrum_hold_points.data(), (std::streamsize)(d0.spectrum_hold_points.size() * sizeof(float)));
                    }
                }
            }
        } else CHECK(!"unknown command");
    }
    CHECK(next == all.size());
    std::printf("FRAMES %d calls %d refused %d banks %zu\n", frames, calls, refused, banks.size());
    return g_fail;
}

int main(int argc, char **argv) {
    if (argc > 7 && !std::strcmp(argv[1], "cpu")) {
        DemodSpectrumBank host;
        CHECK(!host.onDevice());
        run({&host}, argv[2], argv[3], argv[4], (unsigned)std::atoi(argv[5]), std::atoi(argv[6]), std::atoi(argv[7]));
        std::printf(g_fail ? "specbank host FAILED (%d)\n" : "specbank host test ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    if (argc > 6 && !std::strcmp(argv[1], "gpu")) {
        csdr_ctx *ctx = nullptr;
        csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
        {
            DemodSpectrumBank dev(ctx), host;
            CHECK(dev.onDevice());
            run({&dev, &host}, argv[2], argv[3], nullptr, (unsigned)std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
        }
        csdr_ctx_destroy(ctx);
        std::printf(g_fail ? "specbank host gpu FAILED (%d)\n" : "specbank host gpu ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    std::printf("usage: see the head of this file\n");
    return 2;
}
