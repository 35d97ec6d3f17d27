// test_scopebank_host.cpp -- DemodScopeBank (cubicsdr_amd/host/DemodScopes.h), driven by tests/test_scopebank_host.py.
//   ./test_scopebank_host cpu
//        the header compiles and links against the library; without a context the constructor throws (the mirror has no host arithmetic).
//   ./test_scopebank_host gpu <iq.bin> <slots.txt> <out.bin> <sample_rate> <channels> <block_len> <blocks> <executes> <center> <fft_size>
//        a channelizer and a demodulator bank (slots.txt: one "modem bandwidth frequency" per slot) run <executes> batches of <blocks> blocks cut
//        from iq.bin (complex float32); a DemodScopeBank processes the bank behind every execute.  Every item it then holds is appended to out.bin:
//        int32 execute, slot, frame, which, n_floats, mode, spectrum, channels, inputRate, sampleRate, fft_size, 0; double fft_floor, fft_ceil; the
//        points.  The Python test compares them with the bytes engine.ScopeBank holds for the same executes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/DemodScopes.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "cpu")) {
        bool threw = false;
        try { DemodScopeBank none(nullptr); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
        std::printf(g_fail ? "scopebank host FAILED (%d)\n" : "scopebank host test ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    if (argc > 11 && !std::strcmp(argv[1], "gpu")) {
        const long long fs = std::atoll(argv[5]), center = std::atoll(argv[10]);
        const int M = std::atoi(argv[6]), block = std::atoi(argv[7]), nb = std::atoi(argv[8]), nexec = std::atoi(argv[9]), L = std::atoi(argv[11]);
        std::vector<float> iq;
        {
            std::ifstream f(argv[2], std::ios::binary);
            std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            iq.resize(b.size() / sizeof(float));
            std::memcpy(iq.data(), b.data(), iq.size() * sizeof(float));
        }
        CHECK(iq.size() >= (size_t)2 * nexec * nb * block);
        std::vector<csdr_demod_params> prm;
        {
            std::ifstream f(argv[3]);
            std::string ln;
            while (std::getline(f, ln)) {
                std::istringstream is(ln);
                csdr_demod_params p{};
                long long freq = 0;
                if (!(is >> p.modem >> p.bandwidth >> freq)) continue;
                p.audio_sample_rate = 48000; p.frequency = freq;
                prm.push_back(p);
            }
        }
        CHECK(!prm.empty());
        csdr_ctx *ctx = nullptr;
        csdr_post *post = nullptr;
        csdr_bank *bank = nullptr;
        csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
        csdr_must(csdr_post_create(ctx, &post), "csdr_post_create");
        csdr_must(csdr_post_configure(post, fs, M, CSDR_POST_PFBCH, block, nb), "csdr_post_configure");
        csdr_must(csdr_bank_create(ctx, (int)prm.size(), nb, &bank), "csdr_bank_create");
        for (size_t i = 0; i < prm.size(); ++i) csdr_must(csdr_bank_configure_slot(bank, (int)i, &prm[i], post), "csdr_bank_configure_slot");
        int items = 0;
        {
            DemodScopeBank scopes(ctx);
            CHECK(!scopes.setup(48, (int)prm.size()) && scopes.errlog.errorCount() == 1);
            CHECK(!scopes.process(bank) && scopes.errlog.errorCount() == 2);           // not set up
            CHECK(scopes.setup(L, (int)prm.size()));
            CHECK(!scopes.process(bank) && scopes.errlog.errorCount() == 3);           // no execute yet
            std::ofstream out(argv[4], std::ios::binary);
            for (int e = 0; e < nexec; ++e) {
                csdr_must(csdr_post_execute(post, iq.data() + (size_t)2 * e * nb * block, 0, nb, block, center), "csdr_post_execute");
                csdr_must(csdr_bank_execute(bank, post), "csdr_bank_execute");
                if (e == 2) scopes.setScopeEnabled(false);
                if (e == 3) { scopes.setScopeEnabled(true); scopes.setSpectrumEnabled(false); }
                if (e == 4) scopes.setSpectrumEnabled(true);
                CHECK(scopes.process(bank));
                for (int slot = 0; slot < (int)prm.size(); ++slot)
                    for (int j = 0; j < scopes.frames(slot); ++j)
                        for (int which = 0; which < 2; ++which) {
                            const ScopeRenderData d = scopes.item(slot, j, which);
                            if (d.waveform_points.empty()) continue;          // that half is switched off
                            CHECK(d.spectrum == (which == 1));
                            const int32_t head[12] = {e, slot, j, which, (int32_t)d.waveform_points.size(), (int32_t)d.mode, d.spectrum ? 1 : 0, d.channels,
                                                      d.inputRate, d.sampleRate, d.fft_size, 0};
                            out.write((const char *)head, sizeof head);
                            out.write((const char *)&d.fft_floor, sizeof(double));
                            out.write((const char *)&d.fft_ceil, sizeof(double));
                            out.write((const char *)d.waveform_points.data(), (std::streamsize)(d.waveform_points.size() * sizeof(float)));
                            ++items;
                        }
            }
            CHECK(scopes.errlog.errorCount() == 3);
            CHECK(scopes.item(0, 1, 0).waveform_points.empty() && scopes.errlog.errorCount() == 4);      // max_frames is 1: no such frame
            CHECK(scopes.resetSlot(0) && !scopes.resetSlot((int)prm.size()));
        }
        csdr_bank_destroy(bank);
        csdr_post_destroy(post);
        csdr_ctx_destroy(ctx);
        std::printf("ITEMS %d\n", items);
        std::printf(g_fail ? "scopebank host gpu FAILED (%d)\n" : "scopebank host gpu ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    std::printf("usage: see the head of this file\n");
    return 2;
}
