// test_squelch_host.cpp -- DemodSquelchBank (cubicsdr_amd/host/DemodSquelch.h), driven by tests/test_squelch_host.py.
//   ./test_squelch_host cpu
//        the header compiles and links against the library; without a context the constructor throws (the mirror has no host arithmetic).
//   ./test_squelch_host gpu <iq.bin> <slots.txt> <out.bin> <sample_rate> <channels> <block_len> <blocks> <executes> <center>
//        a channelizer and a demodulator bank (slots.txt: one "modem bandwidth frequency squelch_dB muted option" per slot) run <executes> batches
//        of <blocks> blocks cut from iq.bin (complex float32); a DemodSquelchBank processes the bank behind every execute.  Appended to out.bin per
//        execute and slot: int32 execute, slot, n_items, n_pcm; the items (csdr_squelch_item); the meters (three floats, int32 squelchBreak); the
//        slot's stretch of the recorder's stream (int16, padded to a multiple of four bytes).  The Python test compares them with what
//        engine.SquelchBank holds for the same executes.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/DemodSquelch.h"

static int g_fail = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } } while (0)

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "cpu")) {
        bool threw = false;
        try { DemodSquelchBank none(nullptr, 4, 4); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
        std::printf(g_fail ? "squelch host FAILED (%d)\n" : "squelch host test ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    if (argc > 10 && !std::strcmp(argv[1], "gpu")) {
        const long long fs = std::atoll(argv[5]), center = std::atoll(argv[10]);
        const int M = std::atoi(argv[6]), block = std::atoi(argv[7]), nb = std::atoi(argv[8]), nexec = std::atoi(argv[9]);
        std::vector<float> iq;
        {
            std::ifstream f(argv[2], std::ios::binary);
            std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
            iq.resize(b.size() / sizeof(float));
            std::memcpy(iq.data(), b.data(), iq.size() * sizeof(float));
        }
        CHECK(iq.size() >= (size_t)2 * nexec * nb * block);
        struct Slot { csdr_demod_params prm; float level; int muted, option; };
        std::vector<Slot> slots;
        {
            std::ifstream f(argv[3]);
            std::string ln;
            while (std::getline(f, ln)) {
                std::istringstream is(ln);
                Slot s{};
                long long freq = 0;
                if (!(is >> s.prm.modem >> s.prm.bandwidth >> freq >> s.level >> s.muted >> s.option)) continue;
                s.prm.audio_sample_rate = 48000; s.prm.frequency = freq;
                slots.push_back(s);
            }
        }
        CHECK(!slots.empty());
        const int ns = (int)slots.size();
        csdr_ctx *ctx = nullptr;
        csdr_post *post = nullptr;
        csdr_bank *bank = nullptr;
        csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
        csdr_must(csdr_post_create(ctx, &post), "csdr_post_create");
        csdr_must(csdr_post_configure(post, fs, M, CSDR_POST_PFBCH, block, nb), "csdr_post_configure");
        csdr_must(csdr_bank_create(ctx, ns, nb, &bank), "csdr_bank_create");
        for (int i = 0; i < ns; ++i) csdr_must(csdr_bank_configure_slot(bank, i, &slots[(size_t)i].prm, post), "csdr_bank_configure_slot");
        int records = 0;
        {
            DemodSquelchBank sq(ctx, ns, nb);
            CHECK(!sq.process(bank) && sq.errlog.errorCount() == 1);                                // no execute yet
            CHECK(!sq.setSquelchLevel(ns, -20.0f) && sq.errlog.errorCount() == 2);                  // no such slot
            CHECK(!sq.setSquelchOption(0, 3) && sq.errlog.errorCount() == 3);                       // no such option
            for (int i = 0; i < ns; ++i) {
                CHECK(!sq.isSquelchEnabled(i));
                CHECK(sq.setSquelchLevel(i, slots[(size_t)i].level) && sq.isSquelchEnabled(i));     // setSquelchLevel switches the squelch on
                CHECK(sq.setMuted(i, slots[(size_t)i].muted != 0) && sq.setSquelchOption(i, slots[(size_t)i].option));
                CHECK(sq.getSquelchLevel(i) == slots[(size_t)i].level && sq.isMuted(i) == (slots[(size_t)i].muted != 0));
            }
            std::ofstream out(argv[4], std::ios::binary);
            std::vector<int16_t> pcm;
            std::vector<int64_t> offs;
            for (int e = 0; e < nexec; ++e) {
                csdr_must(csdr_post_execute(post, iq.data() + (size_t)2 * e * nb * block, 0, nb, block, center), "csdr_post_execute");
                csdr_must(csdr_bank_execute(bank, post), "csdr_bank_execute");
                CHECK(sq.process(bank));
                CHECK(sq.record(pcm, offs) && (int)offs.size() == ns + 1);
                for (int slot = 0; slot < ns; ++slot) {
                    const std::vector<csdr_squelch_item> items = sq.items(slot);
                    CHECK((int)items.size() == sq.blocks(slot));
                    float m[3] = {0, 0, 0};
                    bool brk = false;
                    CHECK(sq.meters(slot, m[0], m[1], m[2], brk));
                    const int32_t n_pcm = (int32_t)(offs[(size_t)slot + 1] - offs[(size_t)slot]);
                    const int32_t head[4] = {e, slot, (int32_t)items.size(), n_pcm}, b = brk ? 1 : 0;
                    out.write((const char *)head, sizeof head);
                    out.write((const char *)items.data(), (std::streamsize)(items.size() * sizeof(csdr_squelch_item)));
                    out.write((const char *)m, sizeof m);
                    out.write((const char *)&b, sizeof b);
                    std::vector<int16_t> part(((size_t)n_pcm + 1) & ~(size_t)1, 0);
                    if (n_pcm) std::memcpy(part.data(), pcm.data() + offs[(size_t)slot], (size_t)n_pcm * sizeof(int16_t));
                    out.write((const char *)part.data(), (std::streamsize)(part.size() * sizeof(int16_t)));
                    ++records;
                }
            }
            CHECK(sq.errlog.errorCount() == 3);
            CHECK(sq.resetSlot(0) && !sq.resetSlot(ns));
            float m[3];
            bool brk = true;
            CHECK(sq.meters(0, m[0], m[1], m[2], brk) && m[0] == -100.0f && m[1] == -30.0f && m[2] == 30.0f && !brk);
        }
        csdr_bank_destroy(bank);
        csdr_post_destroy(post);
        csdr_ctx_destroy(ctx);
        std::printf("RECORDS %d\n", records);
        std::printf(g_fail ? "squelch host gpu FAILED (%d)\n" : "squelch host gpu ok\n", g_fail);
        return g_fail ? 1 : 0;
    }
    std::printf("usage: see the head of this file\n");
    return 2;
}
