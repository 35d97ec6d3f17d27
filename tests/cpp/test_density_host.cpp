// test_density_host.cpp -- cubicsdr_amd/host/DemodDensity.h (DemodDensityBank) compiled with g++ -Wall against libcsdr_hip.so.
//   cpu                          the constructor throws without a context; csdr_design_density_cover gives the header's example without a device
//   pipe iq slots out fs M block blocks executes center F W H
//                                DemodDensityBanks behind a running pipeline (run_pipe below): stepSpectrumBank and stepSpectrum, frames in HBM only
//   gpu floats plan out          a DemodDensityBank runs the plan tests/test_density_host.py wrote and writes every fetched grid, peak and picture
// Plan lines:  setup W H slots max_frames max_points | palette <offset of 1024 floats holding bytes> | step n_items {slot offset n frames stride
// layout kind keep weight}*  (offset -1: no points) | fetch slot | render cols n_views {slot full}*
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>

#include "../../cubicsdr_amd/host/DemodDensity.h"

static std::vector<float> read_floats(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<float> v(raw.size() / sizeof(float));
    std::memcpy(v.data(), raw.data(), v.size() * sizeof(float));
    return v;
}

static int run_cpu() {
    bool threw = false;
    try { DemodDensityBank none(nullptr); } catch (const std::invalid_argument &) { threw = true; }
    if (!threw) { std::printf("no exception without a context\n"); return 1; }
    const float y[3] = {0.95f, 0.05f, 0.95f};
    const int lo[7] = {0, 2, 7, 2, 0, 1, 1}, hi[7] = {2, 7, 9, 7, 2, 0, 0};
    uint32_t cover[10 * 7];
    csdr_must(csdr_design_density_cover(y, 3, 0, 3, 1, CSDR_TRACE_SPECTRUM, 7, 10, cover), "csdr_design_density_cover");
    for (int r = 0; r < 10; ++r)
        for (int c = 0; c < 7; ++c)
            if (cover[r * 7 + c] != (uint32_t)(r >= lo[c] && r <= hi[c])) { std::printf("cover[%d][%d] = %u\n", r, c, cover[r * 7 + c]); return 1; }
    std::printf("density host test ok\n");
    return 0;
}

static int run_gpu(const char *p_floats, const char *p_plan, const char *p_out) {
    const std::vector<float> floats = read_floats(p_floats);
    std::ifstream plan(p_plan);
    std::ofstream out(p_out, std::ios::binary);
    csdr_ctx *ctx = nullptr;
    csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
    int steps = 0, fetched = 0, pictures = 0;
    {
        DemodDensityBank bank(ctx);
        std::string line;
        while (std::getline(plan, line)) {
            std::istringstream in(line);
            std::string what;
            in >> what;
            bool ok = true;
            if (what == "setup") {
                int W, H, slots, mf, mp;
                in >> W >> H >> slots >> mf >> mp;
                ok = bank.setup(W, H, slots, mf, mp);
            } else if (what == "palette") {
                long long off;
                in >> off;
                unsigned char pal[1024];
                for (int i = 0; i < 1024; ++i) pal[i] = (unsigned char)floats[(size_t)off + i];
                ok = bank.setPalette(pal);
            } else if (what == "step") {
                int n;
                in >> n;
                std::vector<DemodDensityBank::Item> items((size_t)n);
                for (auto &it : items) {
                    long long off;
                    in >> it.slot >> off >> it.n >> it.frames >> it.strideFloats >> it.layout >> it.kind >> it.keepQ16 >> it.weight;
                    it.points = off < 0 ? nullptr : floats.data() + off;
                    it.isDev = 0;
                }
                ok = bank.step(items);
                ++steps;
            } else if (what == "fetch") {
                int slot;
                in >> slot;
                std::vector<uint32_t> grid;
                unsigned pk = 0;
                ok = bank.fetch(slot, grid) && bank.peak(slot, pk);
                out.write(reinterpret_cast<const char *>(grid.data()), (std::streamsize)(grid.size() * sizeof(uint32_t)));
                const uint32_t p32 = pk;
                out.write(reinterpret_cast<const char *>(&p32), sizeof p32);
                ++fetched;
            } else if (what == "render") {
                int cols, n;
                in >> cols >> n;
                std::vector<DemodDensityBank::View> views((size_t)n);
                for (auto &v : views) in >> v.slot >> v.full;
                std::vector<unsigned char> pic;
                ok = bank.render(views, cols, pic);
                out.write(reinterpret_cast<const char *>(pic.data()), (std::streamsize)pic.size());
                ++pictures;
            } else if (!what.empty()) ok = false;
            if (!ok) { std::printf("FAILED %s: %s\n", line.c_str(), bank.errlog.lastError().c_str()); return 1; }
        }
        // a refused step is logged, not thrown
        if (bank.step({DemodDensityBank::Item{0, nullptr, 0, 0, 0, 0, 7, 0, 65536u, 1u}}) || bank.errlog.errorCount() != 1) { std::printf("a bad kind was not refused\n"); return 1; }
    }
    csdr_ctx_destroy(ctx);
    std::printf("DONE steps %d fetched %d pictures %d\n", steps, fetched, pictures);
    std::printf("density host gpu ok\n");
    return 0;
}

// A channelizer and a demodulator bank (slots.txt: one "modem bandwidth frequency" per slot) run <executes> batches of <blocks> blocks cut from
// iq.bin.  Behind every execute a csdr_specbank processes the bank and a DemodDensityBank of one slot per demodulator steps through
// stepSpectrumBank; a csdr_spec with hideDC on processes the same wideband samples, every frame, and a second DemodDensityBank of one slot steps
// through stepSpectrum.  Nothing but the fetched grids crosses the link.  After every execute every grid and peak is appended to out, at the end
// the two pictures.
static int run_pipe(char **argv) {
    const long long fs = std::atoll(argv[5]), center = std::atoll(argv[10]);
    const int M = std::atoi(argv[6]), block = std::atoi(argv[7]), nb = std::atoi(argv[8]), nexec = std::atoi(argv[9]), F = std::atoi(argv[11]);
    const int W = std::atoi(argv[12]), H = std::atoi(argv[13]);
    const std::vector<float> iq = read_floats(argv[2]);
    if (iq.size() < (size_t)2 * nexec * nb * block) { std::printf("iq.bin is too short\n"); return 1; }
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
    const int slots = (int)prm.size();
    std::ofstream out(argv[4], std::ios::binary);
    csdr_ctx *ctx = nullptr;
    csdr_post *post = nullptr;
    csdr_bank *bank = nullptr;
    csdr_specbank *sb = nullptr;
    csdr_spec *spec = nullptr;
    csdr_must(csdr_ctx_create(0, nullptr, &ctx), "csdr_ctx_create");
    csdr_must(csdr_post_create(ctx, &post), "csdr_post_create");
    csdr_must(csdr_post_configure(post, fs, M, CSDR_POST_PFBCH, block, nb), "csdr_post_configure");
    csdr_must(csdr_bank_create(ctx, slots, nb, &bank), "csdr_bank_create");
    for (int i = 0; i < slots; ++i) csdr_must(csdr_bank_configure_slot(bank, i, &prm[(size_t)i], post), "csdr_bank_configure_slot");
    csdr_must(csdr_specbank_create(ctx, &sb), "csdr_specbank_create");
    csdr_must(csdr_specbank_setup(sb, F, slots, 64), "csdr_specbank_setup");
    const int wide_frames = nb * (block / (2 * F)) + 2;
    csdr_must(csdr_spec_create(ctx, &spec), "csdr_spec_create");
    csdr_must(csdr_spec_setup(spec, F, wide_frames), "csdr_spec_setup");
    csdr_must(csdr_spec_set_hide_dc(spec, 1), "csdr_spec_set_hide_dc");
    csdr_must(csdr_spec_set_center_frequency(spec, center), "csdr_spec_set_center_frequency");
    csdr_must(csdr_spec_set_bandwidth(spec, fs), "csdr_spec_set_bandwidth");
    csdr_must(csdr_spec_set_input_frequency(spec, center), "csdr_spec_set_input_frequency");
    int grids = 0, fail = 0;
    {
        DemodDensityBank banks(ctx), wide(ctx);
        if (banks.stepSpectrumBank(sb, 65536u, 1u) || banks.errlog.errorCount() != 1) { std::printf("a step before setup was not refused\n"); ++fail; }
        if (!banks.setup(W, H, slots, 64, F) || !wide.setup(W, H, 1, wide_frames, F)) { std::printf("setup: %s\n", banks.errlog.lastError().c_str()); ++fail; }
        auto put = [&](DemodDensityBank &b, int slot) {
            std::vector<uint32_t> grid;
            unsigned pk = 0;
            if (!b.fetch(slot, grid) || !b.peak(slot, pk)) { std::printf("fetch: %s\n", b.errlog.lastError().c_str()); ++fail; }
            const uint32_t p32 = pk;
            out.write(reinterpret_cast<const char *>(grid.data()), (std::streamsize)(grid.size() * sizeof(uint32_t)));
            out.write(reinterpret_cast<const char *>(&p32), sizeof p32);
            ++grids;
        };
        for (int e = 0; e < nexec && !fail; ++e) {
            const float *x = iq.data() + (size_t)2 * e * nb * block;
            csdr_must(csdr_post_execute(post, x, 0, nb, block, center), "csdr_post_execute");
            csdr_must(csdr_bank_execute(bank, post), "csdr_bank_execute");
            csdr_must(csdr_specbank_process_bank(sb, bank), "csdr_specbank_process_bank");
            if (!banks.stepSpectrumBank(sb, 60000u, 3u)) { std::printf("stepSpectrumBank: %s\n", banks.errlog.lastError().c_str()); ++fail; }
            csdr_must(csdr_spec_process(spec, x, 0, nb, block, CSDR_SPEC_CONTIGUOUS), "csdr_spec_process");
            const int nf = csdr_spec_frames(spec);
            if (!wide.stepSpectrum(0, spec, 1, nf - 1, 62000u, 2u)) { std::printf("stepSpectrum: %s\n", wide.errlog.lastError().c_str()); ++fail; }
            if (wide.stepSpectrum(0, spec, 1, nf, 62000u, 2u) || wide.errlog.errorCount() != 1 + e) { std::printf("frames outside the process were not refused\n"); ++fail; }
            for (int s = 0; s < slots; ++s) put(banks, s);
            put(wide, 0);
        }
        std::vector<DemodDensityBank::View> views;
        for (int s = 0; s < slots; ++s) views.push_back(DemodDensityBank::View{s, 0u});
        std::vector<unsigned char> pic;
        if (!banks.render(views, 2, pic)) ++fail;
        out.write(reinterpret_cast<const char *>(pic.data()), (std::streamsize)pic.size());
        if (!wide.render({DemodDensityBank::View{0, 40u}}, 1, pic)) ++fail;
        out.write(reinterpret_cast<const char *>(pic.data()), (std::streamsize)pic.size());
    }
    csdr_spec_destroy(spec);
    csdr_specbank_destroy(sb);
    csdr_bank_destroy(bank);
    csdr_post_destroy(post);
    csdr_ctx_destroy(ctx);
    std::printf("GRIDS %d\n", grids);
    std::printf(fail ? "density host pipe FAILED (%d)\n" : "density host pipe ok\n", fail);
    return fail ? 1 : 0;
}

int main(int argc, char **argv) {
    try {
        if (argc > 1 && !std::strcmp(argv[1], "cpu")) return run_cpu();
        if (argc > 13 && !std::strcmp(argv[1], "pipe")) return run_pipe(argv);
        if (argc > 4 && !std::strcmp(argv[1], "gpu")) return run_gpu(argv[2], argv[3], argv[4]);
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("usage: test_density_host cpu | gpu floats plan out\n");
    return 2;
}
