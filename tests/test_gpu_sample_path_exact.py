"""-m gpu: the channelizers (chan_analyze_p2, chan_analyze_fft, chan_analyze) and every demodulator front-end kernel (demod_frontend_s3 ..
_s6, _s56, _generic, _interp) against float64 restatements of the same operations on the same float32 input, sample by sample.

The parity tests hold this path to 1e-5 of the PEAK of liquid's float32 output (channelizer rows: of the block's strongest channel).  That
passes arithmetic that is subtly wrong: a transform coefficient off by 3e-5 passes it in every case, and so does the resampled IQ behind a
half-band tap off by half a percent (the mutation record below).  Here every output is held to what float32 rounding can explain (tests/util.py derives
the bounds, u = 2^-24; tests/sample_path_oracle.py holds the restatements, built on the taps, phase words and table the library uploads):
  front-end     |y^_j - y_j| <= c_fe u A_j       A_j the absolute-value cascade of output j, c_fe = 4 (0.816 [mixed] + sum sqrt((m_e + 1) / 3) + 2.160)
  channelizer   (a) ||X^ - X||_2 <= u (kappa L ||X||_2 + 1.633 sqrt(M) ||a||_2),   L = log2 M (+ 1 oversampled), kappa = 2 with a chirp-z pass
                (b) |X^_t,k - X_t,k| <= u (4 (kappa L ||v_t||_2 + 1.633 ||a_t||_2) + 4 kappa sum_tones |X_t,k0|)       every row of every frame
Every case asserts through Context.profile() / SDRPost.kernel_name that the kernel it is named for ran and no other front-end variant did.
The reference library (liquid) runs over the same inputs; its ratios to the same bounds are printed beside the kernel's, not asserted.

Worst ratio to the BOUND per kernel, over all cases and inputs (the condition of tests/util.py reads "below 0.5"; `pytest -s` prints the
table of its own run).  The host-thread emulation (tests/emu) executes the same fused multiply-adds: its front-end figures are the device's.
                                          emulation        MI355X           liquid, same inputs and bounds
  demod_frontend_s3 / _s4                 0.041 / 0.051    0.041 / 0.051    1.23 / 0.20
  demod_frontend_s5 / _s6                 0.037 / 0.034    0.037 / 0.034    0.90 / 6.9
  demod_frontend_s56, S = 5 / 6           0.029 / 0.027    0.029 / 0.027    0.92 / 0.68
  demod_frontend_generic, S = 0 / 1       0.261 / 0.138    0.261 / 0.138    0.91 / 1.73          (3.10 and 2.71 u A_j: the bare arm is the furthest from float64)
  demod_frontend_generic, S = 2 / 10      0.039 / 0.033    0.039 / 0.033    0.73 / 0.47
  demod_frontend_interp, S = 0 / 1        0.349 / 0.246    0.349 / 0.246    8.7 / 2.5            (4.15 and 4.81 u A_j)
  chan_analyze_p2           (a) | (b)     0.298 | 0.260    0.298 | 0.260    1.65 | 1.51
  chan_analyze_p2 oversampled             0.288 | 0.315    0.288 | 0.315    1.58 | -
  chan_analyze_fft                        0.363 | 0.294    0.363 | 0.294    2.85 | 2.18
  chan_analyze_fft, chirp-z pass (422)    0.139 | 0.128    0.137 | 0.126    0.26 | 0.42
  chan_analyze_fft oversampled            0.239 | 0.225    0.243 | 0.267    1.11 | -
  chan_analyze (2048)                     0.361 | 0.393    0.361 | 0.393    0.46 | 1.06
  chan_analyze oversampled (6, 1024)      0.437 | 0.395    0.437 | 0.395    0.97 | -
liquid's figures are a record: they hold its first outputs (14 .. 19 u A_j) and its float32 prototype taps, which the product's match to 1e-7
of the peak tap; on a lone sample through the oversampled bank that tap difference alone is 1e6 x (b) (shown as -).
With the spectrum's tone rule (rows above log2 M ||v_t||_2) the oversampled M = 122 bank sat at 0.59 of (b) on a tone halfway between two
centres: the model was corrected (tone rows from 4 ||v_t||_2 on, tests/util.py), the kernel was right.

Mutation record (by hand, host-thread emulation, every case of this module and tests/test_emu_logic.py as it stood before this module; no
mutant is committed).  Each mutant exceeds its bound here:
  outermost tap of the m = 10 half-band stage of the IQ resampler x 1.005 (fill_resamp_cfg)
      here: all 19 front-end cases fail; 8.4e4 u A_j on the first output (0.005 / u: that output is this tap's path alone) against bounds of
      19.6 .. 62.2, 5.5e4 .. 8.4e4 on the lone-sample cases.
      before: every resampled-IQ array passes 1e-5 of its peak, but all 13 front-end tests of the full suite fail behind it: the NBFM
      discriminator turns the first outputs of a stream, 0.5 % off, into audio 1.5e-3 .. 3.1e-3 of the peak (CW: block level and peak, 1.4e-5 .. 6.2e-5).
  sine-table entry 700 moved a tenth of the way to entry 699 (csdr_ctx_create)
      here: fails wherever the oscillator visits the entry: s5 78 .. 98 u A_j (bound 39.1), s3 159 .. 189 (29.8), generic S = 2 186 .. 361 (25.2),
      interpolating 3.7e3 .. 3.9e3 (19.6).
      before: fails 4 of the 13 front-end tests (test_emu_depth_two_cascade with IQ at 3.1e-5 of the peak, mixed modems, both CW tests), passes 9, among
      them the interpolating case that sits at 190 x its bound here.
  one entry of a matrix-pipe coefficient fragment of chan_analyze_p2 x (1 + 3e-5) (chan_mx_table)
      here: noise fails at M = 22 (7.7 x (a)), 62 (1.45 x (b)), 74 (1.95 x (a)), 122 (1.49 x (a)), oversampled 122 (1.74 x (a)); oversampled 38 passes.
      before: passes (the default subset and all 70 channelizer cases of the full suite).
  one entry of the direct prime pass's table, cf_prime_pass_mx, x (1 + 3e-5) (chanfft_direct_mx_tables)
      here: noise fails at M = 116 (1.38 x (a)) and 398 (2.05 x (b)).
      before: passes (the same).
  entry 3 of the M-entry twiddle table of chan_analyze_fft x (1 + 3e-5)
      here: noise fails (a) at 13 of the 16 sizes that run the kernel, 1.37 x (M = 422) .. 14 x (M = 20) the bound; M = 2, 4 and oversampled 8 pass.
      before: passes (the same).
"""
import numpy as np
import pytest

from tests import sample_path_oracle as SP
from tests.util import chan_bin_bound, chan_l2_bound, chan_stages, chan_tone_rows, fe_const, fe_ratio

pytestmark = pytest.mark.gpu

CENTER = 100000000
FE_WORST = {}       # (kernel, S) -> [worst ratio to the bound, worst |e| / (u A), liquid's worst ratio to the bound, outputs]
CH_WORST = {}       # kernel (+ " os2") -> [worst (a), worst (b), liquid's (a), liquid's (b), sizes]


def _backend():
    import oracle.liquid_api as A
    return "ref" if A.available("ref") else "port"


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()
    print_tables()


def print_tables():
    if FE_WORST:
        print("\nfront-end, worst ratio to the bound c_fe u A_j per kernel  (|e| / (u A_j) | c_fe | liquid's ratio to the same bound | outputs):")
        for (k, S), (r, raw, lq, n, c) in sorted(FE_WORST.items()):
            print("  %-24s S = %-2d  %.3f   (%.2f | %.1f | %s | %d)" % (k, S, r, raw, c, "%.3f" % lq if lq >= 0 else "-", n))
    if CH_WORST:
        print("channelizer, worst ratio to the bounds (a) | (b) per kernel  (liquid's | sizes):")
        for k, (ra, rb, la, lb, sizes) in sorted(CH_WORST.items()):
            print("  %-24s %.3f | %.3f   (%s | %s)" % (k, ra, rb, "%.3f | %.3f" % (la, lb) if la >= 0 else "-", ",".join(str(s) for s in sizes)))


# ----------------------------------------------------------------------------------------------- front-end
# name -> (fs, M, channel samples per block of the two batches, [(modem, bandwidth, frequency)], front-end kernels that must run -- and no others)
# Offsets from the channel centre between them: 0, +-1 Hz, both signs in the tens of kHz, 37 500 Hz of 600 kS/s (phase word 2^28: always on a
# table entry), 449 kHz of 600 kS/s (the limit is 0.75 x the rate: routed to the wrap channel M).
FE_CASES = {
    "s56": (2400000, 4, (2501, 2503), [("NBFM", 12500, CENTER + 600000 + 37500), ("AM", 6000, CENTER + 600000 - 23456), ("USB", 5400, CENTER - 600000 + 1),
                                       ("NBFM", 12500, CENTER)], {"demod_frontend_s56"}),
    "s5": (2400000, 4, (2501, 2503), [("NBFM", 12500, CENTER - 1200000 + 20000), ("NBFM", 12500, CENTER + 1200000 + 449000), ("NBFM", 12500, CENTER + 600000 - 1)],
           {"demod_frontend_s5"}),
    "s6": (2400000, 4, (2501, 2503), [("AM", 6000, CENTER - 600000 - 41234), ("USB", 5400, CENTER + 600000 + 77777)], {"demod_frontend_s6"}),
    "s3s4": (600000, 4, (2501, 2503), [("NBFM", 12500, CENTER + 150000 + 12345), ("AM", 6000, CENTER + 150000 - 33333), ("NBFM", 12500, CENTER - 150000)],
             {"demod_frontend_s3", "demod_frontend_s4"}),
    "generic": (2400000, 4, (2501, 2503), [("FM", 200000, CENTER + 600000 + 50000), ("FM", 360000, CENTER - 600000 - 60000)], {"demod_frontend_generic"}),
    "generic-s2": (781250, 8, (2501, 2503), [("NBFM", 12500, CENTER + 97656 + 10000), ("NBFM", 12500, CENTER - 195313 - 1)], {"demod_frontend_generic"}),
    "generic-cw10": (2400000, 4, (10001, 10003), [("CW", 500, CENTER + 600000 - 70000)], {"demod_frontend_generic"}),
    "interp": (2400000, 4, (2501, 2503), [("FM", 800000, CENTER + 600000 + 30000), ("FM", 1500000, CENTER - 600000 - 123457)], {"demod_frontend_interp"}),
    # single-channel mode (M = 1: the channel is the input behind the DC blocker), one demodulator each: a lone sample shows the cascade's own
    # impulse response, every tap of every stage
    "single-s5": (600000, 1, (2501, 2503), [("NBFM", 12500, CENTER + 37500)], {"demod_frontend_s5"}),
    "single-s6": (600000, 1, (2501, 2503), [("AM", 6000, CENTER - 23456)], {"demod_frontend_s6"}),
    "single-generic": (600000, 1, (2501, 2503), [("FM", 200000, CENTER + 50000)], {"demod_frontend_generic"}),
}
ON_TABLE_ENTRY = {("s56", 0), ("single-s5", 0)}        # (case, slot) whose phase increment is a whole multiple of 2^22: every phase on a table entry
FE_RUNS = [(c, s) for c in ("s56", "s5", "s6", "s3s4", "generic", "generic-s2", "generic-cw10", "interp") for s in ("noise", "blocker")] + \
          [(c, "impulse") for c in ("single-s5", "single-s6", "single-generic")]
FE_QUICK = [("s56", "blocker"), ("s5", "noise"), ("s6", "blocker"), ("s3s4", "blocker"), ("generic", "noise"), ("interp", "blocker"), ("single-s5", "impulse")]


def fe_signal(kind, n, fs, M, demods, lens, seed=7):
    """the float32 stream into the channelizer.  noise: white; blocker: per demodulator a tone of 1e-3 inside its band under a blocker 57 dB
    above it, 0.4 channel widths away towards the channel's centre (in the stop band of the narrow demodulators, in the channel); impulse: a lone sample at an irregular index
    of the second block"""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.3).astype(np.complex64)
    if kind == "impulse":
        x = np.zeros(n, np.complex64)
        x[lens[0] * max(M, 1) + 1237] = 0.75 - 0.5j
        return x
    t = np.arange(n, dtype=np.float64) / fs
    x = np.zeros(n, np.complex128)
    chan_bw = fs // M
    for _, bw, f in demods:
        df = f - CENTER
        near = chan_bw * round(df / chan_bw)                     # the demodulator's channel centre, relative to the input's
        away = -0.4 * chan_bw if df - near >= 0 else 0.4 * chan_bw
        x += 1e-3 * np.exp(2j * np.pi * (df + bw / 8.0) * t) + 1e-3 * 10 ** (57 / 20.0) * np.exp(2j * np.pi * (df + away) * t + 1j)
    return x.astype(np.complex64)


def _fe_kernel(plan, kernels):
    S = plan["S"]
    if plan["interp"]:
        return "demod_frontend_interp"
    if 3 <= S <= 6 and plan["m"] == ([10, 5] + [3] * (S - 2)):
        if S >= 5 and "demod_frontend_s56" in kernels:
            return "demod_frontend_s56"
        return "demod_frontend_s%d" % S
    return "demod_frontend_generic"


def check_frontend(ctx, case, signal, liquid=True, quiet=False):
    """two batches of three blocks through SDRPost + DemodBank; every demodulator's resampled IQ against the float64 front-end of the channel
    row the kernel read.  Returns {slot: worst ratio to the bound}."""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    fs, M, lens, demods, kernels = FE_CASES[case]
    nb = 3
    n = nb * sum(lens) * M
    x = fe_signal(signal, n, fs, M, demods, lens)
    post = SDRPost(ctx, fs, M, max(lens) * M, max_blocks=nb)
    bank = DemodBank(ctx, len(demods), max_blocks=nb)
    rows, got = [[] for _ in demods], [[] for _ in demods]
    try:
        for i, (k, bw, f) in enumerate(demods):
            bank.configure(i, post, k, bw, f)
        ctx.profile_enable(True)
        pos = 0
        for bl in lens:
            post.execute(x[pos:pos + nb * bl * M], nb, bl * M, CENTER)
            bank.execute(post)
            pos += nb * bl * M
            for i, (k, bw, f) in enumerate(demods):
                ch = post.channel_at(f)
                rows[i].append(post.read_channel(ch))
                res = bank.results(i)
                assert len(res) == nb and not any(r.skipped for r in res), (case, i)
                iq = bank.iq(i)
                assert iq.size == sum(r.n_iq for r in res), (case, i)
                got[i].append(iq)
        ran = {k for k in ctx.profile() if k.startswith("demod_frontend")}
        ctx.profile_enable(False)
        assert ran == kernels, (case, ran)
        rate = post.channel_rate
        centres = [post.channel_center(post.channel_at(f)) if M > 1 else CENTER for _, _, f in demods]
    finally:
        bank.close(); post.close()
    worst = {}
    for i, (k, bw, f) in enumerate(demods):
        row = np.concatenate(rows[i])
        assert row.size == nb * sum(lens)
        shift = f - centres[i]
        plan = SP.msresamp_plan(float(np.float32(float(bw) / float(rate))))
        if (case, i) in ON_TABLE_ENTRY:
            assert SP.nco_word(shift, rate) % (1 << 22) == 0
        y, A = SP.frontend(row, shift, rate, plan)
        g = np.concatenate(got[i])
        assert g.size == y.size, (case, i, g.size, y.size)                # the closed-form output count of the whole stream
        assert np.all(np.isfinite(g.view(np.float32))), (case, i)
        c = fe_const(plan["m"], shift != 0)
        r = fe_ratio(g, y, A)
        j = int(np.argmax(r))
        name = _fe_kernel(plan, kernels)
        lq = -1.0
        if liquid:
            lq = _liquid_frontend(k, bw, f, rate, centres[i], rows[i], y, A) / c
        w = FE_WORST.setdefault((name, plan["S"]), [0.0, 0.0, -1.0, 0, c])
        w[0], w[1], w[2], w[3] = max(w[0], r[j] / c), max(w[1], r[j]), max(w[2], lq), w[3] + g.size
        if not quiet:
            print("%s / %s, %s %d Hz at %+d Hz (%s, S = %d): worst |e| / (u A) %.2f at output %d of %d, bound %.1f%s"
                  % (case, signal, k, bw, shift, name, plan["S"], r[j], j, g.size, c, ", liquid %.2f" % (lq * c) if liquid else ""))
        assert r[j] <= c, (case, signal, i, "output %d: |e| = %.3g u A_j, bound %.3g" % (j, r[j], c))
        worst[i] = r[j] / c
    return worst


def _liquid_frontend(kind, bw, f, rate, centre, rows, y, A):
    """liquid's own front-end (oscillator + msresamp_crcf of the reference binary) over the same channel rows: its worst |e| / (u A)"""
    from oracle.cubicsdr_chain import RefDemod
    rd = RefDemod(_backend(), kind, bw, f, rate)
    out = np.concatenate([rd.pre(r, centre, rate) for r in rows])
    n = min(out.size, y.size)
    return float(fe_ratio(out[:n], y[:n], A[:n]).max()) if n else 0.0


@pytest.mark.parametrize("case,signal", FE_RUNS)
def test_frontend_against_float64(ctx, case, signal):
    check_frontend(ctx, case, signal)


# ----------------------------------------------------------------------------------------------- channelizers
# (M, frames per block): one M per kernel family and pass structure; three blocks (one call, then a batch of two: the carried history)
CRITICAL = [(2, 150), (4, 131), (10, 130), (14, 70), (22, 77), (62, 67), (74, 80), (122, 70), (20, 77), (36, 70), (52, 40), (68, 30), (92, 33), (116, 21),
            (398, 17), (422, 11), (200, 37), (256, 37), (1024, 19), (2048, 10)]
OVERSAMPLED = [(6, 75), (8, 77), (38, 50), (40, 61), (122, 39), (256, 27), (1024, 10)]
CH_QUICK = {(10, False), (20, False), (122, False), (116, False), (38, True), (40, True)}


def chan_kernel(M, oversampled):
    if oversampled:
        return "chan_analyze_fft" if M % 4 == 0 and M < 1024 else "chan_analyze_p2" if (M // 2) % 2 == 1 and 38 <= M <= 126 else "chan_analyze"
    return "chan_analyze" if M == 2048 else "chan_analyze_p2" if M in (10, 14, 22, 62, 74, 122) else "chan_analyze_fft"


def _irregular(n, frac):
    """an index near frac * n that is neither 0 nor a power of two (n >= 4), else n - 1"""
    if n < 4:
        return n - 1
    k = max(3, int(frac * n)) % n
    while k == 0 or (k & (k - 1)) == 0:
        k = (k + 1) % n
    return k


def chan_inputs(M, n, hop, seed=5):
    """(name, complex64 stream, row whose error is reported relative to its own value or None)"""
    rng = np.random.default_rng(seed + M)
    t = np.arange(n, dtype=np.int64)

    def tone(k2, amp=1.0):
        return amp * np.exp(2j * np.pi * ((k2 * t) % (2 * M)).astype(np.float64) / (2 * M))       # k2 in halves of a channel spacing

    yield "noise", ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * 0.5).astype(np.complex64), None
    frame = (n // hop) // 2 + 1
    for n0 in sorted({_irregular(n, 0.37), frame * hop + hop - 1}):
        x = np.zeros(n, np.complex64)
        x[n0] = 0.75 - 0.5j
        yield "impulse@%d" % n0, x, None
    k0 = _irregular(M, 0.2371)
    for k2 in sorted({2 * k0, 2 * k0 + 1, M}):          # a channel centre, halfway to the next, channel M / 2
        yield "tone@%g" % (k2 / 2), (tone(k2) * (0.6 + 0.3j)).astype(np.complex64), None
    if M >= 4:
        k1, kw = _irregular(M, 0.1234), _irregular(M, 0.6789)
        if abs(kw - k1) < 2:
            kw = (k1 + M // 2) % M
        yield "tones@%d,%d(-100dB)" % (k1, kw), (tone(2 * k1) + tone(2 * kw, 1e-5)).astype(np.complex64), kw


def check_channelizer(ctx, M, frames, oversampled=False, liquid=True, quiet=False):
    """every input of chan_inputs through SDRPost (DC blocker off: row 0 is a row like the others), EVERY row of every frame against the
    float64 bank.  Returns the worst ratios to (a) and (b)."""
    from cubicsdr_amd.engine import SDRPost
    fs, block, nb = 500000 * M, M * frames, 3
    hop = M // 2 if oversampled else M
    kap, L = chan_stages(M, oversampled)
    worst_a = worst_b = liq_a = liq_b = 0.0
    post = SDRPost(ctx, fs, M, block, max_blocks=2, oversampled=oversampled)
    assert post.kernel_name == chan_kernel(M, oversampled), (M, oversampled, post.kernel_name)
    post.close()
    for name, x, weak in chan_inputs(M, nb * block, hop):
        post = SDRPost(ctx, fs, M, block, max_blocks=2, oversampled=oversampled)       # a fresh object per input: an all-zero history
        try:
            post.set_dc_blocker(False)
            post.execute(x[:block], 1, block, CENTER)
            first = np.stack([post.read_channel(ch) for ch in range(M)], axis=1)
            post.execute(x[block:], 2, block, CENTER)
            got = np.concatenate([first, np.stack([post.read_channel(ch) for ch in range(M)], axis=1)]).astype(np.complex128)
        finally:
            post.close()
        X, v, a = SP.firpfbch(x, M, oversampled)
        assert got.shape == X.shape, (M, name, got.shape, X.shape)
        assert np.all(np.isfinite(got)), (M, name)
        ra, rb = _chan_ratios(M, got, X, v, a, L, oversampled)
        worst_a, worst_b = max(worst_a, ra), max(worst_b, rb)
        msg = "M = %d%s %s: (a) %.3f, (b) %.3f of the bound" % (M, " oversampled" if oversampled else "", name, ra, rb)
        if liquid:
            la, lb = _chan_ratios(M, _liquid_channelizer(x, fs, M, block, nb, oversampled), X, v, a, L, oversampled)
            liq_a, liq_b = max(liq_a, la), max(liq_b, lb)
            msg += "; liquid %.3f, %.3f" % (la, lb)
        if weak is not None:
            t = X.shape[0] - 1
            msg += "; the weak tone's row within %.2g of its value" % (abs(got[t, weak] - X[t, weak]) / abs(X[t, weak]))
        if not quiet:
            print(msg)
        assert ra <= 1.0, (M, oversampled, name, "||X^ - X||_2 at %.3g x the bound (a)" % ra)
        assert rb <= 1.0, (M, oversampled, name, "a row at %.3g x the bound (b)" % rb)
    w = CH_WORST.setdefault(chan_kernel(M, oversampled) + (" os2" if oversampled else "") + (" chirp-z" if kap > 1 else ""), [0.0, 0.0, -1.0, -1.0, []])
    w[0], w[1] = max(w[0], worst_a), max(w[1], worst_b)
    if liquid:
        w[2], w[3] = max(w[2], liq_a), max(w[3], liq_b)
    w[4].append(M)
    return worst_a, worst_b


def _chan_ratios(M, got, X, v, a, L, oversampled):
    """ratios of the error to (a) and (b); (b) over every row of every frame but the tones' own (tests.util.chan_tone_rows)"""
    d = np.abs(got - X)
    ra = float(np.linalg.norm(d)) / max(chan_l2_bound(M, X, a, oversampled), 1e-300)
    b = chan_bin_bound(M, v, a, X, oversampled)[:, None]
    d = np.where(chan_tone_rows(v, X), 0.0, d)
    r = np.divide(d, b, out=np.where(d > 0, np.inf, 0.0), where=b > 0)       # (a frame of zeros must come out as zeros)
    return ra, float(r.max())


def _liquid_channelizer(x, fs, M, block, nb, oversampled):
    from oracle.cubicsdr_chain import RefSDRPost
    ref = RefSDRPost(_backend(), fs, M, oversampled=oversampled)
    out = []
    for b in range(nb):
        ref.run_block(x[b * block:(b + 1) * block], CENTER)
        out.append(ref.data_out.reshape(-1, M).astype(np.complex128))
    return np.concatenate(out)


@pytest.mark.parametrize("M,frames", CRITICAL)
def test_channelizer_against_float64(ctx, M, frames):
    check_channelizer(ctx, M, frames)


@pytest.mark.parametrize("M,frames", OVERSAMPLED)
def test_oversampled_channelizer_against_float64(ctx, M, frames):
    check_channelizer(ctx, M, frames, oversampled=True)
