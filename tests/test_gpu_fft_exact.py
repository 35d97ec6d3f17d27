"""-m gpu: every transform plan of csdr_spec (SpectrumProcessor.fft_only) against a float64 DFT of the same float32 input, bin by bin.

test_fft_matches_liquid holds the transform to 1e-5 of its PEAK bin: on its carrier-over-noise signal that passes an error of 1 % of a
median bin, and with it a wrong twiddle entry.  Here each plan is held to what float32 rounding can explain (tests/util.py derives the
two bounds, u = 2^-24, N_eff = N, or the convolution length L of a chirp-z transform):
  (a)  ||X^ - X||_2 / ||X||_2       <= c2    u log2 N_eff          c2 = 1,    x 2 for chirp-z
  (b)  max_k |X^_k - X_k|            <= u (c_inf log2 N_eff ||x||_2 + c_tone sum_t |X_kt|)   c_inf = c_tone = 4, x 2 for chirp-z
on complex white noise, impulses at an irregular position and at N - 1 (no tone term: every bin held to a few u log2 N of ||x||_2),
tones exactly on bin 0, N / 2, N - 1 and an irregular bin (every bin but k0 held to (b), as |X^_k - X_k| and as |X^_k|), and two tones
100 dB apart (the weak tone's bin held to (b), which is a few % of its own value at N = 4 and 1e-4 of it at N = 2^22).

Worst ratio to the bound per plan, MI355X (max over the inputs and sizes of the plan; (a) | (b)); the host-thread emulation of the same
sources (tests/emu) gives the same figures:
  spec_fft_small                 N = 4 .. 2048                     0.290 | 0.315
  spec_fft_rows4096              N = 4096                          0.286 | 0.165
  radix 2 / 4 / 8 / 16 + rows    N = 8192 .. 65536                 0.284 | 0.224
  radix 32 + rows                N = 2^17                          0.237 | 0.185
  Ra x Rb + rows                 N = 2^18 .. 2^20, 2^22            0.232 | 0.258
  spec_cols512 + rows            N = 2^21                          0.262 | 0.203
  chirp-z in LDS                 fftSize 3, 5, 37, 1023            0.228 | 0.096
  chirp-z, power-of-two chains   fftSize 1025, 12345 .. 1048575    0.201 | 0.188
A copied entry of the fine twiddle table (lo[700] = lo[699] in csdr_spec_setup) fails (a) on noise at 21, 12.5 and 3.0 x the bound at
fftSize 8192, 16384 and 65536, where test_fft_matches_liquid still passes.

Display points (test_spectrum_display_points_against_float64), worst ratio of |point - exact point| to DisplayBound, MI355X:
  spec_fft_small 0.247, radix 8 0.107, fused 2^17 chain 0.116, Ra x Rb 0.121, spec_cols512 0.107, chirp-z in LDS 0.210, chirp-z chains 0.105.
The fused chain sits as close to float64 as the other plans; one wrong entry of its W512 table (s_w of spec_cols512p) puts a point at 11 x
its bound.
(the module prints the table of its own run at the end, `pytest -s`).
"""
import math

import numpy as np
import pytest

from tests.util import U32, fft_bin_bound, fft_bin_err, fft_l2_bound, fft_l2_err, fft_n_eff

pytestmark = pytest.mark.gpu


def fft_plan(fft_size):
    """the plan csdr_spec_setup / spec_run_fft picks for fft_only at this fftSize (N = 2 fftSize)"""
    N = 2 * fft_size
    if N & (N - 1):
        L, _ = fft_n_eff(fft_size)
        return "chirp-z in LDS" if L <= 4096 else "chirp-z, power-of-two chains"
    if N <= 2048:
        return "spec_fft_small"
    if N == 4096:
        return "spec_fft_rows4096"
    if N <= 1 << 16:
        return "radix %d + rows" % (N // 4096)
    if N == 1 << 17:
        return "radix 32 + rows"
    if N == 1 << 21:
        return "spec_cols512 + rows"
    return "Ra x Rb + rows"


POW2 = [1 << k for k in range(1, 22)]
NPOT = [3, 5, 37, 1023, 1025, 12345, 100001, 1048575]
SIZES = POW2 + NPOT

WORST = {}          # plan -> [worst (a) ratio, worst (b) ratio, sizes]


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()
    if WORST:
        print("\nworst ratio to the bound per plan ((a) relative L2 | (b) per bin):")
        for plan, (ra, rb, sizes) in WORST.items():
            print("  %-30s %-40s %.3f | %.3f" % (plan, ",".join(str(s) for s in sizes), ra, rb))


def _irregular(n, frac):
    """an index near frac * n that is neither 0 nor a power of two"""
    k = max(3, int(frac * n)) % n
    while k == 0 or (k & (k - 1)) == 0:
        k = (k + 1) % n
    return k


def fft_inputs(N, seed=5):
    """(name, complex64 input, float64 DFT of that input, bins exempt from (b), bin whose error is reported relative to its value)"""
    rng = np.random.default_rng(seed + N)
    n = np.arange(N, dtype=np.int64)

    def tone(k, amp=1.0):
        return amp * np.exp(2j * np.pi * ((k * n) % N).astype(np.float64) / N)

    def case(name, x, exempt=(), weak=None):
        x = x.astype(np.complex64)
        return name, x, np.fft.fft(x.astype(np.complex128)), exempt, weak

    yield case("noise", (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * 0.5)
    for n0 in sorted({_irregular(N, 0.37), N - 1}):
        x = np.zeros(N, np.complex128)
        x[n0] = 0.75 - 0.5j
        yield case("impulse@%d" % n0, x)
    for k0 in sorted({0, N // 2, N - 1, _irregular(N, 0.2371)}):
        yield case("tone@%d" % k0, tone(k0) * (0.6 + 0.3j), exempt=(k0,))
    if N >= 4:
        k1, k2 = _irregular(N, 0.1234), _irregular(N, 0.6789)
        if k2 == k1:
            k2 = (k1 + 1) % N
        yield case("tones@%d,%d(-100dB)" % (k1, k2), tone(k1) + tone(k2, 1e-5), exempt=(k1,), weak=k2)


def check_fft_exact(ctx, F, quiet=False):
    """run every input of fft_inputs through fft_only at fftSize F; assert (a) and (b); return the worst ratios to the two bounds"""
    from cubicsdr_amd.engine import SpectrumProcessor
    N = 2 * F
    b2 = fft_l2_bound(F)
    sp = SpectrumProcessor(ctx, F, max_frames=1)
    worst_a = worst_b = 0.0
    try:
        for name, x, want, tones, weak in fft_inputs(N):
            got = sp.fft_only(x).astype(np.complex128)
            assert np.all(np.isfinite(got)), (F, name)
            binf = fft_bin_bound(F, x, want, tones)
            ea = fft_l2_err(got, want)
            eb = fft_bin_err(got, want, tones)
            worst_a, worst_b = max(worst_a, ea / b2), max(worst_b, eb / binf)
            assert ea <= b2, (F, name, "relative L2 %.3g u log2 N_eff, bound %.3g" % tuple(e / U32 / math.log2(fft_n_eff(F)[0]) for e in (ea, b2)))
            assert eb <= binf, (F, name, "per-bin error %.3g x the bound" % (eb / binf))
            if tones:
                # off the tones' bins the spectrum is the input's own rounding and the transform's: |X^_k| itself within (b)
                off = np.abs(got)
                off[list(tones)] = 0.0
                if weak is not None:
                    off[weak] = 0.0
                assert off.max() <= binf, (F, name, "leakage %.3g x the bound" % (off.max() / binf))
            if weak is not None and not quiet:
                print("fftSize %d %s: the weak tone's bin within %.2g of its value" % (F, name, abs(got[weak] - want[weak]) / abs(want[weak])))
    finally:
        sp.close()
    return worst_a, worst_b


@pytest.mark.parametrize("F,plan", [(F, fft_plan(F)) for F in SIZES])
def test_fft_exact_against_float64(ctx, F, plan):
    ra, rb = check_fft_exact(ctx, F)
    w = WORST.setdefault(plan, [0.0, 0.0, []])
    w[0], w[1] = max(w[0], ra), max(w[1], rb)
    w[2].append(F)
    print("fftSize %d (%s): worst (a) %.3f, (b) %.3f of the bound" % (F, plan, ra, rb))


# ----------------------------------------------------------------------------------------------- display points of process(), contiguous frames
DISPLAY_SIZES = [(512, "spec_fft_small"), (8192, "radix 8 + rows"), (65536, "fused spec_cols512p + spec_rows256_ema"), (1 << 18, "Ra x Rb + rows"),
                 (1 << 20, "spec_cols512 + rows"), (600, "chirp-z in LDS"), (12345, "chirp-z, power-of-two chains")]


def check_display_exact(ctx, F, frames_per_batch=(3, 4, 2), fs=2400000, seed=61):
    """process(contiguous=True) over three calls -- several frames per call, the first call leaving an odd number of samples behind, so
    that frame 0 of the next call lies in two pieces (carry ++ new data) -- against the restatement with a float64 transform
    (tests.util.exact_spectrum): every display point within DisplayBound, ceiling and floor within theirs.  Dense noise (sigma 0.2 per
    component) under four carriers.  Returns the worst ratio of |point - exact point| to its bound."""
    from cubicsdr_amd.engine import SpectrumProcessor
    from tests.test_gpu_parity import _backend
    from tests.util import exact_spectrum, synth_iq
    N = 2 * F
    odd = ((1000 % N) | 1, (77 % N) | 1, 0)
    lens = [nf * N + o for nf, o in zip(frames_per_batch, odd)]
    lens[1] -= odd[0]
    lens[2] -= odd[1]
    x = synth_iq(sum(lens), fs, 0, [("NBFM", 0.21 * fs), ("AM", -0.33 * fs), ("USB", 0.05 * fs), ("NBFM", -0.07 * fs)], seed=seed, noise=0.2)
    ex = exact_spectrum(_backend(), F)
    sp = SpectrumProcessor(ctx, F, max_frames=max(frames_per_batch) + 1)
    pos = done = 0
    worst = worst_ce = 0.0
    try:
        for k, n in enumerate(lens):
            nf = sp.process(x[pos:pos + n], 1, n, contiguous=True)
            assert nf == (pos + n) // N - done, (F, k, nf)
            for j in range(nf):
                wp, wce, wfl = ex.process_frame(x[(done + j) * N:(done + j + 1) * N])
                b = ex.bound.point_bound
                pts, ce, fl = sp.fetch(j)
                assert np.array_equal(pts[0::2], wp[0::2]), (F, k, j)
                err = np.abs(pts[1::2].astype(np.float64) - wp[1::2].astype(np.float64))
                ratio = np.divide(err, b, out=np.zeros_like(err), where=err > 0)      # (an exact match needs no bound: b may be 0 there)
                i = int(np.argmax(ratio))
                assert ratio[i] <= 1.0, (F, k, j, "point %d: |hip - exact| %.3g, bound %.3g" % (i, err[i], b[i]))
                worst = max(worst, float(ratio[i]))
                assert abs(ce - wce) <= ex.bound.ceil_bound and abs(fl - wfl) <= ex.bound.floor_bound, (F, k, j, ce, wce, fl, wfl)
                worst_ce = max(worst_ce, abs(ce - wce) / max(ex.bound.ceil_bound, 1e-300), abs(fl - wfl) / max(ex.bound.floor_bound, 1e-300))
            done += nf
            pos += n
    finally:
        sp.close()
    assert done == sum(frames_per_batch)
    return worst, worst_ce


@pytest.mark.parametrize("F,plan", DISPLAY_SIZES)
def test_spectrum_display_points_against_float64(ctx, F, plan):
    w, wc = check_display_exact(ctx, F)
    print("fftSize %d (%s): display points at worst %.3f of their bound, ceiling / floor %.3f" % (F, plan, w, wc))
