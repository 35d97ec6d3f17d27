"""Shared helpers for the parity tests: seeded synthetic IQ and error metrics."""
import math

import numpy as np


def rel_err(a, b):
    """max |a - b| relative to the reference's peak magnitude (the tolerance unit used throughout: 1e-5)."""
    a = np.asarray(a)
    b = np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    s = float(np.max(np.abs(b)))
    return float(np.max(np.abs(a - b))) / max(s, 1e-30)


# ----------------------------------------------------------------------------------------------- transform accuracy against float64
# rel_err is blind to a transform that is subtly wrong: on a carrier-over-noise signal the peak bin is ~1000 x the median one, so an error of
# 1 % of a median bin passes 1e-5 of the peak.  The metrics below hold a float32 transform to what its rounding can explain.
#
# Model.  A power-of-two transform of N = 2^m points is m radix-2 stages (a radix-R pass or an R-point row counts log2 R of them: in exact
# arithmetic it is the same linear map).  Each stage is sqrt(2) times a unitary map, so an error the stage adds travels to the output
# scaled exactly as the signal is.  Stage j, computed in float32 from its computed input v, returns the exact stage of v plus a local
# error e_j.  Per output element e_j holds the rounding of the sum a +- w b (two real roundings), of the product w b (two with FMA) and the
# twiddle's own table error (a correctly rounded entry, a product of split-table entries or of up to four of them: a few roundings, but
# on half the elements or fewer).  With roundings independent, zero mean and uniform on [-u, u] (variance u^2 / 3 each, u = 2^-24) that
# is an rms of at most u |v|: ||e_j||_2 <= u ||v_j||_2.  Adding the m stages' errors IN PHASE (the worst the random model allows, and
# more than independent errors give: their sum grows as sqrt(m)) bounds the transform:
#   (a)  ||X^ - X||_2 / ||X||_2 <= c2 u log2 N,                c2 = 1
# (the worst-case analysis, Higham, Accuracy and Stability of Numerical Algorithms, thm 24.2, gives 4 sqrt(2) + 1 per stage: every rounding
# extreme and aligned -- a bound no real transform comes near and one that would pass a wrong twiddle).
# Per bin.  The error stage j leaves in bin k is the sum, over the 2^(m-j) elements of stage j that feed bin k, of their local errors
# times unit twiddles: variance <= u^2 times the energy of those elements, which is ||x||_2^2 when the input is spread (noise, impulse).
# So the rms error of one bin is <= c2 u log2 N ||x||_2, and the largest of N such errors exceeds the rms by the tail factor of N complex
# Gaussians, sqrt(ln N) <= sqrt(ln 2^22) = 3.9:
#   (b)  max_k |X^_k - X_k| <= c_inf u log2 N ||x||_2  (+ the tone term below),          c_inf = 4
# This is the form that makes a sparse input meaningful: every bin of an impulse has modulus ||x||_2 and is held to a few u log2 N of it.
# A tone is the one input whose energy does NOT stay spread: its path through the stages concentrates it, so its bin k0 is a sum of N
# values of one phase (exempt from (b); (a) holds it), and the roundings on its path land in the bins the factorisation aliases k0 to
# (k0 + j N / R).  On that path stage m - i holds 2^-i of the tone's bins' modulus |X_k0| in each of 2^i elements, whose errors (rms
# u 2^-i |X_k0| each, independent phases) reach one bin as u 2^(-i/2) |X_k0|; summed over the stages, u |X_k0| / (1 - 2^-1/2) = 3.41 u |X_k0|:
#   tone term      + c_tone u sum_t |X_kt|  over the tones' bins k_t,                    c_tone = 4
# (without it the lattice bins of a tone at an irregular bin sit at 0.5 .. 1.5 u |X_k0|, up to 2.4 x a bound scaled by ||x||_2 alone).
# Chirp-z (N not a power of two: X = w . IFFT_L(Bf . FFT_L(w . x)) / L, L >= 2 N - 1 a power of two): two L-point transforms and three
# pointwise products (x w, times Bf, times w) with rounded tables w and Bf -- at most twice the stages of one L-point transform, so
# N_eff = L and both constants carry the factor CHIRP_Z = 2.
# Mutation check: one copied entry of the 1024-entry fine twiddle table (lo[700] = lo[699]) puts (a) at 12.5 u log2 N at fftSize 16384 and
# 3.0 u log2 N at fftSize 65536; every plan of a correct transform stays under 0.32 of both bounds (tests/test_gpu_fft_exact.py).
U32 = 2.0 ** -24
FFT_C2 = 1.0
FFT_CINF = 4.0
FFT_CTONE = 4.0
CHIRP_Z = 2.0


def fft_n_eff(fft_size):
    """(N_eff, is_chirp_z) of the spectrum's transform of 2 fftSize points: N itself, or the chirp-z convolution length L"""
    N = 2 * int(fft_size)
    if N & (N - 1) == 0:
        return N, False
    L = 1
    while L < 2 * N - 1:
        L <<= 1
    return L, True


def fft_l2_bound(fft_size):
    """the bound of (a) for the spectrum's transform at fftSize"""
    n_eff, cz = fft_n_eff(fft_size)
    return (CHIRP_Z if cz else 1.0) * FFT_C2 * U32 * math.log2(n_eff)


def fft_l2_err(got, want):
    """(a): ||got - want||_2 / ||want||_2, in float64"""
    d = np.asarray(got, np.complex128) - np.asarray(want, np.complex128)
    return float(np.linalg.norm(d) / max(np.linalg.norm(np.asarray(want, np.complex128)), 1e-300))


def fft_bin_bound(fft_size, x, want, tones=()):
    """(b) as an absolute bound on |X^_k - X_k|: c_inf u log2 N_eff ||x||_2 + c_tone u sum |X_kt| over the tones' bins (chirp-z: x CHIRP_Z)"""
    n_eff, cz = fft_n_eff(fft_size)
    kap = CHIRP_Z if cz else 1.0
    tone = sum(abs(complex(want[k])) for k in tones)
    return kap * U32 * (FFT_CINF * math.log2(n_eff) * float(np.linalg.norm(np.asarray(x, np.complex128))) + FFT_CTONE * tone)


def fft_bin_err(got, want, exclude=()):
    """max_k |got_k - want_k| over the bins not in `exclude` (compared with fft_bin_bound)"""
    d = np.abs(np.asarray(got, np.complex128) - np.asarray(want, np.complex128))
    if len(exclude):
        d[list(exclude)] = 0.0
    return float(d.max())


def fft_tone_bins(fft_size, x, X):
    """the bins a general input concentrates its energy in, for the tone term of fft_bin_bound: |X_k| > log2 N_eff ||x||_2 (there the
    tone term outweighs the spread one; white noise reaches 4 ||x||_2 in one bin of 2^22)"""
    n_eff, _ = fft_n_eff(fft_size)
    return np.flatnonzero(np.abs(X) > math.log2(n_eff) * float(np.linalg.norm(np.asarray(x, np.complex128))))


# ----------------------------------------------------------------------------------------------- sample path accuracy against float64
# The channelizers and the demodulator front-end in front of the modems, held the same way (tests/test_gpu_sample_path_exact.py; the float64
# restatements are tests/sample_path_oracle.py).  Same random-rounding model: every rounded float32 operation adds an independent, zero-mean
# error of variance <= u^2 / 3 times the square of its result; errors of stages in series are added IN PHASE; the maximum over the n outputs
# of a run exceeds the rms by the tail factor of n complex Gaussians, sqrt(ln n) <= 3.9 up to n = 2^22: TAIL = 4 (= c_inf above).
#
# Front-end, per output j:    |y^_j - y_j| <= c_fe u A_j
# A_j is the ABSOLUTE-VALUE cascade of output j: the same mix -> half-band stages -> 2^-S -> 14-tap arm with |taps| applied to |x_n|.  Every
# partial sum of every chain that feeds y_j is at most its share of A_j in modulus, and a local error made at one stage reaches y_j through
# the later stages' taps, i.e. scaled by no more than the absolute-value cascade from there on (the errors of different samples are
# independent, so they add as sqrt(sum h^2 e^2) <= sum |h| |e|).  So a stage whose outputs each pass r rounded operations IN SERIES adds an
# error of rms <= sqrt(r / 3) u A_j to output j (real and imaginary parts are separate real filters of |Re x| and |Im x|, whose absolute
# cascades combine to no more than that of |x|: no further factor for the complex modulus).  Roundings in series per stage:
#   mix            x (c +- j s) per component fma(x, c, rounded(y s)): 2, each of modulus <= |x| over the two components   sqrt(2 / 3) = 0.816
#                  (no mix at offset 0: the term is dropped.  The table's own rounding is not in it: the restatement reads the same table)
#   half-band, m   y = O + sum_{j<m} h_j (E_k-j + E_k-(2m-1)+j): the m pair sums are parallel (one rounding deep, their errors weighted by
#                  |h_j|: together <= one rounding of the absolute sum), then an m-term fma chain: 1 + m                    sqrt((m + 1) / 3)
#                  m = 3, 5, 10: 1.155, 1.414, 1.915
#   2^-S           a power of two: exact                                                                                   0
#   arm            14-term fma chain, its last rounding the stored float32: 14                                             sqrt(14 / 3) = 2.160
#   c_fe = TAIL (0.816 [mixed] + sum over the stages sqrt((m_e + 1) / 3) + 2.160)
#   bare arm 8.6, arm + mix (S = 0) 11.9, S = 1 (m = 10) 19.6, S = 2 25.2, S = 3 (3, 5, 10) 29.8, S = 4 34.5, S = 5 39.1, S = 6 43.7, S = 10 62.2
# The interpolating form (arm first, then S x2 stages: w'[2q] = w[q - m] a copy, w'[2q + 1] the same folded m-term chain) has the same count
# with the stages behind the arm, and A_j is the absolute-value cascade in that order.  No absolute floor: where A_j = 0 (in front of a lone
# sample) every product is an exact zero and so must the output be.
#
# Channelizer (firpfbch / firpfbch2), frame t:  v_t[c] = sum_{n<8} taps[c][n] x[..] (an 8-term fma chain: rms sqrt(8 / 3) u a_t[c], a_t the
# absolute-value FIR sum |taps| |x|), X_t = DFT_M(v_t).  Forms (a) and (b) of the transform with N_eff = M -- a radix-R pass, a direct prime
# pass on the matrix pipe or an R-point row counts log2 R stages --, CHIRP_Z = 2 where a prime factor >= 211 runs as a chirp-z pass, and one
# term for the FIR, whose errors (independent per commutator position) reach every bin with unit weights: rms sqrt(8 / 3) u ||a_t||_2 per
# bin, sqrt(M) times that over the frame.  The oversampled bank multiplies every output by its post factor W_M^k / M (a rounded table entry
# and a complex product: one more stage of the model, log2 M + 1; the gain 1 / M and the sign (-1)^k of odd frames are exact):
#   (a)  ||X^ - X||_2 <= u (kappa c2 L ||X||_2 + c_fir sqrt(M) ||a||_2)                        over all frames, L = log2 M (+ 1 oversampled)
#   (b)  |X^_t,k - X_t,k| <= u (TAIL (kappa L ||v_t||_2 + c_fir ||a_t||_2) + c_tone kappa sum_tones |X_t,k0|)     c_fir = sqrt(8 / 3) = 1.633
# (the oversampled bank's X, v and a carry its gain 1 / M).  The tone term is needed exactly as for the spectrum: a tone on a channel centre
# is a constant v_t, whose path through the factorisation leaves 2.6 .. 3.3 u |X_k0| in the rows k0 aliases to (M = 122).
# Tone rows.  A row of a frame is a tone's own -- exempt from (b), held by (a), its modulus in the tone term -- where it holds more than
# white noise of the frame's energy puts into any row: |X_t,k| > TAIL ||v_t||_2 (M <= 16 has no such row: sqrt(M) <= 4).  The spectrum's
# rule (fft_tone_bins: above log2 N ||x||_2, where ONE tone's term outweighs the spread term) is not enough here: a bank's prototype spans
# two channels (the oversampled one four), so a tone lies in two or three rows, each under that threshold (7.8 ||v_t||_2 twice against
# L = 7.9 at M = 122, halfway between two centres) and each leaving its 3.3 u |X| in the rows it aliases to: 0.59 of a bound without their
# terms in the first run of this test, against the condition below.  The threshold was moved to where concentration begins, not sized to
# that figure.
# Condition on both models (instead of a number fitted to a run): every correct kernel stays below HALF its bound, on the host-thread
# emulation and on the MI355X, and every mutant of the mutation record in tests/test_gpu_sample_path_exact.py exceeds it.
FE_TAIL = 4.0
FE_MIX = math.sqrt(2.0 / 3.0)
FE_ARM = math.sqrt(14.0 / 3.0)
CHAN_FIR = math.sqrt(8.0 / 3.0)


def fe_const(ms, mixed):
    """c_fe of a front-end cascade with half-band stages of half-lengths `ms` (decimating or interpolating), behind a mix or not"""
    return FE_TAIL * ((FE_MIX if mixed else 0.0) + sum(math.sqrt((m + 1) / 3.0) for m in ms) + FE_ARM)


def fe_ratio(got, want, A):
    """per output |got - want| / (u A); the floor only keeps 0 / 0 out (A = 0 demands an exact zero)"""
    e = np.abs(np.asarray(got, np.complex128) - np.asarray(want, np.complex128))
    return e / (U32 * np.asarray(A, np.float64) + 1e-300)


def chan_stages(M, oversampled=False):
    """(kappa, L) of the channelizer's transform: CHIRP_Z where M has a prime factor >= 211, log2 M stages (+ 1: firpfbch2's post factors)"""
    n, p, big = int(M), 2, 1
    while p * p <= n:
        while n % p == 0:
            big, n = max(big, p), n // p
        p += 1
    big = max(big, n)
    return (CHIRP_Z if big >= 211 else 1.0), math.log2(M) + (1.0 if oversampled else 0.0)


def chan_l2_bound(M, X, a, oversampled=False):
    """(a) as an absolute bound on ||X^ - X||_2 over all frames: X [frames, M] the exact rows, a [frames, M] the absolute-value FIR sums"""
    kap, L = chan_stages(M, oversampled)
    return U32 * (kap * FFT_C2 * L * float(np.linalg.norm(X)) + CHAN_FIR * math.sqrt(M) * float(np.linalg.norm(a)))


def chan_tone_rows(v, X):
    """[frames, M] mask of the rows a frame concentrates its energy in (exempt from (b), held by (a), their moduli in (b)'s tone term):
    |X_t,k| > TAIL ||v_t||_2, more than white noise of that energy reaches in a row"""
    return np.abs(X) > FE_TAIL * np.linalg.norm(v, axis=1)[:, None]


def chan_bin_bound(M, v, a, X, oversampled=False):
    """(b) per frame, [frames]: the bound on |X^_t,k - X_t,k| of every row k of frame t but the tones' own (chan_tone_rows)"""
    kap, L = chan_stages(M, oversampled)
    tone = np.sum(np.abs(X) * chan_tone_rows(v, X), axis=1)
    return U32 * (FE_TAIL * (kap * L * np.linalg.norm(v, axis=1) + CHAN_FIR * np.linalg.norm(a, axis=1)) + FFT_CTONE * kap * tone)


def exact_spectrum(backend, fft_size, average_rate=0.65, scale=1.0):
    """oracle.cubicsdr_chain.RefSpectrum with its transform in float64: the display points of the exact transform of each frame.  The
    instance also carries DisplayBound (display_bound()), the bound on |HIP point - exact point| that the transform bound (b) implies."""
    from oracle.cubicsdr_chain import RefSpectrum

    class ExactSpectrum(RefSpectrum):
        def fft(self, frame):
            x = np.asarray(frame, dtype=np.complex128)
            Y = np.fft.fft(x)
            if hasattr(self, "bound"):
                self.bound.transform(x, Y)
            return Y

        def process_frame(self, frame):
            out = super().process_frame(frame)
            if hasattr(self, "bound"):
                self.bound.display(self, out)
            return out

    ex = ExactSpectrum(backend, fft_size, average_rate, scale)
    ex.bound = DisplayBound(ex)
    return ex


class DisplayBound:
    """The transform bound (b) of every bin carried through the display arithmetic of RefSpectrum.process_frame (full-span view, no
    peak hold), evaluated in float64 from the exact restatement's own values: the bound on |point - exact point| of the current frame.
      magnitudes     |X^_k| - |X_k| <= e_k = (b) + 4 u |X_k|            (the float32 square, root and store, on either side)
      averagers      ma += (res - ma) r,  maa += (ma_old - maa) r: convex combinations (total weight <= 1), so
                     D_maa <- (1 - r) D_maa + r D_ma_old,  D_ma <- (1 - r) D_ma + r e
      ceiling/floor  the float32 max / min of maa move by at most max_k D_maa + 2 u |value|; their trackers (weight 0.05, ceil_maa from the
                     new ceil_ma) are convex combinations again: the same recursions
      pair sum       acc = maa_2x + maa_2x+1 (point 0: floor_maa + maa_1), float32 on the HIP side: D_acc = D_2x + D_2x+1 + 3 u acc
      logarithms     y = sf ln(a) / ln(d), a = 1 + acc / 2 - pf, d = 1 + pc - pf:
                     |dy| <= sf (D_a / (a- ln d-) + |ln a| D_d / (d- ln^2 d-)), a- = a - D_a, d- = d - D_d (the smaller value bounds both quotients)
      evaluation     the point's float32 arithmetic: the rounding of a - 1 (sf u |a - 1| / (a ln d)), that of d - 1 likewise relative to ln d,
                     log1p / reciprocal / products / store on the HIP side (8 u |y|) and the store of the exact point (u |y|)."""

    def __init__(self, ex):
        self.F, self.N, self.r, self.sf = ex.F, ex.N, ex.rate, ex.sf
        self.d_ma = np.zeros(self.N)
        self.d_maa = np.zeros(self.N)
        self.d_cma = self.d_cmaa = self.d_fma = self.d_fmaa = 0.0
        self.e = None

    def transform(self, x, Y):
        tones = fft_tone_bins(self.F, x, Y)
        aY = np.abs(Y)
        e = fft_bin_bound(self.F, x, Y, tones) + 4 * U32 * aY
        self.e = np.concatenate([e[self.N // 2:], e[:self.N // 2]])        # display (fftshift) order, as res
        self.e_max = float(e.max())

    def display(self, ex, out):
        pts, _, _ = out
        r, u = self.r, U32
        self.d_maa = (1 - r) * self.d_maa + r * self.d_ma
        self.d_ma = (1 - r) * self.d_ma + r * self.e
        dm = float(self.d_maa.max())
        fin = ex.maa[~np.isnan(ex.maa)]
        c = max(0.0, float(fin.max())) if fin.size else 0.0
        f = min(1.0, float(fin.min())) if fin.size else 1.0
        self.d_cma = 0.95 * self.d_cma + 0.05 * (dm + 2 * u * abs(c))
        self.d_cmaa = 0.95 * self.d_cmaa + 0.05 * self.d_cma
        self.d_fma = 0.95 * self.d_fma + 0.05 * (dm + 2 * u * abs(f))
        self.d_fmaa = 0.95 * self.d_fmaa + 0.05 * self.d_fma
        pc, pf = ex.ceil_maa, ex.floor_maa
        acc = ex.maa[0::2] + ex.maa[1::2]
        d_acc = self.d_maa[0::2] + self.d_maa[1::2] + 3 * u * np.abs(acc)
        acc[0] = ex.floor_maa + ex.maa[1]
        d_acc[0] = self.d_fmaa + self.d_maa[1] + 3 * u * abs(acc[0])
        a = 1.0 + acc / 2 - pf
        d = 1.0 + pc - pf
        d_a = d_acc / 2 + self.d_fmaa
        d_d = self.d_cmaa + self.d_fmaa
        a_lo, d_lo = a - d_a, d - d_d
        y = self.sf * np.log(a) / np.log(d)
        with np.errstate(divide="ignore", invalid="ignore"):
            ln_dlo = np.log(d_lo) if d_lo > 1.0 else 0.0
            prop = self.sf * (d_a / (a_lo * ln_dlo) + np.abs(np.log(a)) * d_d / (d_lo * ln_dlo ** 2))
            ev = self.sf * u * np.abs(a - 1) / (a * np.log(d)) + np.abs(y) * (u * abs(d - 1) / (d * np.log(d)) + 9 * u)
            b = prop + ev
        b[~(a_lo > 0)] = np.inf                                              # (a point the bound cannot place: not held)
        self.point_bound = b
        self.ceil_bound = self.d_cmaa / self.sf + 2 * u * abs(pc / self.sf)
        self.floor_bound = self.d_fmaa + 2 * u * abs(pf)
        return b


def demod_frequencies(center, fs, n):
    """evenly spaced, never on a channel centre: f0 + (k + 0.37) Fs / N - Fs / 2"""
    return [int(center + (k + 0.37) * fs / n - fs / 2) for k in range(n)]


def synth_iq(n, fs, center, demods, seed=0xC0B1C5D2, t0=0, noise=0.05, dc=(0.01, 0.01)):
    """complex64[n]: white noise sigma `noise` per component + one modulated carrier per demod + a DC offset.
    demods: list of (kind, frequency) with kind in NBFM/FM/AM/USB/LSB; amplitude 0.5 / sqrt(N)."""
    rng = np.random.default_rng(seed)
    t = (np.arange(n, dtype=np.float64) + t0) / fs
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * noise
    amp = 0.5 / math.sqrt(max(len(demods), 1))
    for kind, f in demods:
        df = f - center
        if kind in ("NBFM", "FM"):
            dev = 2500.0 if kind == "NBFM" else 50000.0
            ph = 2 * np.pi * df * t + (dev / 1000.0) * np.sin(2 * np.pi * 1000.0 * t)
            x += amp * np.exp(1j * ph)
        elif kind == "AM":
            x += amp * (1 + 0.8 * np.sin(2 * np.pi * 1000.0 * t)) * np.exp(2j * np.pi * df * t)
        elif kind == "USB":
            x += amp * np.exp(2j * np.pi * (df + 1000.0) * t)
        elif kind == "LSB":
            x += amp * np.exp(2j * np.pi * (df - 1000.0) * t)
        elif kind == "DSB":
            x += amp * np.sin(2 * np.pi * 700.0 * t) * np.exp(1j * (0.4 + 2 * np.pi * (df + 35.0) * t))   # suppressed carrier, 35 Hz off tune
        elif kind == "CW":
            x += amp * np.exp(2j * np.pi * (df + 60.0) * t) * (np.floor(t * 40.0) % 2 == 0)    # keyed carrier, 20 Hz dots
        elif kind == "I/Q":
            x += amp * np.exp(2j * np.pi * (df + 3000.0) * t)
        elif kind == "FMS":
            # FM broadcast multiplex: (L + R) + 19 kHz pilot + (L - R) on the suppressed 38 kHz subcarrier, 75 kHz deviation
            Ls = 0.8 * np.sin(2 * np.pi * 1000.0 * t) + 0.3 * np.sin(2 * np.pi * 3300.0 * t)
            Rs = 0.9 * np.sin(2 * np.pi * 700.0 * t + 1.0)
            mpx = 0.45 * (Ls + Rs) + 0.1 * np.sin(2 * np.pi * 19000.0 * t) + 0.45 * (Ls - Rs) * np.sin(2 * np.pi * 38000.0 * t)
            x += amp * np.exp(1j * (2 * np.pi * df * t + 2 * np.pi * 75000.0 * np.cumsum(mpx) / fs))
    x += dc[0] + 1j * dc[1]
    return x.astype(np.complex64)


def synth_iq_fast(n, fs, center, demods, seed=0xC0B1C5D2, noise=0.05, dc=(0.01, 0.01)):
    """the same signal model as synth_iq for the NBFM / AM / USB carriers of the BASELINE configurations, formed on the GPU when
    one is present (hundreds of carriers over millions of samples), numpy otherwise; returns a host complex64 array"""
    try:
        import torch
        use = torch.cuda.is_available()
    except Exception:
        use = False
    if not use:
        return synth_iq(n, fs, center, demods, seed=seed, noise=noise, dc=dc)
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed))
    x = torch.randn(n, 2, generator=g, device=dev, dtype=torch.float32) * noise
    amp = 0.5 / math.sqrt(max(len(demods), 1))
    SL = 1 << 21
    for s0 in range(0, n, SL):
        s1 = min(n, s0 + SL)
        t = torch.arange(s0, s1, device=dev, dtype=torch.float64) / fs
        tone = torch.sin(2 * math.pi * 1000.0 * t)
        ar = torch.zeros(s1 - s0, device=dev, dtype=torch.float64)
        ai = torch.zeros(s1 - s0, device=dev, dtype=torch.float64)
        for kind, f in demods:
            df = float(f - center)
            if kind in ("NBFM", "FM"):
                ph = (2 * math.pi * df) * t + ((2500.0 if kind == "NBFM" else 50000.0) / 1000.0) * tone
                ar += amp * torch.cos(ph); ai += amp * torch.sin(ph)
            elif kind == "AM":
                ph = (2 * math.pi * df) * t
                env = amp * (1 + 0.8 * tone)
                ar += env * torch.cos(ph); ai += env * torch.sin(ph)
            elif kind == "USB":
                ph = (2 * math.pi * (df + 1000.0)) * t
                ar += amp * torch.cos(ph); ai += amp * torch.sin(ph)
            else:
                raise ValueError(kind)
        x[s0:s1, 0] += (ar + dc[0]).float()
        x[s0:s1, 1] += (ai + dc[1]).float()
    return x.cpu().numpy().view(np.complex64).reshape(-1).copy()
