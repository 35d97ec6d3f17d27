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
