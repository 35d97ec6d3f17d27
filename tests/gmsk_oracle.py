"""TEST INFRASTRUCTURE ONLY: the reference's GMSK modem (ModemGMSK.cpp) as the parity oracle.

tests/digital/liquid_gmsk_shim.c is compiled at test time (gcc, into a pytest tmp dir) and linked against the oracle's loader of the reference
liquid-dsp binary (oracle/_ref/libliquid_ref.so); it calls the binary's own gmskdem / gmskmod objects and filter designs.  RefGMSK restates,
around a gmskdem object, what ModemGMSK::demodulate does per block (ModemGMSK.cpp:116-134): the inputBuffer grows by the block and shrinks by
the samples "processed", while each symbol reads the current block from its start -- samples past the block's end read as zero here (the
reference reads whatever lies beyond its vector: DESIGN section 15).
"""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.digital_oracle import REF_DIR, available  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM_SRC = os.path.join(HERE, "digital", "liquid_gmsk_shim.c")
DEFAULT_RATE = 19200          # CubicSDR.cpp registry: ModemGMSK::getDefaultSampleRate


def h_len(k, m):
    return 2 * int(k) * int(m) + 1


def refused(k, m, bt):
    """gmskdem_create's refusals: k < 2, m < 1, BT outside (0, 1)"""
    return k < 2 or m < 1 or not (0.0 < np.float32(bt) < 1.0)


_shim = None


def shim(build_dir):
    """compile (once per process) and load the shim; build_dir: a writable scratch directory"""
    global _shim
    if _shim is None:
        out = os.path.join(str(build_dir), "libliquid_gmsk_shim.so")
        subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", SHIM_SRC, "-o", out, "-L" + REF_DIR, "-lliquid_ref",
                        "-Wl,-rpath," + REF_DIR], check=True)
        lib = C.CDLL(out)
        p, i, u, f = C.c_void_p, C.c_int, C.c_uint, C.c_float
        sig = {"shim_gmsk_ready": (i, []), "shim_gmskdem_create": (p, [u, u, f]), "shim_gmskdem_reset": (None, [p]),
               "shim_gmskdem_destroy": (None, [p]), "shim_gmskdem_run": (None, [p, p, i, i, p]), "shim_gmskmod_create": (p, [u, u, f]),
               "shim_gmskmod_destroy": (None, [p]), "shim_gmskmod_run": (None, [p, p, i, i, p]), "shim_firdes_gmsktx": (i, [u, u, f, p]),
               "shim_firdes_gmskrx": (i, [u, u, f, p])}
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        assert lib.shim_gmsk_ready(), "the reference binary lacks a gmskdem / gmskmod / firdes export"
        _shim = lib
    return _shim


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def taps(lib, k, m, bt):
    """(tx, rx): the binary's liquid_firdes_gmsktx / liquid_firdes_gmskrx, h_len = 2 k m + 1 each"""
    n = h_len(k, m)
    tx, rx = np.zeros(n, np.float32), np.zeros(n, np.float32)
    lib.shim_firdes_gmsktx(k, m, bt, _ptr(tx))
    lib.shim_firdes_gmskrx(k, m, bt, _ptr(rx))
    return tx, rx


def modulate(lib, sym, k, m, bt):
    """the binary's gmskmod: k samples per symbol from a fresh object"""
    sym = np.ascontiguousarray(sym, dtype=np.uint32)
    q = lib.shim_gmskmod_create(k, m, bt)
    assert q
    out = np.zeros(sym.size * k, np.complex64)
    lib.shim_gmskmod_run(q, _ptr(sym), sym.size, k, _ptr(out))
    lib.shim_gmskmod_destroy(q)
    return out


class Dem:
    """one gmskdem object of the reference binary"""

    def __init__(self, lib, k, m, bt):
        self.lib, self.k = lib, int(k)
        self.q = lib.shim_gmskdem_create(k, m, bt)
        assert self.q

    def demodulate(self, x):
        """len(x) // k consecutive gmskdem_demodulate calls"""
        x = np.ascontiguousarray(x, dtype=np.complex64)
        n = x.size // self.k
        out = np.zeros(max(1, n), np.uint32)
        self.lib.shim_gmskdem_run(self.q, _ptr(x), n, self.k, _ptr(out))
        return out[:n]

    def close(self):
        if self.q:
            self.lib.shim_gmskdem_destroy(self.q)
            self.q = None


def phase_differences(x, x_prime=0j):
    """phi[i] = arg(conj(x[i - 1]) x[i]) of float32 samples (x[-1] = x_prime), as the binary evaluates it -- exact zeros included"""
    x = np.asarray(x, dtype=np.complex64)
    xp = np.concatenate([np.array([x_prime], np.complex64), x[:-1]])
    a, b, c, d = (v.astype(np.float32) for v in (xp.real, xp.imag, x.real, x.imag))
    with np.errstate(all="ignore"):
        re = (a * c) + (b * d)
        im = (a * d) - (b * c)
    return np.arctan2(im, re).astype(np.float32)


def soft(h, phi, k, hist=None):
    """float64 d_hat of each symbol: the filter output after the symbol's first push, sum_i h[i] phi[n - i] (hist: the h_len - 1 phase
    differences before phi, oldest first; None = a fresh object's zeros)"""
    h = np.asarray(h, np.float64)
    L = h.size
    hist = np.zeros(L - 1) if hist is None else np.asarray(hist, np.float64)
    s = np.concatenate([hist, np.asarray(phi, np.float64)])
    n_sym = len(phi) // k
    idx = (L - 1) + np.arange(n_sym) * k
    win = s[idx[:, None] - np.arange(L)[None, :]]
    return win @ h


def rounding_bound(h, k):
    """how far a float32 d_hat may lie from the float64 one: phi rounded (2 ulp of pi each), the h_len-term float32 sum and the product's taps
    against the binary's (1e-5 of the peak, the design tolerance), all scaled by pi sum |h|"""
    h = np.asarray(h, np.float64)
    u = 2.0 ** -24
    return np.pi * np.abs(h).sum() * (4 * u + h.size * u + 1e-5)


class RefGMSK:
    """ModemGMSK::demodulate (ModemGMSK.cpp:116-134) block by block around the binary's gmskdem object"""

    def __init__(self, lib, sps=4, fdelay=3, ebf=0.3):
        self.k, self.m, self.bt = int(sps), int(fdelay), float(ebf)
        self.dem = Dem(lib, self.k, self.m, self.bt)
        self.c = 0                      # inputBuffer.size(): only the count matters, its contents are never read

    def plan(self, n):
        """(symbols, carry after, the last sample index read + 1) of a block of n samples"""
        S = self.c + n
        i_max = S // self.k
        n_sym = (i_max + self.k - 1) // self.k
        return n_sym, S - n_sym * self.k, n_sym * self.k

    def demodulate(self, x):
        """one block: (symbols, console text, inputBuffer.size() after)"""
        x = np.asarray(x, dtype=np.complex64)
        n_sym, carry, end = self.plan(x.size)
        buf = np.zeros(max(end, x.size), np.complex64)
        buf[:x.size] = x
        syms = self.dem.demodulate(buf[:n_sym * self.k])
        self.c = carry
        return syms, "".join("%x" % int(s) for s in syms), carry

    def close(self):
        self.dem.close()
