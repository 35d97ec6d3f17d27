"""TEST INFRASTRUCTURE ONLY: the reference's digital modems as the parity oracle.

tests/digital/liquid_digital_shim.c is compiled at test time (gcc, into a pytest tmp dir) and linked against the oracle's loader of the
reference liquid-dsp binary (oracle/_ref/libliquid_ref.so); it calls the binary's own modemcf / fskdem objects.  RefDigital restates, around
those objects, what the reference classes of src/modules/modem/digital/ do per block: one modemcf object per constellation created up front
and switched by writeSetting("cons"), updateDemodulatorLock after each block, ModemFSK's inputBuffer and its hex console text.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
SHIM_SRC = os.path.join(HERE, "digital", "liquid_digital_shim.c")

KINDS = ["PSK", "DPSK", "ASK", "QAM", "BPSK", "QPSK", "OOK", "FSK"]
CONS = {"PSK": [2, 4, 8, 16, 32, 64, 128, 256], "DPSK": [2, 4, 8, 16, 32, 64, 128, 256], "ASK": [2, 4, 8, 16, 32, 64, 128, 256],
        "QAM": [4, 8, 16, 32, 64, 128, 256], "BPSK": [2], "QPSK": [4], "OOK": [2]}
SENSITIVITY = {"PSK": 0.005, "DPSK": 0.005, "ASK": 0.005, "QAM": 0.5, "BPSK": 0.005, "QPSK": 0.8, "OOK": 0.005}   # updateDemodulatorLock calls
DEFAULT_RATE = {"FSK": 19200}          # CubicSDR.cpp registry: getDefaultSampleRate (every other digital modem: 200000)


def scheme(kind, cons):
    """liquid's modulation_scheme enum value: PSK2..256 = 1..8, DPSK 9..16, ASK 17..24, QAM4..256 = 25..31, BPSK 39, QPSK 40, OOK 41"""
    m = int(cons).bit_length() - 1
    return {"PSK": m, "DPSK": 8 + m, "ASK": 16 + m, "QAM": 23 + m}.get(kind) or {"BPSK": 39, "QPSK": 40, "OOK": 41}[kind]


def available():
    return os.path.exists(os.path.join(REF_DIR, "libliquid_ref.so")) and os.path.exists(os.path.join(REF_DIR, "libliquid.dll"))


_shim = None


def shim(build_dir):
    """compile (once per process) and load the shim; build_dir: a writable scratch directory"""
    global _shim
    if _shim is None:
        out = os.path.join(str(build_dir), "libliquid_digital_shim.so")
        subprocess.run([os.environ.get("CC", "gcc"), "-O2", "-fPIC", "-shared", SHIM_SRC, "-o", out, "-L" + REF_DIR, "-lliquid_ref",
                        "-Wl,-rpath," + REF_DIR], check=True)
        lib = C.CDLL(out)
        p, i = C.c_void_p, C.c_int
        sig = {"shim_ready": (i, []), "shim_modem_create": (p, [i]), "shim_modem_destroy": (None, [p]), "shim_modem_evm": (C.c_float, [p]),
               "shim_modem_modulate": (None, [p, p, i, p]), "shim_modem_run": (None, [p, p, i, p, p]),
               "shim_fsk_create": (p, [C.c_uint, C.c_uint, C.c_float]), "shim_fsk_destroy": (None, [p]), "shim_fsk_run": (None, [p, p, i, i, p])}
        for name, (res, args) in sig.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        assert lib.shim_ready(), "the reference binary lacks a modemcf / fskdem export"
        _shim = lib
    return _shim


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Modem:
    """one modemcf object of the reference binary"""

    def __init__(self, lib, kind, cons):
        self.lib, self.q = lib, lib.shim_modem_create(scheme(kind, cons))
        assert self.q

    def demodulate(self, x, evm_each=False):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        s = np.zeros(x.size, np.uint32)
        e = np.zeros(x.size, np.float32) if evm_each else None
        self.lib.shim_modem_run(self.q, _ptr(x), x.size, _ptr(s), _ptr(e) if evm_each else None)
        return (s, e) if evm_each else s

    def modulate(self, sym):
        sym = np.ascontiguousarray(sym, dtype=np.uint32)
        out = np.zeros(sym.size, np.complex64)
        self.lib.shim_modem_modulate(self.q, _ptr(sym), sym.size, _ptr(out))
        return out

    def evm(self):
        return float(self.lib.shim_modem_evm(self.q))

    def close(self):
        if self.q:
            self.lib.shim_modem_destroy(self.q)
            self.q = None


def fsk_create(lib, bps, k, bw):
    return lib.shim_fsk_create(int(bps), int(k), float(bw))


def fsk_symbols(lib, q, x, k):
    x = np.ascontiguousarray(x, dtype=np.complex64)
    n = x.size // k
    out = np.zeros(max(1, n), np.uint32)
    lib.shim_fsk_run(q, _ptr(x), n, int(k), _ptr(out))
    return out[:n]


def constellation(lib, kind, cons):
    """every point of the reference's constellation, by symbol (the DLL's own modulator; DPSK: its PSK points)"""
    m = Modem(lib, "PSK" if kind == "DPSK" else kind, cons)
    pts = m.modulate(np.arange(cons, dtype=np.uint32))
    m.close()
    return pts


def min_distance(pts):
    d = np.abs(pts[:, None] - pts[None, :])
    return float(d[d > 0].min())


class RefDigital:
    """ModemPSK / DPSK / ASK / QAM / BPSK / QPSK / OOK / FSK (src/modules/modem/digital/) around the reference binary's objects, block by block"""

    def __init__(self, lib, kind, cons=0, bps=1, sps=9600, bw=0.45, rate=None):
        self.lib, self.kind = lib, kind
        self.lock = False
        if kind == "FSK":
            self.bps, self.sps, self.bw = bps, sps, bw
            self.rate = rate
            self.k = int(rate) // int(sps)
            self.q = fsk_create(lib, bps, self.k, bw)
            self.buf = np.zeros(0, np.complex64)
            return
        self.objs = {}
        self.set_cons(cons or CONS[kind][0])

    def set_cons(self, cons):            # updateDemodulatorCons: the object of that constellation, created once, its state kept
        self.cons = cons
        if cons not in self.objs:
            self.objs[cons] = Modem(self.lib, self.kind, cons)

    def demodulate(self, x):
        """one block: returns (symbols, evm or None, console text)"""
        x = np.asarray(x, dtype=np.complex64)
        if self.kind == "FSK":         # ModemFSK.cpp:127-143
            self.buf = np.concatenate([self.buf, x])
            n = self.buf.size // self.k
            syms = fsk_symbols(self.lib, self.q, self.buf[:n * self.k], self.k)
            self.buf = self.buf[n * self.k:].copy()
            return syms, None, "".join("%x" % int(s) for s in syms)
        m = self.objs[self.cons]
        syms = m.demodulate(x)
        evm = m.evm()
        self.lock = evm <= np.float32(SENSITIVITY[self.kind])
        return syms, evm, ""

    def close(self):
        if self.kind == "FSK":
            if self.q:
                self.lib.shim_fsk_destroy(self.q)
                self.q = None
            return
        for m in self.objs.values():
            m.close()
        self.objs = {}


def perturbed_runs(lib, kind, cons, x, rel=1e-6):
    """the reference decisions of x moved by `rel` relative in eight directions (scaled, rotated, shifted on each rail, both signs), each
    through a fresh object: a sample whose decision changes in any of them lies on a decision boundary"""
    x = np.asarray(x, dtype=np.complex64)
    a = np.abs(x).astype(np.float32)
    outs = []
    for d in (x * (1 + rel), x * (1 - rel), x * (1 + 1j * rel), x * (1 - 1j * rel), x + rel * a, x - rel * a, x + 1j * rel * a, x - 1j * rel * a):
        m = Modem(lib, kind, cons)
        outs.append(m.demodulate(d.astype(np.complex64)))
        m.close()
    return outs


def boundary_mask(lib, kind, cons, x, ref_syms, rel=1e-6):
    mask = np.zeros(ref_syms.size, bool)
    for s in perturbed_runs(lib, kind, cons, x, rel):
        mask |= s != ref_syms
    return mask
