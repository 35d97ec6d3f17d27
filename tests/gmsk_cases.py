"""TEST INFRASTRUCTURE ONLY: the GMSK checks shared by the CPU emulation (tests/test_gmsk_emu.py) and the device (tests/test_gpu_gmsk.py), all
through csdr_gmsk_run against the reference binary's gmskdem (tests/gmsk_oracle.py).

A decision is compared wherever the float64 filter output d64 (the binary's taps, the phase differences of the float32 input) lies further from
zero than the rounding bound: float32 phase differences, the float32 sum, and the product's taps against the binary's, scaled by pi sum |h|.
"""
import ctypes as C

import numpy as np

from cubicsdr_amd import build
from cubicsdr_amd.engine import gmsk_run
from tests import gmsk_oracle as G

# (sps, fdelay, ebf): the default, short and long filters, a non-power-of-two sps
SETTINGS = [(4, 3, 0.3), (2, 1, 0.5), (8, 8, 0.3), (5, 2, 0.49), (16, 3, 0.3), (3, 24, 0.49)]
SNRS = [30.0, 15.0, 10.0]

_design = None


def product_taps(k, m, bt):
    """the receive filter the product uploads (design.hpp gmsk_rx_taps through libcsdr_design.so)"""
    global _design
    if _design is None:
        _design = C.CDLL(build.build_design(verbose=False))
        _design.csdr_design_gmsk.argtypes = [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int]
    n = G.h_len(k, m)
    tx, rx = np.zeros(n, np.float32), np.zeros(n, np.float32)
    assert _design.csdr_design_gmsk(k, m, bt, tx.ctypes.data, rx.ctypes.data, n) == n
    return tx, rx


def bound(lib, k, m, bt):
    _, h_ref = G.taps(lib, k, m, bt)
    _, h = product_taps(k, m, bt)
    return G.rounding_bound(h_ref, k) + np.pi * float(np.abs(h.astype(np.float64) - h_ref).sum()), h_ref


def modulated(lib, k, m, bt, n_sym, snr_db, cfo, seed):
    """the binary's gmskmod of random symbols, a carrier offset of `cfo` cycles per sample, complex AWGN at snr_db"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2, n_sym).astype(np.uint32)
    x = G.modulate(lib, bits, k, m, bt).astype(np.complex128)
    x *= np.exp(2j * np.pi * cfo * np.arange(x.size) + 1j * rng.uniform(0, 2 * np.pi))
    s = 10 ** (-snr_db / 20) / np.sqrt(2)
    x += s * (rng.standard_normal(x.size) + 1j * rng.standard_normal(x.size))
    return x.astype(np.complex64)


def noise(n, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)).astype(np.complex64)


def compare(ctx, lib, k, m, bt, x, max_exempt=None):
    """one call of the product and a fresh binary object on x; returns the exempt fraction after the filters' fill"""
    sym, soft, _ = gmsk_run(ctx, x, sps=k, fdelay=m, ebf=bt)
    dem = G.Dem(lib, k, m, bt)
    want = dem.demodulate(x)
    dem.close()
    b, h_ref = bound(lib, k, m, bt)
    d64 = G.soft(h_ref, G.phase_differences(x), k)
    assert sym.size == want.size == d64.size == x.size // k
    firm = np.abs(d64) > b
    bad = np.flatnonzero(firm & (sym != want))
    assert bad.size == 0, ("decisions differ", bad[:10], d64[bad[:10]], b)
    err = np.abs(soft.astype(np.float64) - d64)
    assert err.max() <= b, ("soft value outside the bound", float(err.max()), b)
    exempt = 1.0 - firm[2 * m:].mean()           # (the first 2m symbols: the modulator's and the demodulator's filters filling)
    if max_exempt is not None:
        assert exempt <= max_exempt, exempt
    return exempt


def check_modulated(ctx, lib, k, m, bt):
    for i, snr in enumerate(SNRS):
        x = modulated(lib, k, m, bt, 3000, snr, 0.0123 / k, seed=17 * k + 3 * m + i)
        compare(ctx, lib, k, m, bt, x, max_exempt=1e-3)


def check_noise(ctx, lib, k, m, bt):
    compare(ctx, lib, k, m, bt, noise(2000 * k, seed=5 + k + m))


def check_split(ctx, lib, k, m, bt):
    """a stream cut at arbitrary symbol boundaries through consecutive calls equals one call, bit for bit"""
    x = modulated(lib, k, m, bt, 1500, 10.0, 0.01 / k, seed=99 + k)
    sym1, soft1, _ = gmsk_run(ctx, x, sps=k, fdelay=m, ebf=bt)
    rng = np.random.default_rng(k * 1000 + m)
    cuts = np.sort(rng.choice(np.arange(1, 1500), 12, replace=False)) * k
    state, syms, softs = None, [], []
    for a, e in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [x.size]])):
        s, f, state = gmsk_run(ctx, x[a:e], state=state, sps=k, fdelay=m, ebf=bt)
        syms.append(s)
        softs.append(f)
    s, f, state = gmsk_run(ctx, x[:0], state=state, sps=k, fdelay=m, ebf=bt)      # an empty call changes nothing
    assert s.size == 0
    import pytest
    with pytest.raises(ValueError):                                                   # a state of other settings: its history has another length
        gmsk_run(ctx, x[:0], state=state, sps=k + 1, fdelay=m, ebf=bt)
    np.testing.assert_array_equal(np.concatenate(syms), sym1)
    np.testing.assert_array_equal(np.concatenate(softs).view(np.uint32), soft1.view(np.uint32))


QUADRANTS = [0.6 + 0.8j, -0.6 + 0.8j, -0.6 - 0.8j, 0.6 - 0.8j, 1 + 0j, -1 + 0j, complex(0.0, 1.0), complex(-0.0, -1.0), complex(-1.0, -0.0)]


def signed_zero_streams(k):
    """exact zeros as real inputs: a fresh object (x_prime = 0) meeting a sample of each quadrant, a sample of each quadrant followed by zeros,
    zeros between samples"""
    out = []
    for q in QUADRANTS:
        out.append(np.full(8 * k, q, np.complex64))
        out.append(np.concatenate([np.full(2 * k, q), np.zeros(6 * k)]).astype(np.complex64))
        out.append(np.concatenate([np.zeros(3 * k), np.full(k, q), np.zeros(2 * k), np.full(2 * k, np.conj(q))]).astype(np.complex64))
    return out


def check_signed_zeros(ctx, lib, k, m, bt):
    for x in signed_zero_streams(k):
        sym, soft, _ = gmsk_run(ctx, x, sps=k, fdelay=m, ebf=bt)
        dem = G.Dem(lib, k, m, bt)
        want = dem.demodulate(x)
        dem.close()
        np.testing.assert_array_equal(sym, want, err_msg=repr(x[:: k]))
        _, h_ref = G.taps(lib, k, m, bt)
        d64 = G.soft(h_ref, G.phase_differences(x), k)
        np.testing.assert_array_equal(sym, (d64 > 0).astype(np.uint32))    # the oracle's phase convention is the binary's


def check_refused(ctx, lib):
    """gmskdem_create's refusals (the binary returns no object) and the settings' walls: CSDR_EUNSUPPORTED (-6)"""
    import cubicsdr_amd.hip as H
    for k, m, bt in [(1, 3, 0.3), (4, 0, 0.3), (4, 3, 1.0), (4, 3, -0.2), (2, 1, 0.999), (513, 1, 0.3), (4, 129, 0.3)]:
        if k < 513 and m < 129:
            q = lib.shim_gmskdem_create(k, m, bt)
            assert bool(q) != G.refused(k, m, bt), (k, m, bt)
            if q:
                lib.shim_gmskdem_destroy(q)
        d = H.DigitalParams(H.CSDR_DIGITAL_GMSK, 0, 0, k, bt, m or -1)      # (0 selects the default in the product)
        st, n = H.GmskState(), C.c_int()
        x, hist = np.zeros(4 * k, np.complex64), np.zeros(max(1, 2 * k * m), np.float32)
        out, soft = np.zeros(4, np.uint32), np.zeros(4, np.float32)
        rc = H.lib().csdr_gmsk_run(ctx.h, d, x.ctypes.data, x.size, st, hist.ctypes.data, out.ctypes.data, soft.ctypes.data, out.size, n)
        assert rc == (0 if not G.refused(k, m, bt) and k <= 512 and m <= 128 else -6), (k, m, bt, rc)
