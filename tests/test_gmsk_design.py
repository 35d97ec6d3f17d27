"""CPU tests of the product's GMSK filter design (design.hpp gmsk_tx_taps / gmsk_rx_taps through libcsdr_design.so csdr_design_gmsk) against
the reference binary's liquid_firdes_gmsktx / liquid_firdes_gmskrx, and of the settings gmskdem_create refuses.

The receive filter is a ratio of spectra lifted by 1e-3, ill-conditioned where both lie near their minima: the binary's float32 steps move its
taps by up to 14 % of the peak from a float64 evaluation of the definition (k 512, m 8, BT 0.1).  The product evaluates the definition in double,
so at every grid point it must lie no further from that evaluation than the binary does (plus 1e-6), and within 1e-5 of the binary's taps
wherever h_len <= 4097 and the binary itself lies within 5e-6 of the definition."""
import time

import numpy as np
import pytest
from scipy.special import erfc, i0

from tests import gmsk_cases as K
from tests import gmsk_oracle as G
from tests.util import rel_err

pytestmark = pytest.mark.skipif(not G.available(), reason="the oracle (oracle/_ref) is not built: run __graft_entry__.build()")

DLL_MAX = 32769
GRID = [(k, m, bt) for k in (2, 3, 4, 5, 8, 16, 37, 512) for m in (1, 2, 3, 8, 128) for bt in (0.1, 0.25, 0.3, 0.49, 0.9)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return G.shim(tmp_path_factory.mktemp("gmsk_shim"))


def _kaiser(n, fc, As):
    As = abs(As)
    beta = 0.1102 * (As - 8.7) if As > 50 else (0.5842 * (As - 21) ** 0.4 + 0.07886 * (As - 21) if As > 21 else 0.0)
    t = np.arange(n) - (n - 1) / 2
    r = 2 * t / (n - 1)
    return np.sinc(2 * fc * t) * i0(beta * np.sqrt(np.maximum(0.0, 1 - r * r))) / i0(beta)


def _req_as(df, n):
    a0, a1 = 0.01, 200.0
    for _ in range(20):
        a = 0.5 * (a0 + a1)
        if float(int((a - 7.95) / (14.26 * df))) < n:
            a0 = a
        else:
            a1 = a
    return a


def definition(k, m, bt):
    """float64 liquid_firdes_gmsktx / liquid_firdes_gmskrx from their definitions (BT as the objects receive it: a float32)"""
    bt = float(np.float32(bt))
    n, km = 2 * k * m + 1, k * m
    t = np.arange(n) / k - m
    c0 = 1 / np.sqrt(np.log(2))
    q = lambda z: 0.5 * erfc(z / np.sqrt(2))
    tx = q(2 * np.pi * bt * (t - 0.5) * c0) - q(2 * np.pi * bt * (t + 0.5) * c0)
    tx *= np.pi / (2 * tx.sum()) * k
    hp, gp = _kaiser(n, 0.5 / k, _req_as(bt / k, n)), _kaiser(n, (0.7 + 0.1 * bt) / k, 60.0)
    Hp, Gp, Ht = (np.fft.fft(np.roll(h, -km)).real for h in (hp, gp, tx))
    H = (Hp - Hp.min() + 1e-3) / (Ht - Ht.min() + 1e-3) * (Gp - Gp.min()) / Gp[0]
    rx = np.roll(np.fft.ifft(H).real, km) * n / (k * n) * k * k
    return tx, rx


@pytest.mark.parametrize("k,m,bt", GRID)
def test_gmsk_taps_match_reference(ref, k, m, bt):
    n = G.h_len(k, m)
    tx, rx = K.product_taps(k, m, bt)
    dtx, drx = definition(k, m, bt)
    e_tx, e_rx = rel_err(tx.astype(np.float64), dtx), rel_err(rx.astype(np.float64), drx)
    if n > DLL_MAX:       # the binary's design keeps 80 h_len bytes on its stack: past this it overflows a thread's stack; the definition only
        assert e_tx <= 1e-6 and e_rx <= 1e-6, (e_tx, e_rx)
        return
    rtx, rrx = G.taps(ref, k, m, bt)
    for name, p, r, d, e_def in (("tx", tx, rtx, dtx, e_tx), ("rx", rx, rrx, drx, e_rx)):
        e_ref = rel_err(r.astype(np.float64), d)
        assert e_def <= e_ref + 1e-6, (name, e_def, e_ref)
        if n <= 4097 and e_ref <= 5e-6:
            assert rel_err(p, r) <= 1e-5, (name, rel_err(p, r), e_ref)


def test_gmsk_design_at_the_limits_is_fast():
    K.product_taps(2, 1, 0.3)             # (loads, and if need be builds, the library outside the timed call)
    t0 = time.perf_counter()
    K.product_taps(512, 128, 0.3)
    assert time.perf_counter() - t0 < 1.0


@pytest.mark.parametrize("k,m,bt", [(1, 3, 0.3), (0, 3, 0.3), (4, 0, 0.3), (4, 3, 0.0), (4, 3, 1.0), (4, 3, -0.5), (2, 1, 0.999), (2, 1, 1e-4),
                                    (512, 8, 0.3), (513, 1, 0.3), (4, 129, 0.3)])
def test_gmsk_refusals_match_gmskdem_create(ref, k, m, bt):
    import ctypes as C
    from cubicsdr_amd import build
    D = C.CDLL(build.build_design(verbose=False))
    D.csdr_design_gmsk.argtypes = [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int]
    n = max(1, 2 * k * m + 1)
    tx, rx = np.zeros(n, np.float32), np.zeros(n, np.float32)
    rc = D.csdr_design_gmsk(k, m, bt, tx.ctypes.data, rx.ctypes.data, n)
    if k > 512 or m > 128:
        assert rc == -1                   # the settings' wall
        return
    q = ref.shim_gmskdem_create(k, m, bt)
    if q:
        ref.shim_gmskdem_destroy(q)
    assert (rc == -1) == (not q) == G.refused(k, m, bt), (rc, bool(q))
