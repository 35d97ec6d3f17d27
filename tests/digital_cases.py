"""Parity cases of the digital decision kernel (csdr_digital_run) against the reference binary, shared by tests/test_digital_emu.py (the
host-thread emulation of the HIP sources) and tests/test_gpu_digital.py (the device)."""
import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import digital_run
from tests import digital_oracle as O

N_SAMPLES = 4096
BOUNDARY_SHARE = 1e-3


def noisy_points(lib, kind, cons, n, seed):
    """random symbols of the reference's own modulator plus complex noise of 0.1 x half the minimum distance"""
    rng = np.random.default_rng(seed)
    pts = O.constellation(lib, kind, cons)
    sig = 0.1 * O.min_distance(pts) / 2
    sym = rng.integers(0, cons, n).astype(np.uint32)
    if kind == "DPSK":
        m = O.Modem(lib, kind, cons)
        x = m.modulate(sym)
        m.close()
    else:
        x = pts[sym]
    noise = sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    return (x + noise).astype(np.complex64)


def uniform_plane(n, seed, span=1.6):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-span, span, n) + 1j * rng.uniform(-span, span, n)).astype(np.complex64)


def evm_close(got, want):
    return abs(got - want) <= 1e-6 + 1e-5 * abs(want)


def check_constellation(ctx, lib, kind, cons, seed=7):
    """noisy points: every decision and the last-sample EVM; then a run continued from the returned state (DPSK's carried phase, the kept
    r / x_hat); uniform points: mismatches only on the reference's own decision boundaries, at most 0.1 %"""
    x = noisy_points(lib, kind, cons, N_SAMPLES, seed)
    ref = O.Modem(lib, kind, cons)
    half = N_SAMPLES // 2
    want1, want2 = ref.demodulate(x[:half]), None
    e1 = ref.evm()
    want2 = ref.demodulate(x[half:])
    e2 = ref.evm()
    ref.close()
    got1, g1, st = digital_run(ctx, kind, x[:half], 200000, cons=cons)
    got2, g2, st = digital_run(ctx, kind, x[half:], 200000, state=st, cons=cons)
    assert np.array_equal(got1, want1), (kind, cons, np.nonzero(got1 != want1)[0][:8])
    assert np.array_equal(got2, want2), (kind, cons, np.nonzero(got2 != want2)[0][:8])
    assert evm_close(g1, e1) and evm_close(g2, e2), (kind, cons, g1, e1, g2, e2)
    # an empty run reports the object's EVM again (the reference's state is not touched by a block without samples)
    got0, g0, st = digital_run(ctx, kind, np.zeros(0, np.complex64), 200000, state=st, cons=cons)
    assert got0.size == 0 and evm_close(g0, e2)
    u = uniform_plane(N_SAMPLES, seed + 1)
    ref = O.Modem(lib, kind, cons)
    want, _ = ref.demodulate(u, evm_each=True)
    ref.close()
    got, _, _ = digital_run(ctx, kind, u, 200000, cons=cons)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        edge = O.boundary_mask(lib, kind, cons, u, want)
        assert edge[bad].all(), (kind, cons, bad[~edge[bad]][:8], u[bad[~edge[bad]][:4]])
    assert bad.size <= BOUNDARY_SHARE * u.size, (kind, cons, bad.size)
    return bad.size


def fsk_tones(lib, bps, k, bw, n_sym, seed, noise=0.7):
    """n_sym symbols of k samples: the tone of a random symbol on its transform bin plus noise"""
    q = O.fsk_create(lib, bps, k, bw)
    assert q
    lib.shim_fsk_destroy(q)
    rng = np.random.default_rng(seed)
    M = 1 << bps
    M2 = 0.5 * (M - 1)
    syms = rng.integers(0, M, n_sym)
    t = np.arange(k)
    freq = (syms - M2) * bw / M2
    sig = np.exp(2j * np.pi * freq[:, None] * t[None, :]).reshape(-1)
    z = sig + noise * (rng.standard_normal(sig.size) + 1j * rng.standard_normal(sig.size)) / np.sqrt(2)
    return z.astype(np.complex64)


def check_fsk(ctx, lib, bps, k, bw, seed=11, n_sym=160):
    """whole symbols against fskdem_demodulate, with the stream cut into pieces that leave samples to carry"""
    x = fsk_tones(lib, bps, k, bw, n_sym, seed)
    x = x[: x.size - k // 2]                      # a part symbol at the end stays in the carry
    q = O.fsk_create(lib, bps, k, bw)
    want = O.fsk_symbols(lib, q, x, k)
    lib.shim_fsk_destroy(q)
    rate = k * 1000
    rng = np.random.default_rng(seed + 1)
    cuts = np.sort(rng.choice(np.arange(1, x.size), size=6, replace=False))
    st, got = None, []
    for a, b in zip(np.r_[0, cuts], np.r_[cuts, x.size]):
        s, evm, st = digital_run(ctx, "FSK", x[a:b], rate, state=st, bps=bps, sps=1000, bw=bw)
        assert evm == 0.0
        got.append(s)
    got = np.concatenate(got)
    assert st.n_carry == x.size % k
    np.testing.assert_array_equal(np.asarray(st.carry[: 2 * st.n_carry], np.float32), x[x.size - st.n_carry:].view(np.float32))
    assert np.array_equal(got, want), (bps, k, bw, np.nonzero(got != want)[0][:8])


FSK_CASES = [(1, 2, 0.45), (1, 16, 0.45), (1, 5, 0.1), (2, 8, 0.3), (2, 13, 0.45), (4, 16, 0.45), (4, 37, 0.2), (4, 100, 0.4),
             (4, 8, 0.45), (2, 3, 0.45), (3, 6, 0.45)]          # the last three: fewer samples per symbol than tones (ModemFSK's 2 bps sps rate)
# settings without a demodulator: fskdem_create returns none (k < 2, k > 2048, bw outside (0, 0.5)) or its bin map is not unique
FSK_REFUSED = [(1, 1, 0.45), (1, 2049, 0.45), (2, 16, 0.5), (2, 16, -0.1), (2, 16, 0.0001), (4, 16, 0.01), (16, 2048, 0.45)]


def check_fsk_refused(ctx, lib, capfd, bps, k, bw):
    """the reference binary builds no usable demodulator for these settings (no object, or it reports a bin map that is not unique), and the
    library refuses them with CSDR_EUNSUPPORTED"""
    capfd.readouterr()
    q = O.fsk_create(lib, bps, k, bw)
    msg = capfd.readouterr().err
    if q:
        lib.shim_fsk_destroy(q)
    assert not q or "not unique" in msg, (bps, k, bw, msg)
    d = H.DigitalParams(H.CSDR_DIGITAL_FSK, 0, bps, 1000, bw)
    st = H.DigitalState()
    n = C_int()
    x = np.zeros(4 * k, np.complex64)
    out = np.zeros(4 * k, np.uint32)
    rc = H.lib().csdr_digital_run(ctx.h, d, k * 1000, x.ctypes.data, x.size, st, out.ctypes.data, out.size, n, None)
    assert rc == -6, (bps, k, bw, rc)


def C_int():
    import ctypes
    return ctypes.c_int()


def check_configure_routes(ctx):
    """csdr_bank_configure_slot refuses CSDR_MODEM_DIGITAL (EINVAL, naming the digital call); the digital call refuses what the reference cannot
    build (EUNSUPPORTED) and a non-digital modem (EINVAL)"""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    post = SDRPost(ctx, 2400000, 4, 40000, 1)
    bank = DemodBank(ctx, 2, 1)
    try:
        l = H.lib()
        p = H.DemodParams(H.CSDR_MODEM_DIGITAL, 200000, 48000, 0, 100000000)
        assert l.csdr_bank_configure_slot(bank.h, 0, p, post.h) == -1
        assert b"csdr_bank_configure_digital_slot" in l.csdr_last_error()
        for kind, cons in (("PSK", 3), ("QAM", 2), ("ASK", 512)):
            d = H.DigitalParams(H.DIGITAL_BY_NAME[kind], cons, 0, 0, 0.0)
            assert l.csdr_bank_configure_digital_slot(bank.h, 0, p, d, post.h) == -6, (kind, cons)
        d = H.DigitalParams(H.CSDR_DIGITAL_FSK, 0, 2, 9600, 0.6)
        assert l.csdr_bank_configure_digital_slot(bank.h, 0, p, d, post.h) == -6
        q = H.DemodParams(H.CSDR_MODEM_NBFM, 12500, 48000, 0, 100000000)
        assert l.csdr_bank_configure_digital_slot(bank.h, 0, q, H.DigitalParams(0, 2, 0, 0, 0.0), post.h) == -1
        bank.configure_digital(1, post, "PSK", 200000, 100000000, cons=8)
        assert l.csdr_bank_set_digital_cons(bank.h, 1, 8) == 0 and l.csdr_bank_set_digital_cons(bank.h, 1, 6) == -6
    finally:
        bank.close()
        post.close()
