"""The spectrum bank on the device: the cases the emulation runs (tests/specbank_cases.py) against one RefSpectrum per slot, the bit-for-bit
properties and refusals, and what only the device path has -- csdr_specbank_process_bank behind a running pipeline against csdr_specbank_process fed
host copies of csdr_bank_fetch_iq, a slot's device points stepped into a waterfall where they lie, and one shape at size (256 slots, fftSize 1024)."""
import ctypes as C

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests import specbank_cases as K
from tests.util import demod_frequencies, synth_iq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("F", K.SIZES)
def test_specbank_against_the_model(ctx, F):
    n, worst = K.check_against_model(ctx, F)
    assert n == 10 + 11 + 12 + 11 + 0 + 11 and worst < K.TOL


@pytest.mark.parametrize("F", K.PEAK_SIZES)
def test_specbank_peak_hold(ctx, F):
    assert K.check_peak_hold(ctx, F) > 20


@pytest.mark.parametrize("F", (16, 32, 256, 2048))
def test_specbank_properties(ctx, F):
    K.check_properties(ctx, F)


@pytest.mark.parametrize("F", (32, 256))
def test_specbank_refusals(ctx, F):
    from cubicsdr_amd.engine import DemodBank
    bank = DemodBank(ctx, 2, 1)
    try:
        K.check_refusals(ctx, F, bank)
    finally:
        bank.close()


def test_process_bank_behind_a_pipeline(ctx):
    """2.4 MS/s, M = 4, blocks of 40 000, two per execute, six executes; NBFM, AM, USB, a QPSK slot and an inactive one.  After every execute
    process_bank equals, byte for byte, process fed host copies of csdr_bank_fetch_iq cut by csdr_block_result.n_iq, and holds TOL against
    RefSpectrum on those samples; the NBFM slot's device points stepped into a waterfall (is_dev = 1) give the ring that the fetched points give."""
    from cubicsdr_amd.engine import DemodBank, SDRPost, SpectrumBank, Waterfall
    from oracle.cubicsdr_chain import RefSpectrum
    fs, M, block, center, nb, nexec, F = 2400000, 4, 40000, 100000000, 2, 6, 256
    kinds = ["NBFM", "AM", "USB", "QPSK", "NBFM"]
    bws = [12500, 6000, 5400, 200000, 12500]
    freqs = demod_frequencies(center, fs, len(kinds))
    x = synth_iq(nexec * nb * block, fs, center, list(zip(["NBFM", "AM", "USB", "NBFM", "NBFM"], freqs)), seed=41)
    post = SDRPost(ctx, fs, M, block, nb)
    bank = DemodBank(ctx, len(kinds), nb)
    for i, k in enumerate(kinds):
        if k == "QPSK":
            bank.configure_digital(i, post, k, bws[i], freqs[i])
        else:
            bank.configure(i, post, k, bws[i], freqs[i])
    bank.set_active(4, False)
    dev, host = SpectrumBank(ctx, F, 8, nb), SpectrumBank(ctx, F, 8, nb)      # (more slots than the bank has: the bank's count bounds the walk)
    wa, wb = Waterfall(ctx, F, 8, 16), Waterfall(ctx, F, 8, 16)
    refs = [RefSpectrum(K.backend(), F) for _ in kinds]
    lib = H.lib()
    frames = [0] * len(kinds)
    try:
        for e in range(nexec):
            post.execute(x[e * nb * block:(e + 1) * nb * block], nb, block, center)
            bank.execute(post)
            dev.process_bank(bank)
            items, want = [], {i: [] for i in range(len(kinds))}
            for i in range(4):
                iq, at = bank.iq(i), 0
                for r in bank.results(i):
                    cut = iq[at:at + r.n_iq].copy()
                    at += r.n_iq
                    items.append((i, cut))
                    w = refs[i].process_input(cut)
                    if w is not None:
                        want[i].append(w)
                assert at == iq.size and at > 0
            host.process(items)
            for i in range(len(kinds)):
                assert dev.frames(i) == host.frames(i) == len(want[i]), (e, i)
                for j in range(dev.frames(i)):
                    a, b = dev.fetch(i, j), host.fetch(i, j)
                    assert K.same_bytes([a + (None,)], [b + (None,)]), (e, i, j)
                    K.check_frame(a + (None,), want[i][j], (e, i, j))
                    frames[i] += 1
            # the NBFM slot's points into a waterfall: where they lie, and fetched
            p, n = dev.device_points(0)
            if n:
                taken = C.c_int()
                H.check(lib.csdr_waterfall_step(wa.h, C.c_void_p(p), 1, F, n, C.byref(taken)))
                wb.step(np.stack([host.fetch(0, j)[0][1::2] for j in range(n)]))
                wa.update(); wb.update()
                for h in range(2):
                    assert np.array_equal(wa.fetch_index(h), wb.fetch_index(h)), (e, h)     # (the fetch also ends the waterfall's reads before the next process)
        assert frames[4] == 0 and frames[3] == nexec * nb and frames[0] >= nexec * nb - 2 and min(frames[:4]) > 0
        assert wa.fetch_index(0).any()
    finally:
        for o in (wa, wb, dev, host, bank, post):
            o.close()


def test_256_slots_at_size(ctx):
    """256 slots, fftSize 1024, 4 items of 208 +- 1 samples each in one call: eight sampled slots against the model, and those eight byte for byte
    against a second object fed only them"""
    from cubicsdr_amd.engine import SpectrumBank
    from oracle.cubicsdr_chain import RefSpectrum
    F, S, NI = 1024, 256, 4
    rng = np.random.default_rng(5)
    x = synth_iq(S * NI * 209, 48000.0, 0, [("NBFM", 5000.0), ("AM", -9000.0)], seed=6)
    items, at = [], 0
    for k in range(NI):
        for s in range(S):
            n = 208 + int(rng.integers(-1, 2))
            items.append((s, x[at:at + n]))
            at += n
    sampled = (0, 1, 63, 64, 127, 128, 200, 255)
    full, few = SpectrumBank(ctx, F, S, NI), SpectrumBank(ctx, F, S, NI)
    try:
        full.process(items)
        few.process([it for it in items if it[0] in sampled])
        assert [full.frames(s) for s in range(S)] == [NI - 1] * S
        assert [few.frames(s) for s in range(S)] == [NI - 1 if s in sampled else 0 for s in range(S)]
        for s in sampled:
            ref = RefSpectrum(K.backend(), F)
            want = [w for w in (ref.process_input(it[1]) for it in items if it[0] == s) if w is not None]
            for j in range(NI - 1):
                a, b = full.fetch(s, j), few.fetch(s, j)
                assert K.same_bytes([a + (None,)], [b + (None,)]), (s, j)
                K.check_frame(a + (None,), want[j], (s, j))
    finally:
        full.close(); few.close()
