"""The view bank on the device: the cases the emulation runs (tests/viewbank_cases.py) against one RefSpectrum in view mode per slot, the bit-for-bit
properties and refusals, and what only the device path has -- csdr_viewbank_process_post behind a running channelizer against csdr_viewbank_process
fed host copies of the same rows, a slot's device points stepped into a waterfall bank where they lie, and one shape at size (256 slots, fftSize
1024, four row blocks of 2048 samples)."""
import ctypes as C

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests import viewbank_cases as K
from tests.specbank_cases import backend, check_frame, same_bytes
from tests.util import demod_frequencies, synth_iq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("F", K.SIZES)
def test_viewbank_against_the_model(ctx, F):
    n, worst = K.check_against_model(ctx, F)
    assert n == sum(K.expected_counts(F).values()) and worst < K.TOL


@pytest.mark.parametrize("F", K.PEAK_SIZES)
def test_viewbank_peak_hold(ctx, F):
    assert K.check_peak_hold(ctx, F) == 5 + 7 + 5


@pytest.mark.parametrize("F", (16, 256))
def test_viewbank_hide_dc(ctx, F):
    assert K.check_hide_dc(ctx, F) == 12


@pytest.mark.parametrize("F", (16, 32, 256, 2048))
def test_viewbank_properties(ctx, F):
    K.check_properties(ctx, F)


@pytest.mark.parametrize("F", (32, 256))
def test_viewbank_refusals(ctx, F):
    from cubicsdr_amd.engine import SDRPost
    post = SDRPost(ctx, 2400000, 4, 4096, 2)
    try:
        K.check_refusals(ctx, F, post)
    finally:
        post.close()


def _state(vb, s):
    return vb.slot_info(s), vb.fetch_last(s).tobytes()


def test_process_post_behind_a_pipeline(ctx):
    """2.4 MS/s, M = 4, blocks of 40 000, two per execute, six executes; four views of 200, 120, 60 and 500 kHz on three rows (two slots share
    one).  After every execute process_post equals, byte for byte, process fed host copies of the rows cut into the execute's blocks and stamped
    with the row's centre and the channel rate, and holds TOL against RefSpectrum on those samples; one slot's device points stepped into a
    waterfall bank (is_dev = 1) give the ring that the fetched points give."""
    from cubicsdr_amd.engine import SDRPost, ViewBank, WaterfallBank
    from oracle.cubicsdr_chain import RefSpectrum
    fs, M, block, center, nb, nexec, F = 2400000, 4, 40000, 100000000, 2, 6, 256
    freqs = demod_frequencies(center, fs, 4)
    x = synth_iq(nexec * nb * block, fs, center, list(zip(["NBFM", "AM", "USB", "NBFM"], freqs)), seed=43)
    post = SDRPost(ctx, fs, M, block, nb)
    rate, bc = post.channel_rate, block // M
    rows = [1, 2, 2, 3]
    bws = [200000, 120000, 60000, 500000]
    slots = [0, 1, 2, 5]
    dev, host = ViewBank(ctx, F, 6, nb, bc), ViewBank(ctx, F, 6, nb, bc)
    wa, wb = WaterfallBank(ctx, F, 16, 2), WaterfallBank(ctx, F, 16, 2)
    refs = [RefSpectrum(backend(), F) for _ in slots]
    lib = H.lib()
    frames = [0] * len(slots)
    try:
        assert rate == 600000
        centres = []
        for e in range(nexec):
            post.execute(x[e * nb * block:(e + 1) * nb * block], nb, block, center)
            if e == 0:                                   # (the rows' centres are known once the post has its frequency)
                for i, s in enumerate(slots):
                    centres.append(post.channel_center(rows[i]))
                    view = (centres[i] + (37000, 0, -52000, 90000)[i], bws[i])
                    for o in (dev, host):
                        o.set_view(s, *view)
                    refs[i].set_view(True, *view)
            dev.process_post(post, slots, rows)
            items, want = [], {i: [] for i in range(len(slots))}
            for i, s in enumerate(slots):
                row = post.read_channel(rows[i])
                assert row.size == nb * bc
                for b in range(nb):
                    cut = row[b * bc:(b + 1) * bc].copy()
                    items.append((s, cut, centres[i], rate))
                    w = refs[i].process_input(cut, centres[i], rate)
                    if w is not None:
                        want[i].append(w)
            host.process(items)
            for i, s in enumerate(slots):
                assert dev.frames(s) == host.frames(s) == len(want[i]), (e, s)
                assert _state(dev, s) == _state(host, s), (e, s)
                assert dev.slot_info(s)["desired_input_size"] == refs[i].desired_input_size and dev.slot_info(s)["resample_bw"] == refs[i].resample_bw
                for j in range(dev.frames(s)):
                    a, b = dev.fetch(s, j), host.fetch(s, j)
                    assert same_bytes([a + (None,)], [b + (None,)]), (e, s, j)
                    check_frame(a + (None,), want[i][j], (e, s, j))
                    frames[i] += 1
            assert dev.frames(3) == 0 and dev.frames(4) == 0
            # slot 0's points into a waterfall bank: where they lie, and fetched
            p, n = dev.device_points(0)
            if n:
                item = (H.WfBankItem * 1)()
                item[0].slot, item[0].n_floats_per_line, item[0].points, item[0].is_dev, item[0].n_lines = 1, F, p, 1, n
                taken = (C.c_int * 1)()
                H.check(lib.csdr_wfbank_step(wa.h, item, 1, taken))
                assert wb.step([(1, np.stack([host.fetch(0, j)[0][1::2] for j in range(n)]))]) == [taken[0]]
                wa.update(); wb.update()
                for h in range(2):
                    assert np.array_equal(wa.fetch_index(1, h), wb.fetch_index(1, h)), (e, h)     # (the fetch also ends the waterfall's reads before the next process)
        assert min(frames) >= nexec * nb - 2, frames
        assert wa.fetch_index(1, 0).any()
    finally:
        for o in (wa, wb, dev, host, post):
            o.close()


def test_256_slots_at_size(ctx):
    """256 slots, fftSize 1024, four row blocks of 2048 samples in one call, a view of 300 kHz on 503606 S/s off centre (ratio 1, mixing): eight
    sampled slots against the model, and those eight byte for byte against a second object fed only them"""
    from cubicsdr_amd.engine import ViewBank
    from oracle.cubicsdr_chain import RefSpectrum
    F, S, NI, B = 1024, 256, 4, 2048
    x = synth_iq(S * B + NI * B, float(K.RATE), K.FREQ, [("NBFM", K.FREQ + 55000.0), ("AM", K.FREQ - 90000.0)], seed=8)
    items = [(s, x[s * B + k * B:s * B + (k + 1) * B], K.FREQ, K.RATE) for k in range(NI) for s in range(S)]      # (overlapping cuts: every slot its own stream)
    sampled = (0, 1, 63, 64, 127, 128, 200, 255)
    full, few = ViewBank(ctx, F, S, NI, B), ViewBank(ctx, F, S, NI, B)
    try:
        for s in range(S):
            view = (K.FREQ + 20000 + 300 * s, 300000)
            full.set_view(s, *view)
            few.set_view(s, *view)
        full.process(items)
        few.process([it for it in items if it[0] in sampled])
        assert [full.frames(s) for s in range(S)] == [NI] * S
        assert [few.frames(s) for s in range(S)] == [NI if s in sampled else 0 for s in range(S)]
        for s in sampled:
            ref = RefSpectrum(backend(), F)
            ref.set_view(True, K.FREQ + 20000 + 300 * s, 300000)
            want = [w for w in (ref.process_input(it[1], K.FREQ, K.RATE) for it in items if it[0] == s) if w is not None]
            assert len(want) == NI
            assert _state(full, s) == _state(few, s)
            for j in range(NI):
                a, b = full.fetch(s, j), few.fetch(s, j)
                assert same_bytes([a + (None,)], [b + (None,)]), (s, j)
                check_frame(a + (None,), want[j], (s, j))
    finally:
        full.close(); few.close()
