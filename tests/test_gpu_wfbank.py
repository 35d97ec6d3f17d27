"""The waterfall bank on the device: the cases the emulation runs (tests/wfbank_cases.py) against one PanelModel per slot and one csdr_waterfall per
slot, byte for byte, and what only the device path has -- csdr_wfbank_step_specbank behind a running pipeline with no host synchronisation between
the spectrum bank and the waterfall bank, and one shape at size (256 slots, fft_size 1024, 256 lines, thumbnails as one atlas)."""
import ctypes as C

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests import wfbank_cases as K
from tests.util import demod_frequencies, synth_iq
from tests.waterfall_cases import PanelModel, np_table
from tests.waterfall_view_cases import np_view

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_wfbank_life_cycle(ctx, fft_size):
    assert K.check_life_cycle(ctx, fft_size) == 6


@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_wfbank_one_item_per_call_and_interleavings(ctx, fft_size):
    K.check_one_item_per_call(ctx, fft_size)


@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_wfbank_slot_alone(ctx, fft_size):
    K.check_slot_alone(ctx, fft_size)


@pytest.mark.parametrize("fft_size", (30, 2048))
def test_wfbank_reset_slot(ctx, fft_size):
    K.check_reset_slot(ctx, fft_size)


def test_wfbank_setup_keeps_points(ctx):
    K.check_setup_keeps_points(ctx)


@pytest.mark.parametrize("fft_size", (2, 30, 2048))
def test_wfbank_refusals(ctx, fft_size):
    K.check_refusals(ctx, fft_size)


@pytest.mark.parametrize("mode", ["linear", "peak"])
@pytest.mark.parametrize("fft_size", K.VIEW_SIZES)
def test_wfbank_views(ctx, fft_size, mode):
    assert K.check_views(ctx, fft_size, mode) == 23


@pytest.mark.parametrize("fft_size", K.VIEW_SIZES)
def test_wfbank_view_properties(ctx, fft_size):
    K.check_view_properties(ctx, fft_size)


@pytest.mark.parametrize("fft_size", (30, 2048))
def test_wfbank_against_one_waterfall_per_slot(ctx, fft_size):
    K.check_against_waterfalls(ctx, fft_size)


def test_step_from_behind_a_pipeline(ctx):
    """2.4 MS/s, M = 4, blocks of 40 000, two per execute, six executes; NBFM, AM, USB, a QPSK slot and an inactive one; a SpectrumBank of F = 256.
    The pipeline runs twice on the same samples.  First the existing route: process_bank, then one csdr_waterfall per slot stepped where
    csdr_specbank_device_points lie, and PanelModel fed csdr_specbank_fetch.  Then the bank: process_bank, step_from, update and a render per
    execute with NO synchronising call in the loop -- none between process_bank and step_from, none between step_from and the next process_bank.
    Lines taken per execute, offsets, textures and tiles are the same, byte for byte."""
    from cubicsdr_amd.engine import DemodBank, SDRPost, SpectrumBank, Waterfall, WaterfallBank
    fs, M, block, center, nb, nexec, F, L = 2400000, 4, 40000, 100000000, 2, 6, 256, 8
    kinds = ["NBFM", "AM", "USB", "QPSK", "NBFM"]
    bws = [12500, 6000, 5400, 200000, 12500]
    freqs = demod_frequencies(center, fs, len(kinds))
    x = synth_iq(nexec * nb * block, fs, center, list(zip(["NBFM", "AM", "USB", "NBFM", "NBFM"], freqs)), seed=41)
    S = len(kinds)

    def pipeline():
        post = SDRPost(ctx, fs, M, block, nb)
        bank = DemodBank(ctx, S, nb)
        for i, k in enumerate(kinds):
            if k == "QPSK":
                bank.configure_digital(i, post, k, bws[i], freqs[i])
            else:
                bank.configure(i, post, k, bws[i], freqs[i])
        bank.set_active(4, False)
        return post, bank, SpectrumBank(ctx, F, 8, nb)    # (more slots than the bank has: the bank's count bounds the walk)
    lib = H.lib()
    wfs = [Waterfall(ctx, F, L, 16) for _ in range(S)]
    models = [PanelModel(F, L) for _ in range(S)]
    wb = WaterfallBank(ctx, F, L, S, 16)
    want, frames = [], []
    post, bank, sb = pipeline()
    try:
        for e in range(nexec):
            post.execute(x[e * nb * block:(e + 1) * nb * block], nb, block, center)
            bank.execute(post)
            sb.process_bank(bank)
            want.append(0)
            frames.append([sb.frames(s) for s in range(S)])
            for s in range(S):
                p, n = sb.device_points(s)
                assert n == frames[e][s]
                if n:
                    t = C.c_int()
                    H.check(lib.csdr_waterfall_step(wfs[s].h, C.c_void_p(p), 1, F, n, C.byref(t)))
                    want[e] += t.value
                    for j in range(n):
                        models[s].set_points(sb.fetch(s, j)[0])
                        models[s].step()
                wfs[s].update()
                models[s].update()
                if wfs[s].offset(0) >= 0:
                    wfs[s].fetch_index(0)                 # (this route's rule: the reader has finished before the next process)
    finally:
        for o in (sb, bank, post):
            o.close()
    post, bank, sb = pipeline()
    try:
        taken = []
        for e in range(nexec):
            post.execute(x[e * nb * block:(e + 1) * nb * block], nb, block, center)
            bank.execute(post)
            sb.process_bank(bank)
            taken.append(wb.step_from(sb))
            wb.update()
            wb.view(S, 16, 4, "linear", 2, fetch=False)
            assert [sb.frames(s) for s in range(S)] == frames[e], e
        assert taken == want and sum(want) >= 4 * (nexec - 1) * nb - 8
        for s in range(S):
            assert wb.offset(s, 0) == wfs[s].offset(0) == (models[s].ofs[0] if models[s].tex_init else -1), s
            if wfs[s].offset(0) >= 0:
                for j in range(2):
                    got = wb.fetch_index(s, j)
                    assert np.array_equal(got, wfs[s].fetch_index(j)) and np.array_equal(got, models[s].tex[j]), (s, j)
        for name in ("linear", "peak"):
            atlas = wb.view(S, 16, 4, name, 2)
            for s in range(S):
                tile = atlas[(s // 2) * 4:(s // 2 + 1) * 4, (s % 2) * 16:(s % 2 + 1) * 16]
                if wfs[s].offset(0) >= 0:
                    assert np.array_equal(tile, wfs[s].view(16, 4, name)) and np.array_equal(tile, np_view(models[s], np_table(), 16, 4, dict(K.MODES)[name])), (s, name)
                else:
                    assert not tile.any(), s
            assert not atlas[8:, 16:].any()
        assert wb.offset(4, 0) == -1 and wb.fetch_index(0, 0).any()
    finally:
        for o in wfs + [wb, sb, bank, post]:
            o.close()


def test_256_slots_at_size(ctx):
    """256 slots x fft_size 1024 x 256 lines (67 MB of textures); six turns of four lines per slot from a torch tensor, one line fewer in the slots
    that the turn's number divides so that the offsets diverge; 64 x 32 thumbnails as a 16-column atlas in both modes.  Eight slots against the
    model and against a second bank fed only those eight."""
    import torch
    from cubicsdr_amd.engine import WaterfallBank
    F, S, L, turns, per = 1024, 256, 256, 6, 4
    sampled = (0, 1, 63, 64, 127, 128, 200, 255)
    rng = np.random.default_rng(9)
    host = rng.uniform(-0.2, 1.2, (turns + 1, S, per, F)).astype(np.float32)
    host[:, :, :, 100] = 0.995
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()                              # (the tensor was made on torch's stream, the bank works on its own)
    full, few = WaterfallBank(ctx, F, L, S, 8), WaterfallBank(ctx, F, L, S, 8)
    models = {s: PanelModel(F, L) for s in sampled}
    try:
        for t in range(turns + 1):                        # (turn 0 is dropped everywhere and creates the textures)
            count = [per - (1 if t and s % (t + 1) == 0 else 0) for s in range(S)]
            items = [(s, dev[t, s, :count[s]], count[s]) for s in range(S)]
            got = full.step(items)
            assert got == ([0] * S if t == 0 else count)
            few.step([items[s] for s in sampled])
            full.update(); few.update()
            for s in sampled:
                for row in host[t, s, :count[s]]:
                    models[s].set_points(row)
                    models[s].step()
                models[s].update()
        assert len({full.offset(s, 0) for s in range(S)}) >= 4
        for s in sampled:
            assert full.offset(s, 0) == few.offset(s, 0) == models[s].ofs[0], s
            for j in range(2):
                a = full.fetch_index(s, j)
                assert np.array_equal(a, few.fetch_index(s, j)) and np.array_equal(a, models[s].tex[j]), (s, j)
        for name, mode in K.MODES:
            atlas = full.view(S, 64, 32, name, 16)
            part = few.view(list(sampled), 64, 32, name, 8)
            assert atlas.shape == (16 * 32, 16 * 64, 4)
            for k, s in enumerate(sampled):
                tile = atlas[(s // 16) * 32:(s // 16 + 1) * 32, (s % 16) * 64:(s % 16 + 1) * 64]
                assert np.array_equal(tile, part[:, k * 64:(k + 1) * 64]) and np.array_equal(tile, np_view(models[s], np_table(), 64, 32, mode)), (s, name)
    finally:
        full.close(); few.close()
