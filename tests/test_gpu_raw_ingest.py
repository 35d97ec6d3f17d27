"""The native-sample-format ingest on the device: the conversion kernels over every component value and every tail length, the raw ring feeding the
channelizer and the spectrum, set_format, the refusals, and the C3 shape end to end -- each against the existing CF32 calls fed the header's
arithmetic restated in numpy (tests/raw_ingest_cases.py), bit for bit."""
import numpy as np
import pytest

from tests import raw_ingest_cases as K
from tests.util import demod_frequencies, synth_iq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_every_component_value(ctx, fmt):
    assert K.check_every_value(ctx, fmt) >= 10


@pytest.mark.parametrize("fmt", K.FORMATS)
def test_every_length(ctx, fmt):
    assert K.check_lengths(ctx, fmt) == 203


def test_cf32_passes_through(ctx):
    K.check_cf32_passes_through(ctx)


def test_ring_contents(ctx):
    K.check_ring_contents(ctx)


def test_ring_slot_tails(ctx):
    K.check_ring_slot_tails(ctx)


def test_full_scale_is_required(ctx):
    K.check_full_scale_is_required(ctx)


def test_set_format(ctx):
    K.check_set_format(ctx)


def test_refusals(ctx):
    K.check_refusals(ctx)


def quantise(fmt, x, amp):
    """complex64 samples -> the format's integers (I, Q), scaled so that `amp` reaches the format's full scale"""
    lo, hi = K.RANGE[fmt]
    mid = 128 if fmt == "CU8" else 0
    s = (hi - 1 - mid) / amp
    i = np.clip(np.round(x.real * s) + mid, lo, hi - 1).astype(np.int64)
    q = np.clip(np.round(x.imag * s) + mid, lo, hi - 1).astype(np.int64)
    return i, q


def test_raw_ring_feeds_channelizer_and_spectrum(ctx, fs=2400000, M=4, block=40000, nb=2, rounds=6, F=2048):
    """tests/test_gpu_io.py's ingest_scenario with raw slots: three slots rotating under back-to-back batches left in flight, swap alternating; CS16 and
    CU8 by commit, CS12 by upload_raw from an unaligned pageable buffer.  Channelizer rows and spectrum frames computed from the ingest's device pointer
    equal those of the existing CF32 calls fed the numpy-converted samples.  A set_format between rounds takes effect at the next commit, not before."""
    from cubicsdr_amd.engine import Ingest, SDRPost, SpectrumProcessor
    center = 100000000
    x = synth_iq(rounds * nb * block, fs, center, [("NBFM", center + 300000.0), ("AM", center - 500000.0)], seed=78)
    amp = float(np.max(np.abs(np.concatenate([x.real, x.imag])))) * 1.02
    for fmt, fs0, fs1, off, by_upload in [("CS16", 32768.0, 32767.0, 0.0, False), ("CU8", 128.0, 127.0, 127.4, False), ("CS12", 2048.0, 2047.0, 0.0, True)]:
        post_a = SDRPost(ctx, fs, M, block, max_blocks=nb); post_b = SDRPost(ctx, fs, M, block, max_blocks=nb)
        spec_a = SpectrumProcessor(ctx, F, max_frames=nb); spec_b = SpectrumProcessor(ctx, F, max_frames=nb)
        ing = Ingest(ctx, nb * block, depth=3, format=fmt, full_scale=fs0, offset=off)
        scale = fs0
        keep = []
        for r in range(rounds):
            xb = x[r * nb * block:(r + 1) * nb * block]
            swap = r % 2 == 1
            i, q = quantise(fmt, xb, amp)
            raw = K.pack(fmt, q, i) if swap else K.pack(fmt, i, q)      # the device delivers Q, I: the swap on the way restores I, Q
            if r == rounds // 2:
                ing.set_format(fmt, full_scale=fs1, offset=off)          # (the batches before it are still in flight with the old scale)
                scale = fs1
            want = K.np_convert(fmt, raw, scale, off, swap)
            if by_upload:
                src = K.unaligned_copy(raw)
                keep.append(src)
                dev = ing.upload_raw(src, xb.size, iq_swap=swap)
            else:
                K.fill(ing.acquire(), fmt, raw)
                dev = ing.commit(xb.size, iq_swap=swap)
            post_a.execute(dev, nb, block, center)
            spec_a.process(dev, nb, block)
            post_b.execute(want, nb, block, center)
            spec_b.process(want, nb, block)
            if r >= rounds - 2 or r == rounds // 2 - 1:          # (other rounds are left in flight: the slot rotation is exercised without host waits)
                for ch in range(M):
                    assert K.same_bits(post_a.read_channel(ch), post_b.read_channel(ch)), (fmt, r, ch)
                for k in range(nb):
                    assert K.same_bits(spec_a.fetch(k)[0], spec_b.fetch(k)[0]), (fmt, r, k)
                assert K.same_bits(K.download(ctx, dev), want), (fmt, r)
        ing.close(); spec_a.close(); spec_b.close(); post_a.close(); post_b.close()


def test_c3_shape_cs16_equals_cf32(ctx):
    """61.44 MS/s, M = 122, blocks of 1 024 068 samples, 36 mixed demodulators, the 65 536-point spectrum: CS16 through the raw ingest ->
    csdr_post_execute -> csdr_bank_execute -> csdr_spec_process gives audio, block results and spectrum frames byte-identical to the CF32 path fed
    the numpy-converted block."""
    from cubicsdr_amd.engine import DemodBank, Ingest, SDRPost, SpectrumProcessor
    fs, M, block, NB, nd, F = 61440000, 122, 1024068, 2, 36, 65536
    center = 100000000
    kinds = ["NBFM", "AM", "USB", "LSB", "FM", "CW"]
    bw = {"NBFM": 12500, "AM": 6000, "USB": 5400, "LSB": 5400, "FM": 200000, "CW": 700}
    freqs = demod_frequencies(center, fs, nd)
    x = synth_iq(NB * block, fs, center, [(("NBFM", "AM", "USB")[i % 3], f) for i, f in enumerate(freqs[:12])], seed=79)
    amp = float(np.max(np.abs(np.concatenate([x.real, x.imag])))) * 1.02
    i, q = quantise("CS16", x, amp)
    raw = K.pack("CS16", i, q)
    want = K.np_convert("CS16", raw, 32768.0)
    nframes = (NB * block) // (2 * F) + 2
    sides = []
    for raw_side in (True, False):
        post = SDRPost(ctx, fs, M, block, max_blocks=NB)
        bank = DemodBank(ctx, nd, max_blocks=NB)
        spec = SpectrumProcessor(ctx, F, max_frames=nframes)
        for k, f in enumerate(freqs):
            bank.configure(k, post, kinds[k % len(kinds)], bw[kinds[k % len(kinds)]], f)
        ing = None
        if raw_side:
            ing = Ingest(ctx, NB * block, depth=2, format="CS16", full_scale=32768.0)
            K.fill(ing.acquire(), "CS16", raw)
            src = ing.commit(NB * block)
        else:
            src = want
        post.execute(src, NB, block, center)
        bank.execute(post)
        nf = spec.process(src, NB, block, contiguous=True)
        res = [[bytes(r) for r in bank.results(k)] for k in range(nd)]
        audio = [bank.audio(k).copy() for k in range(nd)]
        frames = [spec.fetch(k)[0].copy() for k in range(nf)]
        sides.append((res, audio, frames))
        if ing:
            ing.close()
        spec.close(); bank.close(); post.close()
    (res_a, audio_a, frames_a), (res_b, audio_b, frames_b) = sides
    assert res_a == res_b
    assert sum(a.size for a in audio_a) > nd * 100
    for k in range(nd):
        assert K.same_bits(audio_a[k], audio_b[k]), k
    assert len(frames_a) == len(frames_b) and len(frames_a) >= (NB * block) // (2 * F)
    for k in range(len(frames_a)):
        assert K.same_bits(frames_a[k], frames_b[k]), k
