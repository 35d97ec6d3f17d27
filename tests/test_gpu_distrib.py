"""The waterfall feed on the device, bit for bit against oracle/fft_distributor.py: the cases the emulation runs (tests/distrib_cases.py) with blocks
given as device pointers (torch tensors, aligned and one sample off a 16-byte boundary) and as host arrays, one shape large enough for the upper
grid dimensions, and the whole visual chain -- raw CS16 ingest -> push -> csdr_spec_process_distrib -> csdr_waterfall_step_spec -> update -- against
the same samples cut by the model on the host and fed through the calls that existed before."""
import numpy as np
import pytest

from tests import distrib_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    from cubicsdr_amd.engine import Context
    c = Context(0, torch.cuda.current_stream().cuda_stream)        # torch produces the device blocks: its stream is the boundary stream
    yield c
    c.close()


BLOCKS = [K.PointerBlocks(K.torch_upload), K.HostBlocks()]


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
@pytest.mark.parametrize("lps,rate", K.PACINGS)
@pytest.mark.parametrize("fft", K.FFT_SIZES)
def test_grid(ctx, fft, lps, rate, blocks):
    st = K.run_plan(ctx, blocks, K.grid_plan(fft, lps, rate), seed=fft + lps)
    assert len(st["lines"]) == 40


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
def test_retune(ctx, blocks):
    st = K.run_plan(ctx, blocks, K.retune_plan(), seed=2)
    assert sum(st["lines"]) > 40


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
def test_fft_size_changes(ctx, blocks):
    st = K.run_plan(ctx, blocks, K.fft_change_plan(), seed=3)
    assert st["entered_full"] == 2


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
def test_overflowing_pushes(ctx, blocks):
    st = K.run_plan(ctx, blocks, K.overflow_plan(), seed=4)
    assert st["dropped_pushes"] == 5 and sum(st["lines"]) == 5


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
def test_refused_range(ctx, blocks):
    K.check_refused_range(ctx, blocks)


def test_refused_arguments(ctx):
    K.check_refused_arguments(ctx, BLOCKS[1])


def test_odd_block_pointer(ctx):
    K.check_odd_block_pointer(ctx, BLOCKS[0])


def test_previous_batch_survives_one_push(ctx):
    st = K.run_plan(ctx, BLOCKS[0], K.grid_plan(16, 5000, 48000), seed=8)
    assert st["previous_checked"] >= 20


def test_large_lines(ctx):
    """fft 131072 at the heavy cadence: 65 workgroups along a line, lines that straddle the carry / block boundary, carries of 106 496 and 81 920 samples"""
    st = K.run_plan(ctx, BLOCKS[0], K.Plan([1024000] * 3, 131072, 1000, 61440000), max_lines=16, seed=11)
    assert st["lines"] == [7, 8, 8] and st["straddle"] == 2


def test_chain_raw_ingest_to_waterfall(ctx, fs=2400000, block=40000, nb=60, F=2048, lps=30, wf_lines=24):
    """Route A: raw CS16 ingest -> push -> csdr_spec_process_distrib -> csdr_waterfall_step_spec -> update, everything in HBM.  Route B, the calls that
    existed before: the numpy-widened samples cut by the model on the host, each push's lines concatenated and given to csdr_spec_process as one host
    call of the same n_blocks, then step_spec into a second panel.  Every fetched frame, both textures, the offsets and the picture are identical,
    and route A downloads no block."""
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import Context, Distributor, Ingest, SpectrumProcessor, Waterfall
    from oracle.fft_distributor import FFTDataDistributorRef
    from tests import raw_ingest_cases as R
    from tests.util import synth_iq
    center = 100000000
    x = synth_iq(nb * block, fs, center, [("NBFM", center + 250000.0), ("AM", center - 400000.0)], seed=19)
    s = 30000.0 / float(np.max(np.abs(np.concatenate([x.real, x.imag]))))
    raw = R.pack("CS16", np.round(x.real * s).astype(np.int64), np.round(x.imag * s).astype(np.int64))
    wide = R.np_convert("CS16", raw, 32768.0)
    own = Context(0)                                               # the ingest is the producer here: a context with a stream of its own
    lib = H.lib()
    downloads = []
    real_download = lib.csdr_dev_download

    def counting_download(*a):
        downloads.append(a)
        return real_download(*a)
    try:
        # route A
        ing = Ingest(own, block, depth=3, format="CS16", full_scale=32768.0)
        dist = Distributor(own, 8, 2 * F, lps)
        spec_a, wf_a = SpectrumProcessor(own, F, 4), Waterfall(own, F, wf_lines)
        assert spec_a.desired_input_size == 2 * F
        frames_a, counts = [], []
        lib.csdr_dev_download = counting_download
        for b in range(nb):
            R.fill(ing.acquire(), "CS16", raw[4 * b * block:4 * (b + 1) * block])
            dev = ing.commit(block)
            n = dist.push(dev, center, fs)
            assert dist.process_into(spec_a) == n
            counts.append(n)
            if n:
                wf_a.step_spec(spec_a, 0, n)
                wf_a.update()
                frames_a += [spec_a.fetch(f) for f in range(n)]
        assert not downloads
        lib.csdr_dev_download = real_download
        # route B
        model = FFTDataDistributorRef(2 * F, lps)
        spec_b, wf_b = SpectrumProcessor(own, F, 4), Waterfall(own, F, wf_lines)
        frames_b = []
        for b in range(nb):
            out = model.push(list(range(b * block, (b + 1) * block)), center, fs)
            assert len(out) == counts[b]
            if out:
                lines = np.concatenate([wide[first:first + cnt] for first, cnt, _, _ in out])
                assert spec_b.process(lines, len(out), 2 * F) == len(out)
                wf_b.step_spec(spec_b, 0, len(out))
                wf_b.update()
                frames_b += [spec_b.fetch(f) for f in range(len(out))]
        assert sum(counts) == 29 and len(frames_a) == len(frames_b) == 29       # 30 lines per second over one second, the first line due after 1 / 30 s
        for (pa, ca, fa), (pb, cb, fb) in zip(frames_a, frames_b):
            assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)) and ca == cb and fa == fb
        for half in (0, 1):
            assert np.array_equal(wf_a.fetch_index(half), wf_b.fetch_index(half)) and wf_a.offset(half) == wf_b.offset(half)
        assert wf_a.fetch_index(0).any()
        assert np.array_equal(wf_a.fetch_rgba(), wf_b.fetch_rgba())
        for o in (wf_a, wf_b, spec_a, spec_b, dist, ing):
            o.close()
    finally:
        lib.csdr_dev_download = real_download
        own.close()
