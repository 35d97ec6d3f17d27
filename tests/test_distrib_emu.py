"""The waterfall feed (kernels_distrib.hpp, csdr_distrib.hip) through the host-thread emulation of the HIP sources (tests/emu) against
oracle/fft_distributor.py, bit for bit: the shared cases of tests/distrib_cases.py with blocks given as host arrays and as pointers (which the
emulation reads as it reads device memory), aligned and one sample off a 16-byte boundary.  No GPU needed; the device runs the same cases in
tests/test_gpu_distrib.py."""
import ctypes as C
import os
import sys

import pytest

from tests import distrib_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))


@pytest.fixture(scope="module")
def ctx():
    import build_emu
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import Context
    path = build_emu.build(os.environ.get("CSDR_EMU_FLAVOR", ""))
    lib = C.CDLL(path)
    for name, (res, args) in H.ABI.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    saved = H._lib
    H._lib = lib
    c = Context(0)
    try:
        yield c
    finally:
        c.close()
        H._lib = saved


BLOCKS = [K.HostBlocks(), K.PointerBlocks(K.numpy_upload)]


def test_the_model_reaches_every_branch_over_the_grid():
    """what the shared grid covers, from the model alone (the figures the cases were chosen for)"""
    from oracle.fft_distributor import FFTDataDistributorRef
    most_lines, most_move_along, drops_at_2400, parities, straddles = 0, 0, [], set(), 0
    for fft in K.FFT_SIZES:
        for lps, rate in K.PACINGS:
            m = FFTDataDistributorRef(fft, lps)
            pos = move_along = drops = 0
            for n in K.CYCLE:
                pre = len(m.buf)
                out = m.push(list(range(pos, pos + n)), K.FREQ, rate)
                most_lines = max(most_lines, len(out))
                move_along += (not out) and not m.buf and pre + n >= fft
                drops += pre + n > m.buffer_max
                parities.add(len(m.buf) % 2)
                straddles += sum(1 for first, cnt, _, _ in out if first < pos < first + cnt)
                pos += n
            most_move_along = max(most_move_along, move_along)
            if rate == 2400:
                drops_at_2400.append(drops)
    assert most_lines == 128 and most_move_along == 32
    assert drops_at_2400 == [17, 17, 16, 6]              # per fft_size: bufferMax is 600, 600, 721 (1.2 * 601) and 2457 (1.2 * 2048) samples
    assert parities == {0, 1} and straddles > 100


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
@pytest.mark.parametrize("lps,rate", K.PACINGS)
@pytest.mark.parametrize("fft", K.FFT_SIZES)
def test_emu_grid(ctx, fft, lps, rate, blocks):
    st = K.run_plan(ctx, blocks, K.grid_plan(fft, lps, rate), seed=fft + lps)
    assert len(st["lines"]) == 40


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
def test_emu_retune(ctx, blocks):
    st = K.run_plan(ctx, blocks, K.retune_plan(), seed=2)
    assert sum(st["lines"]) > 40


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
def test_emu_fft_size_changes(ctx, blocks):
    st = K.run_plan(ctx, blocks, K.fft_change_plan(), seed=3)
    assert st["entered_full"] == 2                       # two pushes enter with bufferedItems >= fft_size


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
def test_emu_overflowing_pushes(ctx, blocks):
    st = K.run_plan(ctx, blocks, K.overflow_plan(), seed=4)
    assert st["dropped_pushes"] == 5 and sum(st["lines"]) == 5


@pytest.mark.parametrize("blocks", BLOCKS, ids=lambda b: b.name)
def test_emu_refused_range(ctx, blocks):
    K.check_refused_range(ctx, blocks)


def test_emu_refused_arguments(ctx):
    K.check_refused_arguments(ctx, BLOCKS[0])


def test_emu_odd_block_pointer(ctx):
    K.check_odd_block_pointer(ctx, BLOCKS[1])


def test_emu_previous_batch_survives_one_push(ctx):
    st = K.run_plan(ctx, BLOCKS[1], K.grid_plan(16, 5000, 48000), seed=8)
    assert st["previous_checked"] >= 20
