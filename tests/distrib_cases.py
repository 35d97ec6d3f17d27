"""Cases shared by tests/test_distrib_emu.py (the host-thread emulation) and tests/test_gpu_distrib.py (the device): csdr_distrib against
oracle/fft_distributor.py::FFTDataDistributorRef used as it stands, bit for bit.

The samples are random 64-bit patterns (an independent uint32 per component, so payload bits, NaNs and denormals included, are checked) and are
only ever compared as integers.  The model is fed the sample INDICES and reports the first id of every emitted line; the line must hold the
samples of the n ids that follow it in the model's buffer -- stream[id : id + n], except for a line that begins in samples carried from a block
whose tail was dropped: there the ids jump, and the expected line follows the model's buffered ids across the jump.  After every push: the line
count and every line, lineRateAccum (== on the double), bufferedItems, bufferOffset, bufferMax, the dropped samples, and the carried samples
themselves (fetch_buffered) against stream[model.buf].
"""
import ctypes as C

import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import DevicePointer, Distributor
from oracle.fft_distributor import FFTDataDistributorRef

CSDR_EINVAL, CSDR_ERANGE = -1, -5
CYCLE = [1, 7, 15, 16, 17, 1000, 1001, 33, 600, 601, 602, 5, 2047, 2048, 2049, 3, 1200, 31, 29, 30] * 2
FFT_SIZES = [16, 30, 601, 2048]
PACINGS = [(30, 48000), (1000, 48000), (30, 2400), (5000, 48000), (1, 48000)]          # (lines per second, sample rate)
FREQ = 100000000


def random_stream(n, seed):
    """n samples of random bits as complex64 (compare through bits())"""
    return np.random.default_rng(seed).integers(0, 1 << 32, 2 * n, dtype=np.uint32).view(np.complex64)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class HostBlocks:
    """blocks as host arrays (iq_is_dev = 0)"""
    name = "host"

    def __call__(self, x, odd):
        return np.array(x, copy=True)


class PointerBlocks:
    """blocks as device pointers over memory this class allocates with `alloc(n) -> (array-like holder, address)`; odd=True places the block one
    sample (8 bytes) off a 16-byte boundary"""
    name = "dev"

    def __init__(self, upload):
        self.upload = upload                   # (complex64 numpy array of n + 1 samples) -> (holder, address of sample 0), 16-byte aligned

    def __call__(self, x, odd):
        buf = np.empty(x.size + 1, np.complex64)
        buf[int(odd):int(odd) + x.size] = x
        holder, addr = self.upload(buf)
        assert addr % 16 == 0
        p = DevicePointer(addr + 8 * int(odd), x.size)
        p.holder = holder
        return p


def numpy_upload(buf):
    """the emulation's device memory is host memory: a 16-byte aligned numpy buffer stands for a device allocation"""
    raw = np.empty(buf.nbytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    al = raw[off:off + buf.nbytes].view(np.complex64)
    al[:] = buf
    return (raw, al), al.ctypes.data


def torch_upload(buf):
    import torch
    t = torch.from_numpy(buf.view(np.float32).copy()).cuda()
    return t, t.data_ptr()


def state_tuple(d):
    s = d.state
    return (s.line_rate_accum, s.buffered_items, s.buffer_offset, s.buffer_max, s.dropped, s.n_lines, s.line_len)


class Plan:
    """one push per entry: samples, and what changes IN FRONT of that push"""

    def __init__(self, lens, fft, lps, rate, freq=FREQ, changes=None):
        self.lens, self.fft, self.lps, self.rate, self.freq = list(lens), fft, lps, rate, freq
        self.changes = changes or {}           # push index -> dict(fft=, lps=, rate=, freq=)


def run_plan(ctx, blocks, plan, max_lines=256, seed=1, keep_previous=True):
    """-> statistics of the run (what the cases reached)"""
    stream = random_stream(sum(plan.lens), seed)
    model = FFTDataDistributorRef(plan.fft, plan.lps)
    d = Distributor(ctx, max_lines, plan.fft, plan.lps)
    fft, lps, rate, freq = plan.fft, plan.lps, plan.rate, plan.freq
    stats = dict(lines=[], move_along=0, dropped_pushes=0, carry_parity=set(), straddle=0, entered_full=0, previous_checked=0)
    pos = 0
    prev = None                                # (pointer, expected bits) of the previous push's batch
    try:
        for i, n in enumerate(plan.lens):
            ch = plan.changes.get(i, {})
            fft, lps, rate, freq = ch.get("fft", fft), ch.get("lps", lps), ch.get("rate", rate), ch.get("freq", freq)
            model.fft_size, model.lps = fft, lps
            d.set_fft_size(fft)
            d.set_lines_per_second(lps)
            reset = model.rate != rate or model.freq != freq
            pre_buf, pre_off = (0, 0) if reset else (len(model.buf), model.offset)
            stats["entered_full"] += pre_buf >= fft
            pre_ids = [] if reset else list(model.buf)
            out = model.push(list(range(pos, pos + n)), freq, rate)
            n_add = n                          # (:66-76 restated for the dropped count alone; the carried ids below check what was appended)
            if pre_off + pre_buf + n > model.buffer_max and pre_buf + n > model.buffer_max:
                n_add = model.buffer_max - pre_buf
            x = stream[pos:pos + n]
            got = d.push(blocks(x, i % 2 == 1), freq, rate)
            where = (i, n, fft, lps, rate)
            assert got == len(out), where
            s = d.state
            assert s.n_lines == len(out) and s.line_len == fft, where
            assert s.line_rate_accum == model.accum, (where, s.line_rate_accum, model.accum)
            assert (s.buffered_items, s.buffer_offset, s.buffer_max) == (len(model.buf), model.offset, model.buffer_max), where
            assert s.dropped == n - n_add, where
            lines = d.fetch_lines()
            assert lines.shape == (len(out), fft), where
            v_ids = np.array(pre_ids + list(range(pos, pos + n_add)), dtype=np.int64)      # the buffer the lines were cut from, as sample ids
            at = {int(first): int(np.searchsorted(v_ids, first)) for first, _, _, _ in out}
            assert all(v_ids[k] == first for first, k in at.items())
            want = np.stack([stream[v_ids[at[first]:at[first] + cnt]] for first, cnt, _, _ in out]) if out else np.empty((0, fft), np.complex64)
            assert all(cnt == fft and f == freq and r == rate for _, cnt, f, r in out)
            assert np.array_equal(bits(lines), bits(want)), (where, np.argwhere(bits(lines) != bits(want))[:4])
            carried = d.fetch_buffered()
            assert np.array_equal(bits(carried), bits(stream[np.array(model.buf, dtype=np.int64)] if model.buf else np.empty(0, np.complex64))), where
            # the previous batch's pointer still holds its lines after this further push
            if keep_previous and prev is not None and prev[1].size:
                back = np.empty(prev[1].size, np.uint64)
                H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(prev[0]), back.nbytes))
                assert np.array_equal(back, prev[1]), where
                stats["previous_checked"] += 1
            ptr, nl, ln = d.lines()
            assert (nl, ln) == (len(out), fft)
            prev = (ptr.ptr, bits(want).reshape(-1).copy())
            stats["lines"].append(len(out))
            stats["move_along"] += (not out) and pre_buf + n_add >= fft and not model.buf
            stats["dropped_pushes"] += n_add < n
            stats["carry_parity"].add(len(model.buf) % 2)
            stats["straddle"] += sum(1 for first, cnt, _, _ in out if first < pos < first + cnt)
            pos += n
    finally:
        d.close()
    return stats


def grid_plan(fft, lps, rate):
    return Plan(CYCLE, fft, lps, rate)


def retune_plan():
    return Plan(CYCLE, 30, 1000, 48000, changes={7: dict(freq=FREQ + 250000), 20: dict(rate=96000)})


def fft_change_plan():
    return Plan(CYCLE, 601, 1000, 48000, changes={6: dict(fft=16), 9: dict(fft=2048), 15: dict(fft=30), 25: dict(lps=3)})


def overflow_plan():
    return Plan([5000, 100, 2458, 2457, 3000, 1, 9000], 2048, 30, 2400)


def check_refused_range(ctx, blocks):
    """max_lines = 8 against the 2049-sample block at fft 16: CSDR_ERANGE with state, carry and previous batch untouched; a distributor with room takes it"""
    lens = [7, 33, 17, 300, 2049]
    stream = random_stream(sum(lens), 5)
    small, roomy = Distributor(ctx, 8, 16, 1000), Distributor(ctx, 256, 16, 1000)
    model = FFTDataDistributorRef(16, 1000)
    try:
        pos = 0
        for n in lens[:-1]:
            out = model.push(list(range(pos, pos + n)), FREQ, 48000)
            assert small.push(blocks(stream[pos:pos + n], False), FREQ, 48000) == len(out) <= 8
            assert roomy.push(blocks(stream[pos:pos + n], True), FREQ, 48000) == len(out)
            pos += n
        before, lines_before, carry_before = state_tuple(small), bits(small.fetch_lines()).copy(), bits(small.fetch_buffered()).copy()
        assert lines_before.size and carry_before.size
        ptr_before = small.lines()[0].ptr
        rc, got = small.try_push(blocks(stream[pos:], True), FREQ, 48000)
        assert rc == CSDR_ERANGE and got == 0
        assert state_tuple(small) == before
        assert small.lines()[0].ptr == ptr_before
        assert np.array_equal(bits(small.fetch_lines()), lines_before) and np.array_equal(bits(small.fetch_buffered()), carry_before)
        out = model.push(list(range(pos, pos + lens[-1])), FREQ, 48000)
        assert len(out) > 8
        assert roomy.push(blocks(stream[pos:], True), FREQ, 48000) == len(out)
        want = np.stack([stream[first:first + 16] for first, _, _, _ in out])
        assert np.array_equal(bits(roomy.fetch_lines()), bits(want))
        assert roomy.state.line_rate_accum == model.accum and roomy.state.buffered_items == len(model.buf)
        # the refused distributor goes on as if the block had never been offered
        rc, got = small.try_push(blocks(stream[pos:pos + 40], False), FREQ, 48000)
        assert rc == 0
    finally:
        small.close()
        roomy.close()


def check_refused_arguments(ctx, blocks):
    """each CSDR_EINVAL refusal leaves the state where it was"""
    lib = H.lib()
    d = Distributor(ctx, 16, 16, 30)
    try:
        stream = random_stream(100, 9)
        d.push(blocks(stream[:50], False), FREQ, 48000)
        before, carry = state_tuple(d), bits(d.fetch_buffered()).copy()
        assert lib.csdr_distrib_set_fft_size(d.h, 0) == CSDR_EINVAL and lib.csdr_distrib_set_fft_size(d.h, -5) == CSDR_EINVAL
        assert lib.csdr_distrib_set_lines_per_second(d.h, -1) == CSDR_EINVAL
        for rate in (0, -48000):
            assert d.try_push(blocks(stream[50:], False), FREQ, rate) == (CSDR_EINVAL, 0)
        assert d.try_push(blocks(stream[50:], False), FREQ, 48000, n_samples=-1) == (CSDR_EINVAL, 0)
        assert state_tuple(d) == before and np.array_equal(bits(d.fetch_buffered()), carry)
        # and the refused setters changed nothing: the next push still cuts 16-sample lines at 30 lines per second
        model = FFTDataDistributorRef(16, 30)
        model.push(list(range(50)), FREQ, 48000)
        out = model.push(list(range(50, 100)), FREQ, 48000)
        assert d.push(blocks(stream[50:], False), FREQ, 48000) == len(out) and d.state.line_len == 16 and d.state.line_rate_accum == model.accum
    finally:
        d.close()


def check_odd_block_pointer(ctx, pointer_blocks):
    """a device block one sample off a 16-byte boundary, with carries of both parities in front of it"""
    for first in (17, 18):
        plan = Plan([first, 1000, 1001, 64, 999], 16, 5000, 48000)
        stream_stats = run_plan(ctx, lambda x, odd: pointer_blocks(x, True), plan, seed=first)
        assert sum(stream_stats["lines"]) > 100 and stream_stats["straddle"] >= 1
