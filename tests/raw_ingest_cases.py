"""Scenarios of the native-sample-format ingest (CS16, CS8, CU8, CS12 widened to complex64 on the GPU), shared by the host-thread emulation
(tests/test_raw_ingest_emu.py) and the device (tests/test_gpu_raw_ingest.py).

The specification is include/csdr_hip.h's: every component is y = ((float)x - offset) * s with s = (float)(1.0 / full_scale), the difference and the
product each rounded once in float32.  `np_convert` restates exactly that; every comparison is np.array_equal on the uint32 view -- no tolerance."""
import ctypes as C

import numpy as np

import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import Ingest, iq_convert, iq_format, pack_cs12

FORMATS = ["CS16", "CS8", "CU8", "CS12"]
FULL_SCALES = [32768.0, 32767.0, 2048.0, 128.0, 127.0]           # powers of two and reciprocals that are not
CU8_OFFSETS = [128.0, 127.5, 127.4]
BYTES = {"CF32": 8, "CS16": 4, "CS8": 2, "CU8": 2, "CS12": 3}
RANGE = {"CS16": (-32768, 32768), "CS8": (-128, 128), "CU8": (0, 256), "CS12": (-2048, 2048)}
DTYPE = {"CS16": np.int16, "CS8": np.int8, "CU8": np.uint8}
LARGE = [1024068 + 1, 1024068 + 3, 999983]                         # odd block lengths around the C3 block


def pack(fmt, i, q):
    """integer component arrays -> the format's byte stream (uint8)"""
    if fmt == "CS12":
        return pack_cs12(i, q)
    a = np.empty((len(i), 2), DTYPE[fmt])
    a[:, 0] = i
    a[:, 1] = q
    return a.reshape(-1).view(np.uint8)


def components(fmt, raw):
    """the format's byte stream -> (I, Q) as int32, decoded independently of pack()"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    if fmt == "CS12":
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        i, q = v & 0xFFF, v >> 12
        return i - ((i & 0x800) << 1), q - ((q & 0x800) << 1)
    a = raw.view(DTYPE[fmt]).reshape(-1, 2).astype(np.int32)
    return a[:, 0], a[:, 1]


def np_convert(fmt, raw, full_scale, offset=0.0, swap=False):
    """the header's arithmetic in numpy: (x.astype(np.float32) - np.float32(offset)) * np.float32(1.0 / full_scale)"""
    i, q = components(fmt, raw)
    s = np.float32(1.0 / full_scale)
    out = np.empty((i.size, 2), np.float32)
    out[:, 0] = (i.astype(np.float32) - np.float32(offset)) * s
    out[:, 1] = (q.astype(np.float32) - np.float32(offset)) * s
    if swap:
        out = out[:, ::-1]
    return np.ascontiguousarray(out).view(np.complex64).reshape(-1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def random_raw(fmt, n, rng):
    lo, hi = RANGE[fmt]
    return pack(fmt, rng.integers(lo, hi, n), rng.integers(lo, hi, n))


def offsets_of(fmt):
    return CU8_OFFSETS if fmt == "CU8" else [0.0]


def convert_guarded(ctx, fmt, raw, n, full_scale, offset, swap):
    """csdr_iq_convert into the front of a longer host array: the samples, and a check that what lies behind them was left alone (the call itself
    checks the guard band behind its device output)"""
    f = iq_format(fmt, full_scale, offset)
    out = np.full(n + 16, np.float32(-7.25) + 1j * np.float32(3.5), np.complex64)
    a = np.ascontiguousarray(raw)
    H.check(H.lib().csdr_iq_convert(ctx.h, C.byref(f), a.ctypes.data_as(C.c_void_p), n, int(swap), out.ctypes.data_as(C.c_void_p)))
    assert np.all(out[n:] == np.complex64(-7.25 + 3.5j)), "host guard band"
    return out[:n]


# ---------------------------------------------------------------------------------------------- 1. the kernel alone
def check_every_value(ctx, fmt):
    """every representable component value in the I and in the Q position, for every full scale (and CU8 offset), swap off and on"""
    lo, hi = RANGE[fmt]
    v = np.arange(lo, hi)
    rng = np.random.default_rng(5)
    i = np.concatenate([v, rng.permutation(v)[:37]])            # (37 more: the length is not a multiple of any lane grouping)
    q = np.concatenate([v[::-1], rng.permutation(v)[:37]])
    q = np.roll(q, 11)
    raw = pack(fmt, i, q)
    ci, cq = components(fmt, raw)
    assert set(ci.tolist()) == set(v.tolist()) and set(cq.tolist()) == set(v.tolist())
    runs = 0
    for fs in FULL_SCALES:
        for off in offsets_of(fmt):
            for swap in (False, True):
                got = convert_guarded(ctx, fmt, raw, i.size, fs, off, swap)
                want = np_convert(fmt, raw, fs, off, swap)
                assert same_bits(got, want), (fmt, fs, off, swap, int(np.sum(got.view(np.uint32) != want.view(np.uint32))))
                runs += 1
    return runs


def check_lengths(ctx, fmt, lengths=None):
    """every length 1 .. 200 and a few large odd ones: every tail of every lane grouping, the first sample past the end untouched"""
    rng = np.random.default_rng(6)
    lengths = list(range(1, 201)) + LARGE if lengths is None else lengths
    for k, n in enumerate(lengths):
        raw = random_raw(fmt, n, rng)
        fs = FULL_SCALES[k % len(FULL_SCALES)]
        off = offsets_of(fmt)[k % len(offsets_of(fmt))]
        swap = (k // 2) % 2 == 1
        got = convert_guarded(ctx, fmt, raw, n, fs, off, swap)
        assert same_bits(got, np_convert(fmt, raw, fs, off, swap)), (fmt, n, fs, off, swap)
    return len(lengths)


def check_cf32_passes_through(ctx):
    """CF32 is accepted so that callers have one code path: the samples come back as they are, or exchanged"""
    rng = np.random.default_rng(8)
    x = (rng.standard_normal(2 * 777).astype(np.float32)).view(np.complex64)
    assert same_bits(iq_convert(ctx, x, "CF32"), x)
    assert same_bits(iq_convert(ctx, x, "CF32", iq_swap=True), (x.imag + 1j * x.real).astype(np.complex64))


# ---------------------------------------------------------------------------------------------- 2. the ring
def download(ctx, dev):
    out = np.empty(dev.n, np.complex64)
    H.check(H.lib().csdr_dev_download(ctx.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(dev.ptr), out.nbytes))
    return out


def fill(slot, fmt, raw):
    slot.reshape(-1).view(np.uint8)[:raw.size] = raw


def unaligned_copy(raw):
    """the same bytes in pageable memory at an odd address"""
    buf = np.empty(raw.size + 64, np.uint8)
    off = 1 + (-buf.ctypes.data) % 16                             # address % 16 == 1
    view = buf[off:off + raw.size]
    view[:] = raw
    assert view.ctypes.data % 16 == 1
    return view


def check_ring_contents(ctx, n=3001, rounds=8):
    """three slots rotating: each commit's device pointer holds the conversion of ITS block while earlier ones are still valid (depth - 1 further
    commits), the pointers cycle through three addresses, CS16 / CU8 by commit and CS12 by upload_raw from an unaligned pageable buffer"""
    rng = np.random.default_rng(9)
    for fmt, fs, off, by_upload in [("CS16", 32768.0, 0.0, False), ("CU8", 128.0, 127.4, False), ("CS12", 2048.0, 0.0, True), ("CS8", 127.0, 0.0, False)]:
        ing = Ingest(ctx, n, depth=3, format=fmt, full_scale=fs, offset=off)
        live = []
        ptrs = []
        for r in range(rounds):
            m = n - (r % 3) * 7
            raw = random_raw(fmt, m, rng)
            swap = r % 2 == 1
            if by_upload:
                dev = ing.upload_raw(unaligned_copy(raw), m, iq_swap=swap)
            else:
                fill(ing.acquire(), fmt, raw)
                dev = ing.commit(m, iq_swap=swap)
            ptrs.append(dev.ptr)
            live = (live + [(dev, np_convert(fmt, raw, fs, off, swap))])[-3:]      # valid until depth - 1 further commits
            for d, want in live:
                assert same_bits(download(ctx, d), want), (fmt, r)
        assert len(set(ptrs)) == 3 and ptrs[:3] == ptrs[3:6]
        ing.close()


def check_ring_slot_tails(ctx, cap=1000):
    """a block shorter than the slot leaves the rest of the HBM slot alone: every slot is filled with a pattern through its device pointer before
    the transfer, and all `cap` samples are read back after it; every format, by commit and by upload_raw, lengths that end inside every lane group"""
    rng = np.random.default_rng(13)
    mark = np.full(cap, np.float32(-3.0e38) + 1j * np.float32(1.5e-38), np.complex64)
    for fmt, fs, off in [("CS16", 32767.0, 0.0), ("CS8", 128.0, 0.0), ("CU8", 127.0, 127.5), ("CS12", 2048.0, 0.0)]:
        ing = Ingest(ctx, cap, depth=3, format=fmt, full_scale=fs, offset=off)
        ptrs = []
        for _ in range(3):                                          # one turn of the ring: the three device slots
            ing.acquire()
            ptrs.append(ing.commit(1).ptr)
        assert len(set(ptrs)) == 3
        for r, m in enumerate([cap - 1, cap - 17, 5, 1, cap - 8, 16, 33, cap // 2 + 3, cap]):
            k = ing.next_slot()
            H.check(H.lib().csdr_dev_upload(ctx.h, C.c_void_p(ptrs[k]), mark.ctypes.data_as(C.c_void_p), mark.nbytes))
            raw = random_raw(fmt, m, rng)
            swap = r % 2 == 1
            if r % 3 == 2:
                dev = ing.upload_raw(unaligned_copy(raw), m, iq_swap=swap)
            else:
                fill(ing.acquire(), fmt, raw)
                dev = ing.commit(m, iq_swap=swap)
            assert dev.ptr == ptrs[k]
            got = download(ctx, type(dev)(dev.ptr, cap))
            assert same_bits(got[:m], np_convert(fmt, raw, fs, off, swap)), (fmt, m)
            assert same_bits(got[m:], mark[m:]), (fmt, m, "the slot behind the block was written")
        ing.close()


def check_full_scale_is_required(ctx):
    """the Python side refuses an integer format without the radio's full scale instead of assuming one"""
    import pytest
    for fmt in FORMATS:
        with pytest.raises(ValueError):
            iq_format(fmt)
        with pytest.raises(ValueError):
            Ingest(ctx, 16, format=fmt)
    assert iq_format("CF32").format == H.CSDR_IQ_CF32


def check_set_format(ctx, n=1500):
    """set_format between blocks: the block committed before it keeps its conversion, the next one has the new one"""
    rng = np.random.default_rng(10)
    ing = Ingest(ctx, n, depth=3, format="CS16", full_scale=32768.0)
    raw_a = random_raw("CS16", n, rng)
    fill(ing.acquire(), "CS16", raw_a)
    dev_a = ing.commit(n)
    ing.set_format("CS16", full_scale=2048.0)                       # a 12-bit radio that delivers sign-extended int16
    assert same_bits(download(ctx, dev_a), np_convert("CS16", raw_a, 32768.0))
    raw_b = random_raw("CS16", n, rng)
    fill(ing.acquire(), "CS16", raw_b)
    dev_b = ing.commit(n, iq_swap=True)
    assert same_bits(download(ctx, dev_b), np_convert("CS16", raw_b, 2048.0, 0.0, True))
    assert same_bits(download(ctx, dev_a), np_convert("CS16", raw_a, 32768.0))
    ing.set_format("CU8", full_scale=128.0, offset=127.5)           # smaller samples fit the slots
    raw_c = random_raw("CU8", n, rng)
    slot = ing.acquire()
    assert slot.dtype == np.uint8 and slot.shape == (n, 2)
    fill(slot, "CU8", raw_c)
    dev_c = ing.commit(n)
    assert same_bits(download(ctx, dev_c), np_convert("CU8", raw_c, 128.0, 127.5))
    ing.set_format("CS12", full_scale=2048.0)
    raw_d = random_raw("CS12", n, rng)
    dev_d = ing.upload_raw(raw_d, n)
    assert same_bits(download(ctx, dev_d), np_convert("CS12", raw_d, 2048.0))
    ing.close()


# ---------------------------------------------------------------------------------------------- 3. refusals
EINVAL, ESTATE, ERANGE = -1, -4, -5


def check_refusals(ctx):
    L = H.lib()
    n = 64
    raw = np.zeros(8 * n, np.uint8)
    out = np.zeros(n, np.complex64)
    h = C.c_void_p()
    p = C.c_void_p()

    def fmt(format, fs, off=0.0):
        return H.IqFormat(int(format), float(off), float(fs))
    bad = [fmt(5, 128.0), fmt(-1, 128.0), fmt(H.CSDR_IQ_CS16, 0.0), fmt(H.CSDR_IQ_CS16, -32768.0), fmt(H.CSDR_IQ_CS16, float("inf")),
           fmt(H.CSDR_IQ_CS16, float("nan")), fmt(H.CSDR_IQ_CU8, 128.0, float("nan")), fmt(H.CSDR_IQ_CU8, 128.0, float("inf")),
           fmt(H.CSDR_IQ_CS16, 32768.0, 1.0), fmt(H.CSDR_IQ_CS8, 128.0, 0.5), fmt(H.CSDR_IQ_CS12, 2048.0, -1.0)]
    good = fmt(H.CSDR_IQ_CS16, 32768.0)
    for f in bad:
        assert L.csdr_iq_convert(ctx.h, C.byref(f), raw.ctypes.data_as(C.c_void_p), n, 0, out.ctypes.data_as(C.c_void_p)) == EINVAL, (f.format, f.full_scale, f.offset)
        assert L.csdr_ingest_create_raw(ctx.h, n, 3, C.byref(f), C.byref(h)) == EINVAL and not h.value
    assert L.csdr_iq_convert(ctx.h, C.byref(good), raw.ctypes.data_as(C.c_void_p), 0, 0, out.ctypes.data_as(C.c_void_p)) == EINVAL
    assert L.csdr_ingest_create_raw(ctx.h, n, 3, None, C.byref(h)) == EINVAL
    assert L.csdr_ingest_create_raw(ctx.h, n, 1, C.byref(good), C.byref(h)) == EINVAL
    b = C.c_uint64()
    for name, per in BYTES.items():
        assert L.csdr_iq_format_bytes(H.IQ_FORMAT_BY_NAME[name], 1000, C.byref(b)) == 0 and b.value == 1000 * per
    assert L.csdr_iq_format_bytes(9, 1000, C.byref(b)) == EINVAL

    # a raw ingest refuses the typed calls, a typed one the raw calls; neither moves the ring
    rawi = Ingest(ctx, n, depth=3, format="CS16", full_scale=32768.0)
    typed = Ingest(ctx, n, depth=3)
    x = np.zeros(n, np.complex64)
    assert L.csdr_ingest_acquire(rawi.h, C.byref(p)) == ESTATE
    assert L.csdr_ingest_commit(rawi.h, n, 0, C.byref(p)) == ESTATE
    assert L.csdr_ingest_upload(rawi.h, x.ctypes.data_as(C.c_void_p), n, 0, C.byref(p)) == ESTATE
    assert L.csdr_ingest_acquire_raw(typed.h, C.byref(p)) == ESTATE
    assert L.csdr_ingest_commit_raw(typed.h, n, 0, C.byref(p)) == ESTATE
    assert L.csdr_ingest_upload_raw(typed.h, raw.ctypes.data_as(C.c_void_p), n, 0, C.byref(p)) == ESTATE
    assert L.csdr_ingest_set_format(typed.h, C.byref(good)) == ESTATE
    assert rawi.next_slot() == 0 and typed.next_slot() == 0

    # one good commit, then refusals: the ring stays at slot 1 and the next commit uses it
    rng = np.random.default_rng(12)
    raw0 = random_raw("CS16", n, rng)
    fill(rawi.acquire(), "CS16", raw0)
    dev0 = rawi.commit(n)
    assert rawi.next_slot() == 1
    assert L.csdr_ingest_commit_raw(rawi.h, n, 0, C.byref(p)) == ESTATE                       # commit without acquire
    assert L.csdr_ingest_upload_raw(rawi.h, raw.ctypes.data_as(C.c_void_p), n + 1, 0, C.byref(p)) == ERANGE
    assert L.csdr_ingest_upload_raw(rawi.h, raw.ctypes.data_as(C.c_void_p), 0, 0, C.byref(p)) == ERANGE
    assert L.csdr_ingest_upload_raw(rawi.h, None, n, 0, C.byref(p)) == EINVAL
    for f in bad:
        assert L.csdr_ingest_set_format(rawi.h, C.byref(f)) == EINVAL
    big = fmt(H.CSDR_IQ_CF32, 1.0)
    assert L.csdr_ingest_set_format(rawi.h, C.byref(big)) == EINVAL                            # 8-byte samples do not fit 4-byte slots
    assert rawi.next_slot() == 1
    slot = rawi.acquire()
    assert L.csdr_ingest_commit_raw(rawi.h, n + 1, 0, C.byref(p)) == ERANGE
    assert rawi.next_slot() == 1
    raw1 = random_raw("CS16", n, rng)
    fill(slot, "CS16", raw1)
    dev1 = rawi.commit(n)                                                                     # (the refused format changes left the format alone)
    assert rawi.next_slot() == 2 and dev1.ptr != dev0.ptr
    assert same_bits(download(ctx, dev1), np_convert("CS16", raw1, 32768.0))
    assert same_bits(download(ctx, dev0), np_convert("CS16", raw0, 32768.0))
    rawi.close(); typed.close()

    # a raw ingest of CF32: one code path for callers whose radio does deliver floats
    cf = Ingest(ctx, n, depth=2, format="CF32")
    xs = (rng.standard_normal(2 * n).astype(np.float32)).view(np.complex64)
    slot = cf.acquire()
    assert slot.dtype == np.float32 and slot.shape == (n, 2)
    slot.reshape(-1)[:] = xs.view(np.float32)
    assert same_bits(download(ctx, cf.commit(n)), xs)
    assert same_bits(download(ctx, cf.upload_raw(xs, n, iq_swap=True)), (xs.imag + 1j * xs.real).astype(np.complex64))
    cf.close()
