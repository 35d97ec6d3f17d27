"""Host-fed rate of the C3 pipeline per sample format: CF32 (the existing entry points, unchanged) against CS16 / CS8 / CS12 / CU8 carried over the
link in the radio's own format and widened on the GPU (csdr_ingest_*_raw).  Run on the GPU box from the repo root:

    python profiles/host_fed_formats.py                 the rates, one process: CF32 - CS16 - CF32 - CS8 - CF32 - CS12 - CF32 - CU8, then "transfer alone" for CS16 and CS8
    python profiles/host_fed_formats.py --trace cf32    a short CF32-only pass   } each under  rocprofv3 --kernel-trace --stats --output-format csv
    python profiles/host_fed_formats.py --trace raw     short upload_raw passes  } in a run of its own (tracing slows the host: no rates are printed)

Every pass is timed by the host clock around work that ends in csdr_ctx_synchronize, over at least a second after a warm-up.  Page-locked sources only."""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import IQ_SAMPLE_BYTES, Context, DemodBank, Ingest, SDRPost, SpectrumProcessor
from tests.util import demod_frequencies

fs, M, block, NB, nd = 61440000, 122, 1024068, 16, 256
center = 100000000
N = NB * block
FULL = {"CS16": 32768.0, "CS8": 128.0, "CU8": 128.0, "CS12": 2048.0}
DT = {"CS16": np.int16, "CS8": np.int8, "CU8": np.uint8}
MIN_SECONDS = 1.2

ctx = Context(0)
L = H.lib()
post = SDRPost(ctx, fs, M, block, max_blocks=NB)
bank = DemodBank(ctx, nd, max_blocks=NB)
kinds = ["NBFM", "AM", "USB"]; bw = {"NBFM": 12500, "AM": 6000, "USB": 5400}
for i, f in enumerate(demod_frequencies(center, fs, nd)):
    bank.configure(i, post, kinds[i % 3], bw[kinds[i % 3]], f)
spec = SpectrumProcessor(ctx, 65536, max_frames=N // 131072 + 2)
rng = np.random.default_rng(0)
x = (rng.standard_normal(N * 2).astype(np.float32) * 0.05).view(np.complex64)


def raw_of(fmt):
    """the same noise in the radio's format (bytes)"""
    v = x.view(np.float32)
    if fmt == "CS12":
        from cubicsdr_amd.engine import pack_cs12
        q = np.clip(np.round(v * 2048 * 4), -2048, 2047).astype(np.int64)
        return pack_cs12(q[0::2], q[1::2])
    if fmt == "CU8":
        return np.clip(np.round(v * 128 * 4) + 128, 0, 255).astype(np.uint8)
    full = FULL[fmt]
    return np.clip(np.round(v * full * 4), -full, full - 1).astype(DT[fmt]).view(np.uint8)


def pipeline(src):
    post.execute(src, NB, block, center); bank.execute(post); spec.process(src, NB, block, contiguous=True)


def timed(step, label, bytes_per_sample, warm=2):
    for _ in range(warm):
        step()
    ctx.synchronize()
    reps, t0 = 0, time.perf_counter()
    while True:
        for _ in range(4):
            step()
        reps += 4
        ctx.synchronize()
        dt = time.perf_counter() - t0
        if dt >= MIN_SECONDS:
            break
    rate = reps * N / dt
    print("%-58s %7.0f MS/s  %5.1f GB/s over the link  (%d calls of %d blocks, %.2f s)" % (label, rate / 1e6, rate * bytes_per_sample / 1e9, reps, NB, dt), flush=True)
    return rate


def host_pointer_pass():
    """profiles/host_fed.py's page-locked shape: the entry points handed the registered host block"""
    return timed(lambda: pipeline(x), "CF32, host block handed to post / spectrum (host_fed.py)", 8)


def ring_pass(fmt, with_pipeline=True, via_upload=False, pinned_src=None):
    """the block ring: commit (or upload_raw from a registered buffer) per 16-block call; the slots are filled once -- filling them is the radio's work"""
    raw = None if fmt == "CF32" else raw_of(fmt)
    ing = Ingest(ctx, N, depth=3, format=None if fmt == "CF32" else fmt, full_scale=FULL.get(fmt), offset=128.0 if fmt == "CU8" else 0.0)
    if not via_upload:
        for _ in range(3):
            slot = ing.acquire()
            if fmt == "CF32":
                slot[:] = x
            else:
                slot.reshape(-1).view(np.uint8)[:] = raw
            dev = ing.commit(N)
        ctx.synchronize()

    def step():
        if via_upload:
            dev = ing.upload_raw(pinned_src, N)
        else:
            ing.acquire()
            dev = ing.commit(N)
        if with_pipeline:
            pipeline(dev)
    what = "upload_raw from a registered buffer" if via_upload else ("commit: one DMA" if fmt == "CF32" else "commit_raw: DMA of the raw bytes + conversion in HBM")
    label = "%-5s ring, %s%s" % (fmt, what, "" if with_pipeline else ", transfer alone")
    r = timed(step, label, IQ_SAMPLE_BYTES[H.IQ_FORMAT_BY_NAME[fmt]])
    ing.wait(); ctx.synchronize()
    ing.close()
    return r


def trace(which):
    if which == "cf32":
        ing = Ingest(ctx, N, depth=3)
        for k in range(4):
            ing.acquire()[:] = x
            pipeline(ing.commit(N, iq_swap=(k % 2 == 1)))
        ctx.synchronize(); ing.close()
        L.csdr_host_register(ctx.h, x.ctypes.data_as(C.c_void_p), x.nbytes)
        for _ in range(2):
            pipeline(x)
        ctx.synchronize()
        print("trace pass cf32 done")
        return
    for fmt in ("CS16", "CS8", "CU8", "CS12"):
        raw = raw_of(fmt)
        H.check(L.csdr_host_register(ctx.h, raw.ctypes.data_as(C.c_void_p), raw.nbytes))
        ing = Ingest(ctx, N, depth=3, format=fmt, full_scale=FULL[fmt], offset=128.0 if fmt == "CU8" else 0.0)
        for _ in range(6):
            ing.upload_raw(raw, N)                         # DMA into the staging buffer, ingest_convert<fmt> in HBM
        for _ in range(3):
            ing.acquire().reshape(-1).view(np.uint8)[:] = raw
            ing.commit(N)                                   # the same two steps from the ring's own page-locked slot
        ing.wait(); ctx.synchronize(); ing.close()
        L.csdr_host_unregister(ctx.h, raw.ctypes.data_as(C.c_void_p))
    print("trace pass raw done")


if "--trace" in sys.argv:
    trace(sys.argv[sys.argv.index("--trace") + 1])
    sys.exit(0)

print("C3: %.2f MS/s, M = %d, %d demodulators, 65536-point spectrum, calls of %d blocks of %d samples; page-locked sources" % (fs / 1e6, M, nd, NB, block))
H.check(L.csdr_host_register(ctx.h, x.ctypes.data_as(C.c_void_p), x.nbytes))
print("\n## host-fed rate per format (one process, in this order)")
host_pointer_pass()
cf, raw_rates = [], {}
for fmt in ("CS16", "CS8", "CS12", "CU8"):
    cf.append(ring_pass("CF32"))
    raw_rates[fmt] = ring_pass(fmt)
cf.append(ring_pass("CF32"))
print("CF32 ring passes: min %.0f  median %.0f  max %.0f MS/s  (spread %.1f %%)" % (min(cf) / 1e6, sorted(cf)[len(cf) // 2] / 1e6, max(cf) / 1e6, 100 * (max(cf) - min(cf)) / min(cf)))
med = sorted(cf)[len(cf) // 2]
for fmt, r in raw_rates.items():
    b = IQ_SAMPLE_BYTES[H.IQ_FORMAT_BY_NAME[fmt]]
    print("%-5s / CF32 median = %.2f   (8 / %d bytes = %.2f if the link alone bounds both)" % (fmt, r / med, b, 8 / b))

print("\n## the transfer alone (commit_raw per 16-block call, no pipeline beside it)")
for fmt in ("CS16", "CS8"):
    ring_pass(fmt, with_pipeline=False)
