"""The way from a spectrum's finished lines to the waterfall picture, timed two ways on the benchmark's C3 spectrum (fftSize 65536, the contiguous
frames of one batch: 128 blocks of 1 024 068 samples = 1000 frames).  Run on the GPU box from the repo root:

    python profiles/waterfall_rate.py a     route (a), what exists WITHOUT csdr_waterfall: per frame csdr_spec_fetch, then the panel's quantiser in numpy
                                            on the host.  It uses nothing but the API of the commit before the waterfall, and is measured on a checkout
                                            of that commit.
    python profiles/waterfall_rate.py b     route (b): csdr_waterfall_step_spec of all frames + update + fetch_rgba(NULL) -- quantised lines, a 512-line ring
                                            and its RGBA picture, all left in HBM -- and the achieved bytes per second of wf_quantize alone
                                            (HIP events around the launch) beside the plain-copy figures of profiles/r05_copy_rate.txt.

Both time the way OUT only: the spectrum is processed once, before the clock starts.  Host clock around work that ends in a device synchronise; two
warm-up passes, then REPEATS timed passes; median, extremes and spread are printed."""
import sys
import time

import numpy as np

sys.path.insert(0, '.')
from cubicsdr_amd.engine import Context, SpectrumProcessor

F, BLOCK, NB, LINES, REPEATS = 65536, 1024068, 128, 512, 9
route = sys.argv[1] if len(sys.argv) > 1 else ""
if route not in ("a", "b"):
    sys.exit(__doc__)

import torch

ctx = Context(0)
n = NB * BLOCK
NF = n // (2 * F)
spec = SpectrumProcessor(ctx, F, max_frames=NF + 2)
g = torch.Generator(device="cuda:0").manual_seed(3)
x = torch.view_as_complex((torch.randn(n, 2, device="cuda:0", generator=g) * 0.05).contiguous())
x += 0.3 * torch.exp(2j * np.pi * 0.0371 * torch.arange(n, device="cuda:0", dtype=torch.float64)).to(torch.complex64)
torch.cuda.synchronize()
assert spec.process(x, NB, BLOCK, contiguous=True) == NF
ctx.synchronize()
print("C3 spectrum: fftSize %d, %d contiguous frames of one batch (%d blocks of %d samples)" % (F, NF, NB, BLOCK))


def report(label, times, extra=""):
    t = sorted(times)
    med = t[len(t) // 2]
    print("%-44s median %9.3f ms   min %9.3f   max %9.3f   spread %4.1f %%   (%d passes)%s" % (label, med * 1e3, t[0] * 1e3, t[-1] * 1e3, 100 * (t[-1] - t[0]) / t[0], len(t), extra), flush=True)
    return med


if route == "a":
    c99, c255, zero = np.float32(0.99), np.float32(255.0), np.float32(0.0)
    out = np.empty((NF, F), np.uint8)

    def way_out():
        for f in range(NF):
            y = spec.fetch(f)[0][1::2]
            out[f] = (np.minimum(np.maximum(y, zero), c99) * c255).astype(np.uint8)     # WaterfallPanel.cpp:64-72 in float32, vectorised

    times = []
    for k in range(2 + REPEATS):
        t0 = time.perf_counter()
        way_out()
        ctx.synchronize()
        if k >= 2:
            times.append(time.perf_counter() - t0)
    med = report("(a) fetch per frame + quantiser in numpy", times)
    print("    per frame %.1f us; %d x %d bytes over the link, %d bytes expanded on the host" % (med / NF * 1e6, NF, 4 * F, 8 * F))
else:
    from cubicsdr_amd.engine import Waterfall
    wf = Waterfall(ctx, F, LINES, max_pending=NF)
    wf.step(None)
    wf.update()

    def way_out():
        assert wf.step_spec(spec, 0, NF) == NF
        wf.update()
        wf.fetch_rgba(0, LINES, fetch=False)
        wf.device_rgba()                                   # the boundary stream waits for the picture ...
        ctx.synchronize()                                  # ... and the host for the boundary stream

    times = []
    for k in range(2 + REPEATS):
        t0 = time.perf_counter()
        way_out()
        if k >= 2:
            times.append(time.perf_counter() - t0)
    med = report("(b) step_spec + update + fetch_rgba(NULL)", times)
    print("    per frame %.2f us; nothing crosses the link" % (med / NF * 1e6))
    ctx.profile_enable(1)
    for _ in range(REPEATS):
        way_out()
    prof = ctx.profile()
    ctx.profile_enable(False)
    moved = {"wf_quantize": NF * 5 * F, "wf_update": 2 * 2 * LINES * (F // 2), "wf_rgba": LINES * F * 5}     # bytes read + written per launch
    for name in ("wf_quantize", "wf_update", "wf_rgba"):
        ms, launches, _ = prof[name]
        per = ms / launches
        print("%-12s %8.1f us per launch, %6.1f MB read + written -> %5.2f TB/s   (%d launches)" % (name, per * 1e3, moved[name] / 1e6, moved[name] / (per * 1e-3) / 1e12, launches))
    print("plain float4 copy on these boxes (profiles/r05_copy_rate.txt): 5.2 - 5.7 TB/s, nt loads + stores 5.9 - 6.2")
    wf.close()
spec.close()
ctx.close()
