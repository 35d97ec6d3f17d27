"""The way from the waterfall's ring to a picture a viewer can show, timed two ways on the benchmark's C3 spectrum's waterfall (fftSize 65536, a
512-line ring) viewed at 1920 x 512.  Run on the GPU box from the repo root:

    python profiles/waterfall_view_rate.py a   route (a), what exists WITHOUT the viewport: csdr_waterfall_fetch_rgba of the whole ring to the host
                                               (512 x 65536 x 4 bytes).  It uses nothing but the API of the commit before the viewport and is measured
                                               on a checkout of that commit.  A LOWER BOUND: the scaling on a host core that would follow is not timed.
    python profiles/waterfall_view_rate.py b   route (b): csdr_waterfall_render_view in each mode with the 1920 x 512 x 4 bytes fetched to the host, and
                                               the two kernels alone (HIP events around the launch) with the bytes they move, wf_view_peak beside the
                                               plain-copy figures of profiles/r05_copy_rate.txt.

Host clock around calls that end in a stream synchronise; two warm-up passes, then REPEATS timed passes; median, extremes and spread are printed."""
import sys
import time

sys.path.insert(0, '.')
from cubicsdr_amd.engine import Context, Waterfall

F, LINES, W, HH, REPEATS = 65536, 512, 1920, 512, 9
route = sys.argv[1] if len(sys.argv) > 1 else ""
if route not in ("a", "b"):
    sys.exit(__doc__)

import torch

ctx = Context(0)
wf = Waterfall(ctx, F, LINES, max_pending=256)
wf.step(None)
wf.update()
g = torch.Generator(device="cuda:0").manual_seed(19)
for n in (256, 256, 88):                                   # the ring goes round once and the last update crosses the wrap
    v = torch.rand(n, F, device="cuda:0", generator=g).contiguous()
    torch.cuda.synchronize()
    assert wf.step(v) == n
    wf.update()
print("C3 spectrum's waterfall: fftSize %d, a ring of %d lines (2 x %d x %d index bytes = %.1f MB), ofs %d" % (F, LINES, LINES, F // 2, LINES * F / 1e6, wf.offset(0)))


def timed(label, fn):
    times = []
    for k in range(2 + REPEATS):
        t0 = time.perf_counter()
        fn()
        if k >= 2:
            times.append(time.perf_counter() - t0)
    t = sorted(times)
    med = t[len(t) // 2]
    print("%-52s median %9.3f ms   min %9.3f   max %9.3f   spread %5.1f %%   (%d passes)" % (label, med * 1e3, t[0] * 1e3, t[-1] * 1e3, 100 * (t[-1] - t[0]) / t[0], len(t)), flush=True)
    return med


if route == "a":
    timed("(a) fetch_rgba of the whole ring to the host", lambda: wf.fetch_rgba(0, LINES))
    print("    %d bytes over the link; the host scaling to %d x %d is not included" % (LINES * F * 4, W, HH))
else:
    for mode in ("linear", "peak"):
        timed("(b) render_view %-6s + fetch of %d x %d" % (mode, W, HH), lambda: wf.view(W, HH, mode))
    print("    %d bytes over the link" % (W * HH * 4))
    ctx.profile_enable(1)
    for mode in ("linear", "peak"):
        for _ in range(REPEATS):
            wf.view(W, HH, mode, fetch=False)
    wf.device_view()
    ctx.synchronize()
    prof = ctx.profile()
    ctx.profile_enable(False)
    # bytes per launch: PEAK reads every index byte of both rings once and the taps, and writes the picture; LINEAR touches four index bytes per pixel
    moved = {"wf_view_peak": LINES * F + W * HH * 4 + 16 * (W + HH), "wf_view_linear": W * HH * (4 + 4) + 16 * (W + HH)}
    for name in ("wf_view_linear", "wf_view_peak"):
        ms, launches, _ = prof[name]
        per = ms / launches
        print("%-15s %8.1f us per launch, %6.2f MB read + written -> %5.2f TB/s   (%d launches)" % (name, per * 1e3, moved[name] / 1e6, moved[name] / (per * 1e-3) / 1e12, launches))
    print("plain float4 copy on these boxes (profiles/r05_copy_rate.txt): 5.2 - 5.7 TB/s, nt loads + stores 5.9 - 6.2")
wf.close()
ctx.close()
