# The zoomed demodulator spectrum per demodulator on the C3 pipeline (256 demodulators, fftSize 1024, four blocks per execute, a view of 300 kHz at
# each demodulator's frequency on its 503606 S/s channel row): what it costs by the two routes.
#   (a) what the library offered before csdr_viewbank: 256 csdr_spec objects in view mode (csdr_spec_set_view), each given its row's block where it
#       lies in HBM (csdr_spec_process, iq_is_dev = 1: one call per slot and block; every object runs a private one-slot front-end and synchronises
#       the host three times per input).  The rows are copied into one device buffer beforehand, outside the timed region.
#   (b) one csdr_viewbank_process_post.
# Method: a host clock around calls that end in a synchronise; 2 warm-up and 9 timed passes per route, the routes alternating pass by pass; medians
# and the spread (min .. max).  Also: the kernel's time by HIP events (csdr_ctx_profile_*), and what process_post adds to a C3 step (channelizer +
# bank execute, synchronised), with and without it, alternating.
# Run from the repository root on an MI355X:   python profiles/viewbank_rate.py [--parent DIR] > profiles/viewbank_rate.txt
#   --parent DIR   also measure route (a) in a checkout of the parent commit built at DIR (a child process, this file, --route a)
#   --route a      route (a) alone, one JSON line (what the child runs; needs nothing this change added)
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

import cubicsdr_amd.hip as H  # noqa: E402
from cubicsdr_amd.engine import Context, DemodBank, DevicePointer, SDRPost, SpectrumProcessor  # noqa: E402
from tests.util import demod_frequencies  # noqa: E402

FS, MC, BLOCK, CENTER, NB, SLOTS, F, VIEW_BW = 61_440_000, 122, 1_024_068, 100_000_000, 4, 256, 1024, 300_000
WARM, TIMED = 2, 9


def pipeline(ctx):
    post = SDRPost(ctx, FS, MC, BLOCK, NB)
    bank = DemodBank(ctx, SLOTS, NB)
    freqs = demod_frequencies(CENTER, FS, SLOTS)
    kinds, bws = ["NBFM", "AM", "USB"], {"NBFM": 12_500, "AM": 6_000, "USB": 5_400}
    for i, f in enumerate(freqs):
        bank.configure(i, post, kinds[i % 3], bws[kinds[i % 3]], f)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(NB * BLOCK) + 1j * rng.standard_normal(NB * BLOCK)).astype(np.complex64) * np.float32(0.1)
    return post, bank, freqs, x


def rows_of(post, freqs):
    """the data row and its centre for every demodulator, as csdr_bank_execute routes them"""
    out = []
    for f in freqs:
        ch = post.channel_at(f)
        out.append((MC // 2 if ch == MC else ch, post.channel_center(ch)))
    return out


class RouteA:
    def __init__(self, ctx, post, freqs):
        lib = H.lib()
        self.ctx = ctx
        self.rate = post.channel_rate
        rows = rows_of(post, freqs)
        bc = BLOCK // MC
        self.specs = []
        flat = np.concatenate([post.read_channel(r) for r, _ in rows])
        assert flat.size == SLOTS * NB * bc
        self.buf = C.c_void_p()
        H.check(lib.csdr_dev_alloc(ctx.h, 8 * flat.size, C.byref(self.buf)))
        H.check(lib.csdr_dev_upload(ctx.h, self.buf, flat.ctypes.data_as(C.c_void_p), 8 * flat.size))
        self.calls = []
        for i, (f, (_, centre)) in enumerate(zip(freqs, rows)):
            sp = SpectrumProcessor(ctx, F, 1)
            sp.set_view(True, f, VIEW_BW)
            self.specs.append(sp)
            for b in range(NB):
                self.calls.append((sp, DevicePointer(self.buf.value + 8 * ((i * NB + b) * bc), bc), centre))

    def one_pass(self):
        t = time.perf_counter()
        for sp, ptr, centre in self.calls:
            sp.process_view_input(ptr, centre, self.rate)
        self.ctx.synchronize()
        return (time.perf_counter() - t) * 1e3

    def close(self):
        for sp in self.specs:
            sp.close()
        H.check(H.lib().csdr_dev_free(self.ctx.h, self.buf))


class RouteB:
    def __init__(self, ctx, post, freqs, x):
        from cubicsdr_amd.engine import ViewBank
        self.ctx, self.post, self.x = ctx, post, x
        self.vb = ViewBank(ctx, F, SLOTS, NB, BLOCK // MC)
        self.rows = [r for r, _ in rows_of(post, freqs)]
        self.slots = list(range(SLOTS))
        for i, f in enumerate(freqs):
            self.vb.set_view(i, f, VIEW_BW)

    def enqueue(self):
        self.vb.process_post(self.post, self.slots, self.rows)
        self.vb.device_points(0)                 # the boundary stream waits for the object's own stream ...

    def one_pass(self):
        self.post.execute(self.x, NB, BLOCK, CENTER)     # (a batch takes four readers: every pass reads a fresh one, made outside the timed region)
        self.ctx.synchronize()
        t = time.perf_counter()
        self.enqueue()
        self.ctx.synchronize()                   # ... and the host for both
        return (time.perf_counter() - t) * 1e3

    def close(self):
        self.vb.close()


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "passes": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="both", choices=["a", "both"])
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    post, bank, freqs, x = pipeline(ctx)
    for _ in range(2):
        post.execute(x, NB, BLOCK, CENTER)
        bank.execute(post)
    ctx.synchronize()
    a = RouteA(ctx, post, freqs)
    if args.route == "a":
        t = [a.one_pass() for _ in range(WARM + TIMED)][WARM:]
        print(json.dumps({"route": "a", "calls_per_pass": len(a.calls), **stats(t)}))
        a.close(); bank.close(); post.close(); ctx.close()
        return
    b = RouteB(ctx, post, freqs, x)
    ta, tb = [], []
    for k in range(WARM + TIMED):
        ta.append(a.one_pass())
        tb.append(b.one_pass())
    ta, tb = ta[WARM:], tb[WARM:]
    assert all(b.vb.frames(s) == NB for s in range(SLOTS))
    print("zoomed view per demodulator, C3 pipeline: %d slots, fftSize %d, view %d Hz on %d S/s rows, %d blocks per execute (%d inputs per pass); %d warm-up + %d timed passes, alternating"
          % (SLOTS, F, VIEW_BW, post.channel_rate, NB, len(a.calls), WARM, TIMED))
    print("route (a) 256 csdr_spec objects in view mode, one csdr_spec_process per slot and block:", json.dumps(stats(ta)))
    print("route (b) one csdr_viewbank_process_post:                                            ", json.dumps(stats(tb)))
    print("factor (a) / (b), medians: %.1f" % (statistics.median(ta) / statistics.median(tb)))
    # the kernel by HIP events
    ctx.profile_enable(True)
    for _ in range(TIMED):
        b.one_pass()
    prof = ctx.profile()
    ctx.profile_enable(False)
    ms, n, _ = prof["viewbank_process"]
    print("viewbank_process by HIP events: %.4f ms per launch (%d launches)" % (ms / n, n))
    # what process_post adds to a C3 step
    def step(with_vb):
        t = time.perf_counter()
        post.execute(x, NB, BLOCK, CENTER)
        bank.execute(post)
        if with_vb:
            b.enqueue()
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3
    s0, s1 = [], []
    for k in range(WARM + TIMED):
        s0.append(step(False))
        s1.append(step(True))
    s0, s1 = s0[WARM:], s1[WARM:]
    print("C3 step (channelizer + bank execute, synchronised) without process_post:", json.dumps(stats(s0)))
    print("C3 step with process_post:                                             ", json.dumps(stats(s1)))
    print("process_post adds %.4f ms to the step (medians; the step's own spread is %.4f ms)" % (statistics.median(s1) - statistics.median(s0), max(s0) - min(s0)))
    a.close(); b.close(); bank.close(); post.close(); ctx.close()
    med_a = statistics.median(ta)
    if args.parent:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", "a"], cwd=args.parent, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip(), "route (a) on the parent checkout failed: " + (r.stderr.strip().splitlines() or ["?"])[-1]
        pa = json.loads(r.stdout.strip().splitlines()[-1])
        print("route (a) on a checkout of the parent commit (a process of its own, behind the passes above):", json.dumps(pa))
        print("factor (a, parent) / (b), medians: %.1f" % (pa["median_ms"] / statistics.median(tb)))
        med_a = min(med_a, pa["median_ms"])
    # the one requirement
    assert statistics.median(tb) < med_a, "route (b) must be faster than route (a)"
    print("route (b) is faster than route (a): ok")


if __name__ == "__main__":
    main()
