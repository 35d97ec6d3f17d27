# A waterfall per demodulator on the C3 bank (256 mixed slots, fftSize 1024, four blocks per execute): what a display turn costs by the two routes.
# A turn: every slot's lines of the spectrum bank's last process_bank (four per slot) stepped where they lie in HBM, an update, and 128 x 64 LINEAR
# thumbnails left on the device (256 lines to a ring).
#   (a) what the library offered before csdr_wfbank: 256 csdr_waterfall objects, each with csdr_waterfall_step(is_dev = 1) on
#       csdr_specbank_device_points, csdr_waterfall_update, csdr_waterfall_render_view(NULL) and csdr_waterfall_device_view (the hand-over of the
#       picture to the boundary stream, which is also what lets the host wait for the object's stream).
#   (b) the bank's three calls -- step_specbank, update, render as a 16-column atlas -- and one csdr_wfbank_device_view.
# Method: a host clock around calls that end in a synchronise; 2 warm-up and 9 timed passes per route, the routes alternating pass by pass; a fresh
# process_bank, synchronised, in front of every pass and outside the clock; medians and the spread (min .. max).  Also: every kernel of both routes by
# HIP events (csdr_ctx_profile_*), with the bytes it moves per launch.
# Run from the repository root on an MI355X:   python profiles/wfbank_rate.py [--parent DIR] > profiles/wfbank_rate.txt
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
from cubicsdr_amd.engine import Context, DemodBank, SDRPost, SpectrumBank, Waterfall  # noqa: E402
from tests.util import demod_frequencies  # noqa: E402

FS, MC, BLOCK, CENTER, NB, SLOTS, F = 61_440_000, 122, 1_024_068, 100_000_000, 4, 256, 1024
LINES, W, HH, COLS = 256, 128, 64, 16
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
    return post, bank, x


def fresh_points(ctx, sb, bank):
    sb.process_bank(bank)
    sb.device_points(0)                          # the boundary stream waits for the spectrum bank's stream ...
    ctx.synchronize()                            # ... and the host for both


class RouteA:
    def __init__(self, ctx, sb):
        self.ctx, self.sb, self.lib = ctx, sb, H.lib()
        self.wfs = [Waterfall(ctx, F, LINES, 8) for _ in range(SLOTS)]
        self.lines = 0

    def one_pass(self):
        lib, sb = self.lib, self.sb
        taken, p, n = C.c_int(), C.c_void_p(), C.c_int()
        t = time.perf_counter()
        for s, wf in enumerate(self.wfs):
            H.check(lib.csdr_specbank_device_points(sb.h, s, C.byref(p), C.byref(n)))
            if n.value:
                H.check(lib.csdr_waterfall_step(wf.h, p, 1, F, n.value, C.byref(taken)))
                self.lines += taken.value
            H.check(lib.csdr_waterfall_update(wf.h))
            if lib.csdr_waterfall_offset(wf.h, 0) >= 0:
                H.check(lib.csdr_waterfall_render_view(wf.h, W, HH, H.WF_VIEW_LINEAR, None, 0))
                H.check(lib.csdr_waterfall_device_view(wf.h, C.byref(p), None, None))
        self.ctx.synchronize()
        return (time.perf_counter() - t) * 1e3

    def close(self):
        for wf in self.wfs:
            wf.close()


class RouteB:
    def __init__(self, ctx, sb):
        from cubicsdr_amd.engine import WaterfallBank
        self.ctx, self.sb = ctx, sb
        self.wb = WaterfallBank(ctx, F, LINES, SLOTS, 8)
        self.lines = 0

    def one_pass(self):
        t = time.perf_counter()
        self.lines += self.wb.step_from(self.sb)
        self.wb.update()
        self.wb.view(SLOTS, W, HH, "linear", COLS, fetch=False)
        self.wb.device_view()                    # the boundary stream waits for the object's own stream ...
        self.ctx.synchronize()                   # ... and the host for both
        return (time.perf_counter() - t) * 1e3

    def close(self):
        self.wb.close()


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "passes": len(v)}


def kernel_lines(prof, names, bytes_of):
    out = []
    for k in names:
        if k in prof and prof[k][1]:
            ms, n, _ = prof[k]
            b = bytes_of.get(k)
            out.append("  %-16s %.4f ms per launch (%d launches)%s" % (k, ms / n, n, "" if b is None else ", %.2f MB per launch: %.1f GB/s" % (b / 1e6, b / (ms / n) / 1e6)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", default="both", choices=["a", "both"])
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    post, bank, x = pipeline(ctx)
    for _ in range(2):
        post.execute(x, NB, BLOCK, CENTER)
        bank.execute(post)
    ctx.synchronize()
    sb = SpectrumBank(ctx, F, SLOTS, NB)
    a = RouteA(ctx, sb)
    if args.route == "a":
        t = []
        for _ in range(WARM + TIMED):
            fresh_points(ctx, sb, bank)
            t.append(a.one_pass())
        print(json.dumps({"route": "a", "lines": a.lines, **stats(t[WARM:])}))
        a.close(); sb.close(); bank.close(); post.close(); ctx.close()
        return
    b = RouteB(ctx, sb)
    ta, tb = [], []
    for k in range(WARM + TIMED):
        fresh_points(ctx, sb, bank)
        ta.append(a.one_pass())
        fresh_points(ctx, sb, bank)
        tb.append(b.one_pass())
    ta, tb = ta[WARM:], tb[WARM:]
    assert a.lines == b.lines > 0, (a.lines, b.lines)
    print("waterfall per demodulator, C3 bank: %d slots, fftSize %d, %d lines, %d blocks per execute (%d lines stepped per route in %d passes); "
          "%d x %d LINEAR thumbnails; %d warm-up + %d timed passes, alternating" % (SLOTS, F, LINES, NB, a.lines, WARM + TIMED, W, HH, WARM, TIMED))
    print("route (a) 256 csdr_waterfall objects, step + update + render_view + device_view each:", json.dumps(stats(ta)))
    print("route (b) csdr_wfbank: step_specbank + update + render + device_view:               ", json.dumps(stats(tb)))
    print("factor (a) / (b), medians: %.1f" % (statistics.median(ta) / statistics.median(tb)))
    # the kernels by HIP events, both routes; bytes per launch of this workload (4 lines per slot and turn)
    half, lines4 = F // 2, 4
    per_wf = {"wf_quantize": lines4 * F * 4 + lines4 * F + F * 4, "wf_update": 2 * lines4 * F, "wf_view_linear": W * HH * 4 + 4 * W * HH}
    per_wb = {"wfb_quantize": SLOTS * per_wf["wf_quantize"], "wfb_update": SLOTS * per_wf["wf_update"], "wfb_view_linear": SLOTS * per_wf["wf_view_linear"]}
    ctx.profile_enable(True)
    for _ in range(3):
        fresh_points(ctx, sb, bank)
        a.one_pass()
        fresh_points(ctx, sb, bank)
        b.one_pass()
    b.wb.view(SLOTS, W, HH, "peak", COLS, fetch=False)
    b.wb.device_view(); ctx.synchronize()
    prof = ctx.profile()
    ctx.profile_enable(False)
    per_wb["wfb_view_peak"] = SLOTS * (LINES * 2 * half + W * HH * 4)
    print("kernels by HIP events (bytes: lines read as floats + index bytes written + kept points; rows read + written; pixels written + texels gathered):")
    for ln in kernel_lines(prof, ("wf_quantize", "wf_update", "wf_view_linear"), per_wf) + kernel_lines(prof, ("wfb_quantize", "wfb_update", "wfb_view_linear", "wfb_view_peak"), per_wb):
        print(ln)
    a.close(); b.close(); sb.close(); bank.close(); post.close(); ctx.close()
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
