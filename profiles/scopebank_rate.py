# An audio scope per demodulator on the C3 bank (256 mixed slots, fftSize 1024, four blocks per execute): what it costs by the two routes.
#   (a) what the library offered before csdr_scopebank: 256 csdr_scope objects, each given its slot's tap where it lies in HBM
#       (csdr_bank_scope_frame + a one-frame csdr_scope_process with data_is_dev = 1 per slot: a frame upload, two launches and a host synchronise each).
#   (b) one csdr_scopebank_process_bank.
# Method: a host clock around calls that end in a synchronise; 2 warm-up and 9 timed passes per route, the routes alternating pass by pass in one
# session; medians and the spread (min .. max).  Also: the two kernels' times by HIP events (csdr_ctx_profile_*), and what process_bank adds to a C3
# step (channelizer + bank execute, synchronised), with and without it, alternating.
# Run from the repository root on an MI355X:   python profiles/scopebank_rate.py > profiles/scopebank_rate.txt
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

from cubicsdr_amd.engine import Context, DemodBank, ScopeBank, ScopeProcessor, SDRPost  # noqa: E402
from tests.util import demod_frequencies  # noqa: E402

FS, MC, BLOCK, CENTER, NB, SLOTS, L = 61_440_000, 122, 1_024_068, 100_000_000, 4, 256, 1024
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


class RouteA:
    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank
        self.scopes = [ScopeProcessor(ctx, L, max_frames=1, max_samples=4096) for _ in range(SLOTS)]

    def one_pass(self):
        t = time.perf_counter()
        n = 0
        for i, sp in enumerate(self.scopes):
            f = self.bank.scope_frame(i)
            if f.n > 0:
                sp.process([f])
                n += 1
        self.ctx.synchronize()
        self.frames = n
        return (time.perf_counter() - t) * 1e3

    def close(self):
        for sp in self.scopes:
            sp.close()


class RouteB:
    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank
        self.sb = ScopeBank(ctx, L, SLOTS, 1, 4096)

    def one_pass(self):
        t = time.perf_counter()
        self.sb.process_bank(self.bank)
        self.sb.device_points(0, True)           # the boundary stream waits for the object's own stream ...
        self.ctx.synchronize()                   # ... and the host for both
        return (time.perf_counter() - t) * 1e3

    def close(self):
        self.sb.close()


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "passes": len(v)}


def main():
    ctx = Context(0)
    post, bank, x = pipeline(ctx)
    for _ in range(2):
        post.execute(x, NB, BLOCK, CENTER)
        bank.execute(post)
    ctx.synchronize()
    a, b = RouteA(ctx, bank), RouteB(ctx, bank)
    ta, tb = [], []
    for k in range(WARM + TIMED):
        ta.append(a.one_pass())
        tb.append(b.one_pass())
    ta, tb = ta[WARM:], tb[WARM:]
    assert a.frames == sum(b.sb.frames(s) for s in range(SLOTS)) == SLOTS
    print("audio scope per demodulator, C3 bank: %d slots, fftSize %d, %d blocks per execute (%d frames per pass); %d warm-up + %d timed passes, alternating"
          % (SLOTS, L, NB, a.frames, WARM, TIMED))
    print("route (a) 256 csdr_scope objects, csdr_bank_scope_frame + one csdr_scope_process per slot:", json.dumps(stats(ta)))
    print("route (b) one csdr_scopebank_process_bank:                                              ", json.dumps(stats(tb)))
    print("factor (a) / (b), medians: %.1f" % (statistics.median(ta) / statistics.median(tb)))
    # the kernels by HIP events
    ctx.profile_enable(True)
    for _ in range(TIMED):
        b.one_pass()
    prof = ctx.profile()
    ctx.profile_enable(False)
    for name in ("scopebank_wave", "scopebank_spectrum"):
        ms, n, _ = prof[name]
        print("%s by HIP events: %.4f ms per launch (%d launches)" % (name, ms / n, n))

    # what process_bank adds to a C3 step
    def step(with_sb):
        t = time.perf_counter()
        post.execute(x, NB, BLOCK, CENTER)
        bank.execute(post)
        if with_sb:
            b.sb.process_bank(bank)
            b.sb.device_points(0, True)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3
    s0, s1 = [], []
    for k in range(WARM + TIMED):
        s0.append(step(False))
        s1.append(step(True))
    s0, s1 = s0[WARM:], s1[WARM:]
    print("C3 step (channelizer + bank execute, synchronised) without process_bank:", json.dumps(stats(s0)))
    print("C3 step with process_bank:                                             ", json.dumps(stats(s1)))
    print("process_bank adds %.4f ms to the step (medians; the step's own spread is %.4f ms)" % (statistics.median(s1) - statistics.median(s0), max(s0) - min(s0)))
    a.close(); b.close(); bank.close(); post.close(); ctx.close()
    # the one requirement
    assert statistics.median(tb) < statistics.median(ta), "route (b) must be faster than route (a)"
    print("route (b) is faster than route (a): ok")


if __name__ == "__main__":
    main()
