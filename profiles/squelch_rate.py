# The squelch decision, the gated mixer feed and the squelch-aware recorder on the C3 bank (256 mixed slots, 128 blocks per execute): what a batch
# costs by the two routes.
#   (a) what the library offered before csdr_squelch, for the same result: 256 x csdr_bank_fetch_results (a copy and a stream synchronise per
#       slot), the level step per block on the host, a csdr_mix_push_bank per slot that may be heard (it takes every block of a slot or none: the
#       per-block gate cannot be honoured, so this route pushes the slots whose last block is open), 256 x csdr_bank_fetch_pcm16 (two synchronises
#       per slot; cutting by the flags would follow on the host and is not timed).  The host level step here is the Python checker
#       (oracle.cubicsdr_chain.RefLevelSquelch), far slower than host/DemodLevel.h's few scalar operations: it is timed and reported on its own and
#       left OUT of route (a)'s total.
#   (b) csdr_squelch_process_bank + csdr_squelch_fetch_flags + csdr_mix_push_squelched + csdr_squelch_record.
# Both routes leave 128 blocks per source in the mixer's queues; a render outside the timed region drains them.
# Method: a host clock around calls that end in a synchronise; 2 warm-up and 7 timed passes per route, the routes alternating pass by pass in one
# session on the same batch; medians and the spread (min .. max).  Also the three kernels' times by HIP events (csdr_ctx_profile_*).
# The IQ is noise under a per-block envelope (six loud, six quiet blocks); every slot's threshold is the median of its own level over the batch, so
# the squelch opens and closes inside the batch.
# Run from the repository root on an MI355X:   python profiles/squelch_rate.py > profiles/squelch_rate.txt
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cubicsdr_amd.engine import AudioMixer, Context, DemodBank, SDRPost, SquelchBank  # noqa: E402
from oracle.cubicsdr_chain import RefLevelSquelch  # noqa: E402
from tests.util import demod_frequencies  # noqa: E402

FS, MC, BLOCK, CENTER, NB, SLOTS = 61_440_000, 122, 1_024_068, 100_000_000, 128, 256
KINDS, BWS = ["NBFM", "AM", "USB"], {"NBFM": 12_500, "AM": 6_000, "USB": 5_400}
WARM, TIMED = 2, 7


def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "passes": len(v)}


def main():
    ctx = Context(0)
    post, bank = SDRPost(ctx, FS, MC, BLOCK, NB), DemodBank(ctx, SLOTS, NB)
    for i, f in enumerate(demod_frequencies(CENTER, FS, SLOTS)):
        bank.configure(i, post, KINDS[i % 3], BWS[KINDS[i % 3]], f)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    x = torch.randn(NB, BLOCK, 2, device="cuda", generator=g) * 0.1
    x *= torch.where((torch.arange(NB, device="cuda") // 6) % 2 == 0, 1.0, 0.05).reshape(NB, 1, 1)
    x = x.reshape(-1, 2)
    torch.cuda.synchronize()
    for _ in range(2):
        post.execute(x, NB, BLOCK, CENTER)
        bank.execute(post)
    ctx.synchronize()
    sq = SquelchBank(ctx, SLOTS, NB)
    mix = AudioMixer(ctx, SLOTS, 48000, 1 << 18)
    slots = list(range(SLOTS))
    # thresholds: the median of every slot's own level over this batch (signalLevel does not depend on the settings)
    sq.process_bank(bank)
    thr = [float(np.median(sq.fetch(s)["level"])) for s in slots]
    for s in slots:
        sq.reset_slot(s)
        sq.set_slot(s, True, thr[s], False, s % 3)

    def drain():
        mix.render(800, NB, fetch=False)
        ctx.synchronize()

    def route_a(parts):
        refs = parts.setdefault("refs", [RefLevelSquelch() for _ in slots])
        t0 = time.perf_counter()
        res = [bank.results(s) for s in slots]
        t1 = time.perf_counter()
        last_open = []
        for s in slots:
            squelched = False
            for r in res[s]:
                squelched = refs[s].step(r.n_audio > 0, r.level_accum, r.level_count, float(r.n_iq) / float(BWS[KINDS[s % 3]]), True, thr[s])
            last_open.append(not squelched)
        t2 = time.perf_counter()
        for s in slots:
            if last_open[s]:
                mix.push_bank(bank, [s])
        ctx.synchronize()
        t3 = time.perf_counter()
        n = sum(bank.pcm16(s).size for s in slots)
        t4 = time.perf_counter()
        parts.setdefault("fetch_results", []).append((t1 - t0) * 1e3)
        parts.setdefault("level_step_python", []).append((t2 - t1) * 1e3)
        parts.setdefault("push_per_slot", []).append((t3 - t2) * 1e3)
        parts.setdefault("fetch_pcm16", []).append((t4 - t3) * 1e3)
        parts["samples"] = n
        return (t1 - t0 + t3 - t2 + t4 - t3) * 1e3

    def route_b(parts):
        t0 = time.perf_counter()
        sq.process_bank(bank)
        t1 = time.perf_counter()
        flags = sq.flags()
        t2 = time.perf_counter()
        mix.push_bank_squelched(bank, sq, slots)
        t3 = time.perf_counter()
        pcm, offs = sq.record(cap=1 << 26)
        ctx.synchronize()
        t4 = time.perf_counter()
        for k, v in (("process_bank_enqueue", t1 - t0), ("fetch_flags", t2 - t1), ("push_bank_squelched", t3 - t2), ("record", t4 - t3)):
            parts.setdefault(k, []).append(v * 1e3)
        parts["open_blocks"], parts["samples"] = int(np.count_nonzero(flags & 4)), int(pcm.size)
        parts["flips"] = int(np.count_nonzero(np.diff((flags & 1).astype(np.int8), axis=1)))
        return (t4 - t0) * 1e3
    pa, pb, ta, tb = {}, {}, [], []
    for k in range(WARM + TIMED):
        ta.append(route_a(pa)); drain()
        tb.append(route_b(pb)); drain()
    ta, tb = ta[WARM:], tb[WARM:]
    print("squelch, gated mix and recorder, C3 bank: %d slots, %d blocks per execute; %d warm-up + %d timed passes, alternating" % (SLOTS, NB, WARM, TIMED))
    print("route (a) per-slot round trips, without the host level step:", json.dumps(stats(ta)))
    for k in ("fetch_results", "push_per_slot", "fetch_pcm16", "level_step_python"):
        print("    (a) %-20s %s" % (k, json.dumps(stats(pa[k][WARM:]))))
    print("    (a) records %d samples before cutting" % pa["samples"])
    print("route (b) process_bank + fetch_flags + push_bank_squelched + record:", json.dumps(stats(tb)))
    for k in ("process_bank_enqueue", "fetch_flags", "push_bank_squelched", "record"):
        print("    (b) %-20s %s" % (k, json.dumps(stats(pb[k][WARM:]))))
    print("    (b) %d open blocks of %d, %d squelch flips inside the batch, %d samples recorded" % (pb["open_blocks"], SLOTS * NB, pb["flips"], pb["samples"]))
    print("factor (a) / (b), medians: %.1f" % (statistics.median(ta) / statistics.median(tb)))
    ctx.profile_enable(True)
    for _ in range(TIMED):
        route_b({}); drain()
    prof = ctx.profile()
    ctx.profile_enable(False)
    for name in ("squelch_scan", "squelch_pack", "squelch_pcm16"):
        ms, n, _ = prof[name]
        print("%s by HIP events: %.4f ms per launch (%d launches)" % (name, ms / n, n))
    for o in (mix, sq, bank, post, ctx):
        o.close()


if __name__ == "__main__":
    main()
