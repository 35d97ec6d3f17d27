# specbank_process and viewbank_process at 200 launches per process: the set-ups of specbank_rate.py and viewbank_rate.py (C3: 256 slots, fftSize
# 1024, four inputs per slot and launch), the kernel's time by HIP events (mean, shortest and longest launch) and the one-call route's median over
# the same passes.  The two rate scripts time nine launches, which is enough for a factor of several hundred and too few to compare two builds
# of one kernel; this is what profiles/specframe_shared_rate.txt alternates between two checkouts.  It uses nothing a checkout without it lacks:
#   cd <checkout> && python <path to this file>        one JSON line
import json
import statistics
import sys

sys.path.insert(0, ".")
from cubicsdr_amd.engine import Context  # noqa: E402
from profiles import specbank_rate as S, viewbank_rate as V  # noqa: E402

WARM, TIMED = 10, 200


def timed(ctx, route, kernel):
    for _ in range(WARM):
        route.one_pass()
    ctx.profile_enable(True)
    t = [route.one_pass() for _ in range(TIMED)]
    prof = ctx.profile()
    ctx.profile_enable(False)
    ms, n = prof[kernel][0], prof[kernel][1]
    return {"kernel_us": round(1e3 * ms / n, 3), "launches": n, "call_median_us": round(1e3 * statistics.median(t), 2)}


def main():
    ctx = Context(0)
    post, bank, x = S.pipeline(ctx)
    for _ in range(2):
        post.execute(x, S.NB, S.BLOCK, S.CENTER)
        bank.execute(post)
    ctx.synchronize()
    b = S.RouteB(ctx, bank)
    out = {"specbank_process": timed(ctx, b, "specbank_process")}
    b.close()
    v = V.RouteB(ctx, post, V.demod_frequencies(V.CENTER, V.FS, V.SLOTS), x)
    out["viewbank_process"] = timed(ctx, v, "viewbank_process")
    v.close(); bank.close(); post.close(); ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
