# Host time of one call that ends in a synchronise, median of 200 calls, for the four calls whose stream ordering stream_order.hpp states:
# SpectrumBank.process_bank, ScopeBank.process_bank, SquelchBank.process_bank and WaterfallBank.step_from (+ update + atlas, as wfbank_rate.py's
# route), at the 256-slot shape of the *_at_size tests and the rate scripts (61.44 MS/s, 122 channels, 256 demodulators, four blocks per execute).
# One reader per writer: the stream operations of each call are the parent's.  This is what profiles/streamorder_rate.txt alternates between two
# checkouts.  It uses nothing a checkout without it lacks:
#   cd <checkout> && python <path to this file>        one JSON line
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
from cubicsdr_amd.engine import Context, SquelchBank  # noqa: E402
from profiles import scopebank_rate as SC, specbank_rate as S, wfbank_rate as W  # noqa: E402

WARM, TIMED = 10, 200


class SquelchRoute:
    def __init__(self, ctx, bank):
        self.ctx, self.bank = ctx, bank
        self.sq = SquelchBank(ctx, S.SLOTS, S.NB)
        for s in range(S.SLOTS):
            self.sq.set_slot(s, True, -40.0, False, s % 3)

    def one_pass(self):
        t = time.perf_counter()
        self.sq.process_bank(self.bank)
        self.sq.device_items()                   # the boundary stream waits for the object's own stream ...
        self.ctx.synchronize()                   # ... and the host for both
        return (time.perf_counter() - t) * 1e3

    def close(self):
        self.sq.close()


def timed(route):
    for _ in range(WARM):
        route.one_pass()
    t = sorted(route.one_pass() for _ in range(TIMED))
    return {"median_us": round(1e3 * statistics.median(t), 2), "p10_us": round(1e3 * t[TIMED // 10], 2), "p90_us": round(1e3 * t[9 * TIMED // 10], 2)}


def main():
    ctx = Context(0)
    post, bank, x = S.pipeline(ctx)
    for _ in range(2):
        post.execute(x, S.NB, S.BLOCK, S.CENTER)
        bank.execute(post)
    ctx.synchronize()
    out = {}
    spec = S.RouteB(ctx, bank)
    out["SpectrumBank.process_bank"] = timed(spec)
    scope = SC.RouteB(ctx, bank)
    out["ScopeBank.process_bank"] = timed(scope)
    scope.close()
    sq = SquelchRoute(ctx, bank)
    out["SquelchBank.process_bank"] = timed(sq)
    sq.close()
    W.fresh_points(ctx, spec.sb, bank)
    wf = W.RouteB(ctx, spec.sb)
    out["WaterfallBank.step_from"] = timed(wf)
    wf.close(); spec.close(); bank.close(); post.close(); ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
