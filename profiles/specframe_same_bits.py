# Are the frames of csdr_specbank and csdr_viewbank the same bits on two checkouts?  Both banks are driven through the case generators of
# tests/specbank_cases.py and tests/viewbank_cases.py at F = 16 and 256 (the main plan with its NaN inputs, and the peak-hold plan; the view bank
# also with hideDC), and one SHA-256 per object is taken over every fetched frame -- points, ceiling, floor, hold points or their absence -- and,
# for the view bank, fetch_last and the slot integers behind every call.  The suites hold the banks to the model only at TOL; this holds one
# checkout to another bit for bit.
# Run from the repository root:   python profiles/specframe_same_bits.py [--emu] [--parent DIR]
#   --emu          through the host-thread emulation of the HIP sources (tests/emu; no GPU needed) instead of the device
#   --parent DIR   also run in a checkout of the parent commit built at DIR (a child process, this file, cwd = DIR) and require equal digests
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402

SIZES = (16, 256)


def context(emu):
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import Context
    if emu:
        sys.path.insert(0, os.path.join("tests", "emu"))
        import build_emu
        lib = C.CDLL(build_emu.build(""))
        for name, (res, args) in H.ABI.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        H._lib = lib
    return Context(0)


def add_frames(h, got):
    for s in sorted(got):
        for p, ce, fl, hold in got[s]:
            h.update(b"F%d" % s + p.tobytes() + np.float64([ce, fl]).tobytes() + (b"-" if hold is None else hold.tobytes()))


def specbank_digest(ctx):
    from cubicsdr_amd.engine import SpectrumBank
    from tests import specbank_cases as K
    h, n = hashlib.sha256(), 0
    for F in SIZES:
        for calls, nan, events in ((K.CALLS, True, ()), (K.PEAK_CALLS, False, (2, 5))):
            data = K.make_inputs(F, sum(calls), nan=nan)
            starts = np.cumsum((0,) + calls[:-1]).tolist()
            sb = SpectrumBank(ctx, F, K.SLOTS, max(calls))
            got = K.run_plan(sb, data, K.call_plan(data, calls), lambda k: sb.set_peak_hold(True) if starts[k] in events else None)
            sb.close()
            add_frames(h, got)
            n += sum(len(v) for v in got.values())
    return h.hexdigest(), n


def viewbank_digest(ctx):
    from cubicsdr_amd.engine import ViewBank
    from tests import viewbank_cases as K
    from tests.util import synth_iq
    h, n = hashlib.sha256(), 0

    def run(vb, w, data, calls, events):
        nonlocal n
        for k0, call in K.call_plan(w, data, calls):
            if k0 in events:
                vb.set_peak_hold(True)
            K.apply_views(vb, w, k0, max(i for _, i in call) + 1)
            got = K.run_call(vb, w, data, call)
            add_frames(h, got)
            n += sum(len(v) for v in got.values())
            for s in sorted(w):
                h.update(repr(sorted(vb.slot_info(s).items())).encode() + vb.fetch_last(s).tobytes())
        vb.close()
    for F in SIZES:
        w, data = K.walks(F), K.make_inputs(F)
        for hide_dc in (False, True):
            vb = K.new_bank(ctx, F)
            vb.set_hide_dc(hide_dc)
            run(vb, w, data, K.CALLS, (1,) if hide_dc else ())
        n_items = sum(K.PEAK_CALLS)
        w = K.peak_walks(F, n_items)
        data = {}
        for s, v in w.items():
            x = synth_iq(sum(v["lens"]), float(K.RATE), K.FREQ, [("NBFM", K.FREQ + 55000.0), ("AM", K.FREQ + 10150.0)], seed=31 + s + F)
            data[s] = [x[k * v["lens"][0]:(k + 1) * v["lens"][0]] for k in range(n_items)]
        run(ViewBank(ctx, F, 3, max(K.PEAK_CALLS), 6 * 2 * F), w, data, K.PEAK_CALLS, (2, 5))
    return h.hexdigest(), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--emu", action="store_true")
    ap.add_argument("--parent", default=None)
    args = ap.parse_args()
    ctx = context(args.emu)
    mine = {"csdr_specbank": specbank_digest(ctx), "csdr_viewbank": viewbank_digest(ctx)}
    ctx.close()
    if not args.parent:
        for name, (d, n) in mine.items():
            print("%s %d %s" % (name, n, d))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + (["--emu"] if args.emu else []), cwd=args.parent, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip(), "the run on the parent checkout failed: " + (r.stderr.strip().splitlines() or ["?"])[-1]
    parent = {ln.split()[0]: (ln.split()[2], int(ln.split()[1])) for ln in r.stdout.strip().splitlines()[-2:]}
    where = "emulation" if args.emu else "device"
    for name, (d, n) in mine.items():
        print("%s, %s, F = 16 and 256, %d frames: sha256 %s; parent %s: %s" % (where, name, n, d, parent[name][0], "equal" if parent[name] == (d, n) else "DIFFERENT"))
    assert all(parent[k] == v for k, v in mine.items()), "parent and change differ"


if __name__ == "__main__":
    main()
