"""The host mirror's density bank (cubicsdr_amd/host/DemodDensity.h: DemodDensityBank), compiled with g++ -Wall against libcsdr_hip.so and exercised
by tests/cpp/test_density_host.cpp.  On the CPU: the header compiles and links, the constructor throws without a context, and
csdr_design_density_cover gives the header's example.  On the GPU: behind a small pipeline (M = 4, a spectrum bank behind the demodulator bank, a
spectrum over the wideband samples) DemodDensityBanks stepped through stepSpectrumBank / stepSpectrum hold what engine.DensityBank holds behind
the same executes; and a DemodDensityBank fed a plan of shared cases (tests/density_cases.py) as host items holds what engine.DensityBank holds
after the same steps -- every grid, peak and picture, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import density_cases as K
from tests import density_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_density_host.cpp")
PLAN_CASES = ["item_forms", "slot_lists", "decay", "tile_65_129"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("density_host")), "test_density_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def test_header_compiles_and_the_constructor_throws(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "density host test ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_host_banks_behind_the_pipeline_hold_what_the_engine_banks_hold(exe, tmp_path):
    """2.4 MS/s, M = 4, blocks of 40 000, two per execute, four executes; NBFM, AM, USB and a second NBFM.  Behind every execute
    the program's DemodDensityBanks step through stepSpectrumBank (a spectrum bank behind the demodulator bank) and stepSpectrum (a spectrum over
    every wideband sample, hideDC on); engine.DensityBank fed the same executes holds the same grids, peaks and pictures, byte for byte."""
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import Context, DemodBank, DensityBank, SDRPost, SpectrumBank, SpectrumProcessor
    from tests.util import demod_frequencies, synth_iq
    fs, M, block, center, nb, nexec, F, W, Hh = 2400000, 4, 40000, 100000000, 2, 4, 256, 96, 40
    kinds = [("NBFM", 12500), ("AM", 6000), ("USB", 5400), ("NBFM", 12500)]
    freqs = demod_frequencies(center, fs, len(kinds))
    x = synth_iq(nexec * nb * block, fs, center, [(k, f) for (k, _), f in zip(kinds, freqs)], seed=27)
    p_iq, p_slots, p_out = (os.path.join(str(tmp_path), n) for n in ("iq.bin", "slots.txt", "out.bin"))
    x.astype(np.complex64).tofile(p_iq)
    with open(p_slots, "w") as f:
        for (k, bw), fr in zip(kinds, freqs):
            f.write("%d %d %d\n" % (H.MODEM_BY_NAME[k], bw, fr))
    r = subprocess.run([exe, "pipe", p_iq, p_slots, p_out] + [str(v) for v in (fs, M, block, nb, nexec, center, F, W, Hh)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "density host pipe ok" in r.stdout, r.stdout + r.stderr
    got = open(p_out, "rb").read()
    slots, wide_frames = len(kinds), nb * (block // (2 * F)) + 2
    ctx = Context(0)
    post, bank, sb, sp = SDRPost(ctx, fs, M, block, nb), DemodBank(ctx, slots, nb), SpectrumBank(ctx, F, slots, 64), SpectrumProcessor(ctx, F, wide_frames)
    banks, wide = DensityBank(ctx, W, Hh, slots, 64, F), DensityBank(ctx, W, Hh, 1, wide_frames, F)
    want, frames_seen = [], 0
    try:
        sp.set_hide_dc(True, center_freq=center, bandwidth=fs, input_freq=center)
        for i, ((k, bw), fr) in enumerate(zip(kinds, freqs)):
            bank.configure(i, post, k, bw, fr)
        for e in range(nexec):
            xe = x[e * nb * block:(e + 1) * nb * block]
            post.execute(xe, nb, block, center)
            bank.execute(post)
            sb.process_bank(bank)
            frames_seen += sum(sb.frames(s) for s in range(slots))
            banks.step_specbank(sb, keep_q16=60000, weight=3)
            nf = sp.process(xe, nb, block, contiguous=True)
            assert nf > 20
            wide.step_spec(0, sp, 1, nf - 1, keep_q16=62000, weight=2)
            for d, s in [(banks, s) for s in range(slots)] + [(wide, 0)]:
                grid = d.fetch(s)
                assert grid.max() == d.peak(s)
                want.append(grid.tobytes() + np.uint32(d.peak(s)).tobytes())
        assert frames_seen > 8 and all(banks.peak(s) > 3 for s in range(slots)) and wide.peak(0) > 40
        want.append(banks.render([(s, 0) for s in range(slots)], 2).tobytes())
        want.append(wide.render([(0, 40)]).tobytes())
    finally:
        for o in (wide, banks, sp, sb, bank, post, ctx):
            o.close()
    assert int(next(ln for ln in r.stdout.splitlines() if ln.startswith("GRIDS ")).split()[1]) == nexec * (slots + 1)
    want = b"".join(want)
    assert len(got) == len(want) and got == want, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)


@pytest.mark.gpu
def test_host_bank_holds_what_the_engine_bank_holds(exe, tmp_path):
    from cubicsdr_amd.engine import Context, DensityBank
    kinds = {"spectrum": 0, "y": 1}
    floats, plan, at = [], [], 0

    def put(a):
        nonlocal at
        a = np.asarray(a, np.float32).ravel()
        floats.append(a)
        at += a.size
        return at - a.size
    ctx = Context(0)
    db = DensityBank(ctx, 8, 8, 1, K.MAX_FRAMES, K.MAX_POINTS)
    want, counts = [], dict(steps=0, fetched=0, pictures=0)
    try:
        for name in PLAN_CASES:
            case = K.CASES[name]
            pal = D.DEFAULT_PALETTE if case.get("palette") is None else case["palette"]
            plan.append("setup %d %d %d %d %d" % (case["W"], case["H"], case["slots"], K.MAX_FRAMES, K.MAX_POINTS))
            plan.append("palette %d" % put(pal.astype(np.float32)))
            db.setup(case["W"], case["H"], case["slots"], K.MAX_FRAMES, K.MAX_POINTS)
            db.set_palette(pal)
            for items in case["steps"]:
                words = []
                for it in items:
                    off = -1 if it.get("points") is None else put(it["points"])
                    layout = it.get("layout", 0)
                    words.append("%d %d %d %d %d %d %d %d %d" % (it["slot"], off, it["n"], it["frames"], it.get("stride_floats", it["n"] * (1 + layout)), layout,
                                                                 kinds[it.get("kind", "spectrum")], it.get("keep_q16", 65536), it.get("weight", 1)))
                plan.append("step %d %s" % (len(items), " ".join(words)))
                db.step(items)
                counts["steps"] += 1
                for s in range(case["slots"]):
                    plan.append("fetch %d" % s)
                    want.append(db.fetch(s).tobytes() + np.uint32(db.peak(s)).tobytes())
                    counts["fetched"] += 1
            plan.append("render %d %d %s" % (case.get("cols", 1), len(case["views"]), " ".join("%d %d" % v for v in case["views"])))
            pic = db.render(case["views"], case.get("cols", 1))
            assert (pic == K.expected(name)[1]).all()
            want.append(pic.tobytes())
            counts["pictures"] += 1
    finally:
        db.close()
        ctx.close()
    p_f, p_plan, p_out = (os.path.join(str(tmp_path), n) for n in ("floats.bin", "plan.txt", "out.bin"))
    np.concatenate(floats).astype(np.float32).tofile(p_f)
    with open(p_plan, "w") as f:
        f.write("\n".join(plan) + "\n")
    r = subprocess.run([exe, "gpu", p_f, p_plan, p_out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "density host gpu ok" in r.stdout, r.stdout + r.stderr
    st = next(ln for ln in r.stdout.splitlines() if ln.startswith("DONE ")).split()
    assert dict(zip(st[1::2], map(int, st[2::2]))) == counts
    got, want = open(p_out, "rb").read(), b"".join(want)
    assert len(got) == len(want) and got == want, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
