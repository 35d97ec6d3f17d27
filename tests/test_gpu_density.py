"""The density bank on the device: every shared case (tests/density_cases.py) against the restated rule (tests/density_oracle.py), count for count and
byte for byte, from host points and from the same points in device memory; and what only the device path has -- one frame against the trace bank's
picture of the same item (two objects, no oracle), a spectrum's and a spectrum bank's frames stepped where they lie in HBM against the oracle fed
what the fetches return, the producer's next process issued straight behind a step, view-bank points as device items, and the picture left on the
device as the base of an overlay."""
import ctypes as C

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests import density_cases as K
from tests import density_oracle as D
from tests.util import demod_frequencies, synth_iq

pytestmark = pytest.mark.gpu
F = 256


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def db(ctx):
    from cubicsdr_amd.engine import DensityBank
    d = DensityBank(ctx, 8, 8, 1, K.MAX_FRAMES, K.MAX_POINTS)
    yield d
    d.close()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(K.CASES))
def test_case(ctx, db, name, dev):
    K.check_case(ctx, db, name, dev=dev)


def test_refusals_change_nothing(db):
    assert K.check_refusals(db) >= 12


def test_one_frame_is_the_trace_banks_picture(ctx, db):
    """keep 0, weight 1, full 1, palette[0] = bg, palette[255] = the line colour with the bg's alpha: csdr_tracebank_render of the same items"""
    from cubicsdr_amd.engine import TraceBank
    r = np.random.default_rng(3)
    W, Hh, cols = 130, 37, 2
    ys = [r.uniform(-0.1, 1.1, n).astype(np.float32) for n in (700, 130, 40)]
    bg, line = (10, 20, 30, 200), (250, 128, 3)
    tb = TraceBank(ctx, max_items=8, max_points=4096)
    try:
        tb.set_colors(bg=bg, line=line)
        want = tb.render([dict(kind="spectrum", points=y) for y in ys], W, Hh, cols)
    finally:
        tb.close()
    pal = np.zeros((256, 4), np.uint8)
    pal[:] = (1, 2, 3, 4)
    pal[0], pal[255] = bg, line + (bg[3],)
    db.setup(W, Hh, 3, 4, 4096)
    db.set_palette(pal)
    db.step([dict(slot=s, points=r.uniform(0, 1, 50).astype(np.float32), n=50, frames=1) for s in range(3)])        # what keep 0 forgets
    db.step([dict(slot=s, points=y, n=y.size, frames=1, keep_q16=0, weight=1) for s, y in enumerate(ys)])
    got = db.render([(s, 1) for s in range(3)], cols)
    assert want[:Hh].any() and K.mismatch(got, want) is None, K.mismatch(got, want)


@pytest.mark.parametrize("hide_dc", [False, True], ids=["plain", "hide_dc"])
def test_step_spec(ctx, db, hide_dc):
    from cubicsdr_amd.engine import SpectrumProcessor
    from tests.waterfall_cases import noise
    frames, W, Hh = 40, 100, 33
    sp = SpectrumProcessor(ctx, F, max_frames=frames)
    try:
        sp.set_hide_dc(hide_dc, center_freq=100000000, bandwidth=240000, input_freq=100000000)
        x = noise(frames * 2 * F, F)
        assert sp.process(x, 1, x.size, contiguous=True) == frames
        pts = np.stack([sp.fetch(f)[0][1::2] for f in range(frames)])
        if hide_dc:                                       # the overwrite did change something in what the fetch returns
            sp.set_hide_dc(False)
            assert any(not np.array_equal(sp.fetch(f)[0][1::2], pts[f]) for f in range(frames))
            sp.set_hide_dc(True)
        db.setup(W, Hh, 2, frames, F)
        db.step_spec(1, sp, 0, frames)
        db.step_spec(0, sp, 3, frames - 5, weight=2)
        twin = D.Bank(W, Hh, 2)
        twin.step([dict(slot=1, points=pts, n=F, frames=frames), dict(slot=0, points=pts[3:frames - 2], n=F, frames=frames - 5, weight=2)])
        for s in range(2):
            assert K.mismatch(db.fetch(s), twin.count[s]) is None, (s, K.mismatch(db.fetch(s), twin.count[s]))
            assert db.peak(s) == twin.peak(s) > 2
        assert H.lib().csdr_density_step_spec(db.h, 0, sp.h, 1, frames, 65536, 1) == -1         # frames outside the last process
        assert np.array_equal(np.stack([sp.fetch(f)[0][1::2] for f in range(frames)]), pts)
    finally:
        sp.close()


@pytest.fixture(scope="module")
def pipeline(ctx):
    """2.4 MS/s, M = 4, blocks of 40 000, two per execute; NBFM, AM, USB, a QPSK slot and an inactive one, a spectrum bank of fftSize 256 behind them"""
    from cubicsdr_amd.engine import DemodBank, SDRPost, SpectrumBank
    fs, M, block, center, nb = 2400000, 4, 40000, 100000000, 2
    kinds, bws = ["NBFM", "AM", "USB", "QPSK", "NBFM"], [12500, 6000, 5400, 200000, 12500]
    freqs = demod_frequencies(center, fs, len(kinds))
    x = synth_iq(4 * nb * block, fs, center, list(zip(["NBFM", "AM", "USB", "NBFM", "NBFM"], freqs)), seed=41)
    post, bank = SDRPost(ctx, fs, M, block, nb), DemodBank(ctx, len(kinds), nb)
    for i, k in enumerate(kinds):
        (bank.configure_digital if k == "QPSK" else bank.configure)(i, post, k, bws[i], freqs[i])
    bank.set_active(4, False)
    sb = SpectrumBank(ctx, F, 6, 64)
    state = dict(e=0)

    def run():
        e = state["e"]
        state["e"] += 1
        post.execute(x[e * nb * block:(e + 1) * nb * block], nb, block, center)
        bank.execute(post)
        sb.process_bank(bank)
    yield dict(run=run, sb=sb, slots=len(kinds))
    for o in (sb, bank, post):
        o.close()


def _bank_points(sb, slots):
    return [np.stack([sb.fetch(s, f)[0][1::2] for f in range(sb.frames(s))]) if sb.frames(s) else None for s in range(slots)]


def test_step_specbank_and_issue_order(ctx, db, pipeline):
    """the oracle is fed csdr_specbank_fetch; the producer's next process is issued straight behind every step, and the counts are fetched only then"""
    sb, run = pipeline["sb"], pipeline["run"]
    W, Hh = 96, 40
    db.setup(W, Hh, 4, 64, F)                             # fewer slots than the spectrum bank: the smaller count bounds the walk
    twin = D.Bank(W, Hh, 4)
    run()
    total = 0
    for rnd in range(3):
        pts = _bank_points(sb, 4)
        total += sum(0 if p is None else len(p) for p in pts)
        db.step_specbank(sb, keep_q16=60000, weight=3)
        run()                                             # rewrites the points the step reads: on the device it has to come behind the step
        twin.step([dict(slot=s, points=p, n=F, frames=0 if p is None else len(p), keep_q16=60000, weight=3) for s, p in enumerate(pts)])
        for s in range(4):
            assert K.mismatch(db.fetch(s), twin.count[s]) is None, (rnd, s, K.mismatch(db.fetch(s), twin.count[s]))
    assert total > 8 and all(twin.peak(s) > 3 for s in range(4))


def test_step_views(ctx, db):
    from cubicsdr_amd.engine import ViewBank

    def _iq(seed, n):
        r = np.random.default_rng(seed)
        return (np.exp(2j * np.pi * (0.05 + 0.1 * seed) * np.arange(n)) * (0.2 + 0.1 * seed) + 0.05 * (r.standard_normal(n) + 1j * r.standard_normal(n))).astype(np.complex64)
    slots, frames, W, Hh = 3, 3, 48, 20
    vb = ViewBank(ctx, 64, slots, frames, 4096)
    try:
        for s in range(slots):
            vb.set_view(s, 100000000 + 20000 * s, 200000)
        for k in range(3):
            vb.process([(s, _iq(s + 3 * k, 4096), 100000000, 2400000) for s in range(slots)])
        assert all(vb.frames(s) > 0 for s in range(slots))
        db.setup(W, Hh, slots, frames, 64)
        twin = D.Bank(W, Hh, slots)
        db.step_views(vb)
        twin.step([dict(slot=s, points=np.stack([vb.fetch(s, f)[0][1::2] for f in range(vb.frames(s))]), n=64, frames=vb.frames(s)) for s in range(slots)])
        for s in range(slots):
            assert K.mismatch(db.fetch(s), twin.count[s]) is None and twin.peak(s) >= 1
    finally:
        vb.close()


def test_overlay_over_the_device_view(ctx, db):
    from cubicsdr_amd.engine import DevicePointer, OverlayBank, overlay_prims
    K.check_case(ctx, db, "item_forms")
    case = K.CASES["item_forms"]
    W, Hh, cols = case["W"], case["H"], case["cols"]
    pic = db.render(case["views"], cols)
    assert db.render(case["views"], cols, fetch=False) is None
    p, w, h = db.device_view()
    assert (h, w) == pic.shape[:2]
    back = np.empty_like(pic)
    H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(p), back.nbytes))
    assert (back == pic).all()
    n_tiles = (h // Hh) * cols
    prims = overlay_prims([(3, 2, 40, 9, (200, 10, 20, 128), 0), (0, 0, W, 1, (1, 255, 1, 255), 2)])
    ov = OverlayBank(ctx, max_tiles=8, max_prims=16)
    try:
        on_device = ov.compose(prims, [(0, 2)] * n_tiles, W, Hh, cols, base=DevicePointer(p, w * h))
        on_host = ov.compose(prims, [(0, 2)] * n_tiles, W, Hh, cols, base=pic)
        assert (on_device == on_host).all() and (on_device != pic).any()
    finally:
        ov.close()


def test_two_sizes_in_a_row(ctx, db):
    for name in ("tile_300_129", "header_example", "tile_300_129"):
        K.check_case(ctx, db, name, dev=True)
