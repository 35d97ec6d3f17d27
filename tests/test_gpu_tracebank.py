"""The trace bank on the device: every shared case (tests/tracebank_cases.py) against the restated rule (tests/trace_oracle.py), byte for byte, from
host points and from the same points in device memory; and what only the device path has -- the points of a spectrum bank, a view bank and a scope
bank rendered where they lie in HBM against the same points fetched and rendered as host items, two renders of different sizes in a row, the picture
left on the device and read back."""
import ctypes as C

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests import trace_oracle as O
from tests import tracebank_cases as K

pytestmark = pytest.mark.gpu
F, SLOTS, FRAMES = 64, 3, 3


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tb(ctx):
    from cubicsdr_amd.engine import TraceBank
    t = TraceBank(ctx, max_items=64, max_points=1 << 21)
    yield t
    t.close()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", list(K.CASES))
def test_case(ctx, tb, name, dev):
    K.check_case(ctx, tb, name, dev=dev)


def test_refusals_change_nothing(tb):
    assert K.check_refusals(tb) >= 12


def _iq(seed, n):
    r = np.random.default_rng(seed)
    t = np.arange(n)
    return (np.exp(2j * np.pi * (0.05 + 0.1 * seed) * t) * (0.2 + 0.1 * seed) + 0.05 * (r.standard_normal(n) + 1j * r.standard_normal(n))).astype(np.complex64)


def _spectra_as_host_items(bank, slots, with_hold=True):
    items = []
    for s in slots:
        f = bank.frames(s) - 1
        if f < 0:
            items.append(None)
            continue
        pts, _, _ = bank.fetch(s, f)
        hold = bank.fetch_hold(s, f) if with_hold else None
        items.append(dict(kind="spectrum", points=pts, layout=1, hold=hold))
    return items


def _check_spectra(tb, bank, had_hold):
    K.set_colors(tb, None)
    slots = [2, 0, 1, 0]
    want_items = _spectra_as_host_items(bank, slots)
    if had_hold:
        assert any(it.get("hold") is not None for it in want_items)
    for W, Hh, cols in ((48, 20, 2), (F, 33, 1), (150, 16, 4)):
        got = tb.render_spectra(bank, slots, W, Hh, atlas_cols=cols)
        assert (got == tb.render(want_items, W, Hh, cols)).all() and (got == O.atlas(want_items, W, Hh, cols)).all(), (W, Hh, cols)
    got = tb.render_spectra(bank, slots, 48, 20, hold=False)
    assert (got == O.atlas(_spectra_as_host_items(bank, slots, False), 48, 20)).all()
    assert (tb.render_spectra(bank, [0], 40, 10, frame=0) == O.atlas([dict(kind="spectrum", points=bank.fetch(0, 0)[0], layout=1, hold=bank.fetch_hold(0, 0))], 40, 10)).all()


def test_render_spectra_of_a_spectrum_bank(ctx, tb):
    from cubicsdr_amd.engine import SpectrumBank
    bank = SpectrumBank(ctx, F, SLOTS + 1, FRAMES)
    try:
        bank.set_peak_hold(True)
        for k in range(3):
            bank.process([(s, _iq(s + 3 * k, F)) for s in range(SLOTS) for _ in range(FRAMES if s else 1)])
        _check_spectra(tb, bank, True)
        assert (tb.render_spectra(bank, [SLOTS], 8, 4) == 0).all()          # a slot without frames: an empty tile
    finally:
        bank.close()


def test_render_spectra_of_a_view_bank(ctx, tb):
    from cubicsdr_amd.engine import ViewBank
    bank = ViewBank(ctx, F, SLOTS, FRAMES, 4096)
    try:
        bank.set_peak_hold(True)
        for s in range(SLOTS):
            bank.set_view(s, 100000000 + 20000 * s, 200000)
        for k in range(3):
            bank.process([(s, _iq(s + 3 * k, 4096), 100000000, 2400000) for s in range(SLOTS)])
        assert all(bank.frames(s) > 0 for s in range(SLOTS))
        _check_spectra(tb, bank, False)                                     # (whether a frame carries hold points is the bank's countdown rule)
    finally:
        bank.close()


def test_render_scopes(ctx, tb):
    from cubicsdr_amd.engine import ScopeBank
    L = 64
    bank = ScopeBank(ctx, L, 4, 1, 4 * L)
    try:
        r = np.random.default_rng(5)
        frames = [dict(data=(1.5 * r.uniform(-1, 1, n)).astype(np.float32), channels=ch, type=ty, sample_rate=48000, input_rate=48000)
                  for n, ch, ty in ((100, 1, 0), (2 * L, 2, 1), (2 * L, 2, 2))]
        bank.process([(s, f) for s, f in enumerate(frames)])
        K.set_colors(tb, None)
        slots = [1, 0, 2, 3, 1]
        items = []
        for s in slots:
            it = bank.fetch(s, 0, False) if bank.frames(s) else None
            if it is None:
                items.append(None)
                continue
            xy = it["mode"] == 2
            items.append(dict(kind=1 + it["mode"], points=it["points"], layout=0 if xy else 1))
        assert [None if it is None else it["kind"] for it in items] == [2, 1, 3, None, 2]
        for W, Hh, cols in ((40, 24, 2), (130, 9, 5)):
            got = tb.render_scopes(bank, slots, W, Hh, atlas_cols=cols)
            assert (got == tb.render(items, W, Hh, cols)).all() and (got == O.atlas(items, W, Hh, cols)).all(), (W, Hh, cols)
    finally:
        bank.close()


def test_two_sizes_in_a_row_and_the_device_view(ctx, tb):
    big, small = K.CASES["rows_in_groups"], K.CASES["atlas"]
    K.set_colors(tb, None)
    for case in (big, small, big):
        assert tb.render(case["items"], case["W"], case["H"], case.get("cols", 1), fetch=False) is None
        p, w, h = tb.device_view()
        want = K.expected(case)
        assert (h, w) == want.shape[:2]
        back = np.empty_like(want)
        H.check(H.lib().csdr_dev_download(ctx.h, back.ctypes.data_as(C.c_void_p), C.c_void_p(p), back.nbytes))
        assert (back == want).all()
        assert (tb.render(case["items"], case["W"], case["H"], case.get("cols", 1)) == want).all()
