"""The overlay planners (csdr_design_freq_scale, _db_grid, _db_labels, _demod_marker, _text: design.hpp through libcsdr_hip.so, no device) against the
numpy restatement (tests/overlay_oracle.py) and against pins worked out from the reference's formulas (src/panel/SpectrumPanel.cpp:117-303,
src/visual/PrimaryGLContext.cpp:89-197)."""
import math

import numpy as np
import pytest

from cubicsdr_amd import engine as E
from tests import overlay_cases as K
from tests import overlay_oracle as O


def _same_scale(got, want):
    for k in ("step_mhz", "precision", "font_size", "tick_rows", "label_row"):
        assert got[k] == want[k], k
    assert got["tick_top"] == want["tick_top"] and got["label_y"] == want["label_y"]
    assert len(got["ticks"]) == len(want["ticks"])
    for a, b in zip(got["ticks"], want["ticks"]):
        assert abs(a["m"] - b["m"]) <= 1e-12 and a["label"] == b["label"] and a["major"] == b["major"] and a["value"] == b["value"], (a, b)
        if abs((b["m"] + 1) * 0.5 * got["_w"] - round((b["m"] + 1) * 0.5 * got["_w"])) > 1e-6:
            assert a["column"] == b["column"]


SCALES = [(100030000, 2400000, 1024, 200, 1.0), (433920000, 250000, 800, 100, 1.0), (1090000000, 61440000, 1920, 256, 1.0), (7100000, 48000, 512, 135, 1.0),
          (7100000, 48000, 512, 136, 1.5), (145500000, 10000000, 300, 64, 2.0), (500000, 2000000, 640, 480, 1.0), (-3000000, 1500000, 333, 77, 1.0),
          (98700000, 3200001, 1001, 33, 1.25), (2400000000, 20000000, 16384, 16384, 1.0), (100000000, 1000000000, 100, 10, 1.0)]


@pytest.mark.parametrize("freq,bw,w,h,fs", SCALES)
def test_freq_scale_against_the_oracle(freq, bw, w, h, fs):
    got = E.design_freq_scale(freq, bw, w, h, fs)
    got["_w"] = w
    _same_scale(got, O.freq_scale(freq, bw, w, h, fs))


def test_freq_scale_pin_100_03_mhz():
    s = E.design_freq_scale(100030000, 2400000, 1024, 200)
    t = s["ticks"]
    assert s["step_mhz"] == 0.1 and s["precision"] == 1 and len(t) == 24
    assert abs(t[0]["m"] - (-0.941666666667)) < 1e-9 and t[0]["label"] == "98.9" and abs(t[-1]["m"] - 0.975) < 1e-9 and t[-1]["label"] == "101.2"
    for k, tick in enumerate(t):
        # the reference's formula: leftFreq 98.83 MHz, firstMhz 98 MHz, so tick k lies at 98.9 + 0.1 k MHz
        m = ((98900000 + 100000 * k) - 98830000) / 2400000 * 2 - 1
        assert abs(tick["m"] - m) < 1e-9 and tick["label"] == "%.1f" % (98.9 + 0.1 * k)
        x = (m + 1) * 0.5 * 1024
        assert abs(x - round(x)) > 0.1 and tick["column"] == math.floor(x)
    assert [c["column"] for c in t[:3]] == [29, 72, 115]
    assert [c["label"] for c in t if c["major"]] == ["99.0", "100.0", "101.0"]
    # (label_y lies on a row boundary: (1 - 0.91) * 100 is 9 less one rounding, so its row is not pinned)
    assert (s["font_size"], s["tick_rows"]) == (16, 2) and s["label_row"] in (8, 9) and s["tick_top"] == 1.0 - 5.0 / 200 and s["label_y"] == 1.0 - 18.0 / 200


def test_freq_scale_further_pins():
    t = E.design_freq_scale(433920000, 250000, 800, 100)["ticks"]
    assert [(c["label"], c["major"]) for c in t] == [("433.8", False), ("433.9", False), ("434.0", True)]
    assert all(abs(c["m"] - m) < 1e-9 for c, m in zip(t, (-0.96, -0.16, 0.64)))
    s = E.design_freq_scale(1090000000, 61440000, 1920, 256)
    t = s["ticks"]
    assert s["step_mhz"] == 2.5 and len(t) == 24 and t[0]["label"] == "1061.5" and t[-1]["label"] == "1119.0"
    assert all(c["major"] == c["label"].endswith(".0") for c in t) and sum(c["major"] for c in t) == 12
    s = E.design_freq_scale(7100000, 48000, 512, 100)
    assert s["precision"] == 2 and s["step_mhz"] == 0.01 and [c["label"] for c in s["ticks"]] == ["7.08", "7.09", "7.10", "7.11", "7.12"]
    assert not any(c["major"] for c in s["ticks"]) and s["font_size"] == 12 and s["label_y"] == 1.0 - 16.0 / 100


def test_freq_scale_refusals():
    import cubicsdr_amd.hip as H
    sc = H.FreqScale()
    for bad in ((1, 0, 10, 10, 1.0), (1, 10, 0, 10, 1.0), (1, 10, 10, 16385, 1.0), (1, 10, 10, 10, 0.0)):
        assert H.lib().csdr_design_freq_scale(*bad, sc, None, 0) == -1, bad
    ticks = (H.FreqTick * 2)()
    assert H.lib().csdr_design_freq_scale(100030000, 2400000, 1024, 200, 1.0, sc, ticks, 2) == -5 and sc.n_ticks == 24


@pytest.mark.parametrize("floor,ceil", [(1, 126), (0, 95), (0, 20), (0, 25), (0, 30), (-10, 139.5), (5, 5), (3, 1), (0, 4999), (0, 5001), (0.5, 97.25), (-120, -20)])
def test_db_grid_against_the_oracle(floor, ceil):
    got, want = E.design_db_grid(floor, ceil), O.db_grid(floor, ceil)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a["alpha"] == b["alpha"] and a["step"] == b["step"] and a["p"].shape == b["p"].shape and (a["p"] == b["p"]).all()


def test_db_grid_pins():
    g = E.design_db_grid(1, 126)
    assert [(r["step"], r["alpha"]) for r in g] == [(100.0, 1.0), (10.0, 1.0)]
    assert np.allclose(g[0]["p"], [0.8, 1.6, 2.4], rtol=0, atol=1e-12)
    assert np.allclose(g[1]["p"], 0.08 * np.arange(1, 15), rtol=0, atol=1e-12) and np.count_nonzero(g[1]["p"] <= 1.0) == 12
    g = E.design_db_grid(0, 95)
    assert (g[0]["step"], g[0]["alpha"]) == (100.0, 0.5)
    assert [r["step"] for r in E.design_db_grid(0, 25)] == [10.0, 1.0] and [r["alpha"] for r in E.design_db_grid(0, 25)] == [0.5, 0.5]


def test_db_labels():
    for floor, ceil, n, ofs in ((1, 126, 1024, 0.0), (0.001, 3.5, 2048, -30.0), (2, 2, 1024, 0.0), (1, 2, 0, 0.0), (0, 1, 512, 5.0)):
        assert E.design_db_labels(floor, ceil, n, ofs) == O.db_labels(floor, ceil, n, ofs)
    assert E.design_db_labels(1, 126, 1024) == ("%.1fdB" % (20 * math.log10(252 / 1024)), "%.1fdB" % (20 * math.log10(2 / 1024)))
    assert E.design_db_labels(2, 2, 1024) == ("", "") and E.design_db_labels(1, 2, 0) == ("", "")


MARKERS = [(100200000, 200000, O.BOTH, 100000000, 2400000, O.CENTERLINE), (100200000, 3000, O.USB, 100000000, 2400000, 0), (99700000, 3000, O.LSB, 100000000, 2400000, O.CENTERLINE),
           (100000000, 18749, O.BOTH, 100000000, 2400000, 0), (100000000, 18751, O.BOTH, 100000000, 2400000, 0),          # either side of 16 / viewWidth at 1024
           (101300000, 500000, O.BOTH, 100000000, 2400000, O.CENTERLINE), (90000000, 100000, O.BOTH, 100000000, 2400000, O.CENTERLINE)]


@pytest.mark.parametrize("args", MARKERS)
@pytest.mark.parametrize("view", [(1024, 200), (130, 33), (7, 5)])
def test_demod_marker_against_the_oracle(args, view):
    got, want = E.design_demod_marker(*args, *view, rgb=(200, 50, 25)), O.demod_marker(*args, *view, rgb=(200, 50, 25))
    for k in ("ux", "ofs_left", "ofs_right", "label_v", "narrow", "halign", "label_x", "label_y", "prefix"):
        assert got[k] == want[k], k
    assert [O.as_tuple(p) for p in got["prims"]] == [O.as_tuple(p) for p in want["prims"]]


def test_demod_marker_pins():
    m = E.design_demod_marker(100200000, 200000, "both", 100000000, 2400000, O.CENTERLINE, 1024, 200, rgb=(200, 50, 25))
    # uxPos = (1.4 / 2.4 - 0.5) * 2 = 1 / 6, ofs = 1 / 12; labelHeight 0.1 of NDC: the ground covers the lowest 2 * 20 / viewHeight, 20 rows
    assert abs(m["ux"] - 1 / 6) < 1e-6 and abs(m["ofs_left"] - 1 / 12) < 1e-6 and m["ofs_left"] == m["ofs_right"] and not m["narrow"]
    # columns (1 + 1 / 12) * 512 = 554.67 and (1 + 1 / 6) * 512 = 597.33; the right edge 640, the ground's top row 180 and the label's row 190 lie on
    # pixel boundaries in exact arithmetic and fall to either side in float
    g, band, line = (O.as_tuple(p) for p in m["prims"])
    assert g[0] == 554 and g[1] in (179, 180) and g[0] + g[2] in (639, 640) and g[1] + g[3] == 200 and g[4:] == ((0, 0, 0, 89), O.OVER, -1, 0)
    assert band[:2] == (554, 0) and band[2] == g[2] and band[3] == 200 and band[4:] == ((200, 50, 25, 51), O.ADD, -1, 0)
    assert line == (597, 0, 1, 200, (200, 50, 25, 128), O.ADD, -1, 0)
    assert (m["halign"], m["label_x"]) == (O.CENTER, 597) and m["label_y"] in (189, 190)
    usb = E.design_demod_marker(100200000, 3000, "usb", 100000000, 2400000, 0, 1024, 200)
    lsb = E.design_demod_marker(100200000, 3000, "lsb", 100000000, 2400000, 0, 1024, 200)
    assert usb["ofs_left"] == 0 and usb["ofs_right"] > 0 and usb["halign"] == O.LEFT and lsb["ofs_right"] == 0 and lsb["ofs_left"] > 0 and lsb["halign"] == O.RIGHT
    assert usb["narrow"] and len(usb["prims"]) == 3 and O.as_tuple(usb["prims"][2])[4:6] == ((255, 255, 255, 51), O.ADD)
    # ofs * 2 < 16 / 1024: the bandwidth either side of 2400000 / 128 = 18750
    assert E.design_demod_marker(100000000, 18749, "both", 100000000, 2400000, 0, 1024, 200)["narrow"]
    assert not E.design_demod_marker(100000000, 18751, "both", 100000000, 2400000, 0, 1024, 200)["narrow"]
    prefixes = {0: "", O.DELTA_LOCK: "[V] ", O.RECORDING: "[R] ", O.MUTED: "[M] ", O.SOLO: "[S] ", O.MUTED | O.SOLO: "[M] ", O.DELTA_LOCK | O.RECORDING | O.MUTED: "[VRM] ",
                O.DELTA_LOCK | O.RECORDING | O.SOLO: "[VRS] ", O.RECORDING | O.SOLO | O.CENTERLINE: "[RS] "}
    for flags, want in prefixes.items():
        assert E.design_demod_marker(100000000, 10000, "both", 100000000, 2400000, flags, 64, 33)["prefix"] == want == O.demod_marker(1, 1, 0, 1, 2, flags, 8, 8)["prefix"]


@pytest.mark.parametrize("halign", [O.LEFT, O.CENTER, O.RIGHT])
@pytest.mark.parametrize("valign", [O.TOP, O.CENTER, O.BOTTOM])
def test_text_alignments(halign, valign):
    g = K.glyph_array()
    for s, x, y in (("101.25dB", 40, 12), ("[VRM] 9", -3, 2), ("0_ #", 7, -5), ("9", 0, 0)):
        got = E.design_text(g, K.LINE_HEIGHT, s, x, y, halign, valign, (1, 2, 3, 200), "add")
        want = O.text(K.GLYPHS, K.LINE_HEIGHT, s, x, y, halign, valign, (1, 2, 3, 200), O.ADD)
        assert [O.as_tuple(p) for p in got] == want, s


def test_text_missing_character_and_empty_string():
    g = K.glyph_array()
    assert [O.as_tuple(p) for p in E.design_text(g, K.LINE_HEIGHT, "1x2", 5, 5, "center", "center")] == [O.as_tuple(p) for p in E.design_text(g, K.LINE_HEIGHT, "12", 5, 5, "center", "center")]
    assert len(E.design_text(g, K.LINE_HEIGHT, "", 5, 5)) == 0 and len(E.design_text(g, K.LINE_HEIGHT, "xyz", 5, 5)) == 0
    assert len(E.design_text(g, K.LINE_HEIGHT, " _", 5, 5)) == 0                     # glyphs without a picture
    one = O.as_tuple(E.design_text(g, K.LINE_HEIGHT, "0", 10, 20)[0])                # the first of the two '0' records
    g0 = K.GLYPHS[0]
    assert one == (10 + g0["xoffset"], 20 + g0["yoffset"], g0["w"], g0["h"], (255, 255, 255, 255), O.OVER, g0["x"], g0["y"])
    # odd widths and a negative anchor: floor division
    adv = sum(next(q for q in K.GLYPHS if q["id"] == ord(c))["xadvance"] for c in "12")
    p = O.as_tuple(E.design_text(g, 9, "12", -7, -7, "center", "center")[0])
    g1 = next(q for q in K.GLYPHS if q["id"] == ord("1"))
    assert p[0] == -7 - adv // 2 + g1["xoffset"] and p[1] == -7 - 9 // 2 + g1["yoffset"]


def test_spectrum_annotations_order():
    kw = dict(markers=[dict(freq=100200000, bandwidth=200000, label="[M] 10", flags=O.CENTERLINE, rgb=(200, 50, 50)), dict(freq=99500000, bandwidth=3000, sideband=O.USB, label="5")])
    got = E.spectrum_annotations(130, 33, 100030000, 2400000, 1.0, 126.0, 1024, K.glyph_array(), K.LINE_HEIGHT, **kw)
    want = O.spectrum_annotations(130, 33, 100030000, 2400000, 1.0, 126.0, 1024, K.GLYPHS, K.LINE_HEIGHT, **kw)
    assert [O.as_tuple(p) for p in got] == want
    modes = [p[5] for p in want]
    n_grid = sum(1 for p in want if p[5] == O.ADD and p[3] == 1 and p[2] == 130)
    assert n_grid >= 1 and modes[:n_grid] == [O.ADD] * n_grid and want[n_grid][6] < 0 and want[n_grid][5] == O.OVER      # grid first, then the ticks
