"""The host mirror's overlay bank (cubicsdr_amd/host/DemodOverlays.h: DemodOverlayBank), compiled with g++ against libcsdr_hip.so and exercised by
tests/cpp/test_overlay_host.cpp, and engine.parse_bmfont.  On the CPU: a host bank without a context composes the shared cases
(tests/overlay_cases.py) from a plan this test writes to a file; every picture and every laid-out string against tests/overlay_oracle.py, byte for
byte, and refused composes.  On the GPU: a device bank and a host bank fed the same plan give the same pictures."""
import os
import subprocess

import numpy as np
import pytest

from tests import overlay_cases as K
from tests import overlay_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_overlay_host.cpp")
TEXTS = [("101.25dB", 40, 12, O.CENTER, O.CENTER), ("[VRM] 9", -3, 2, O.RIGHT, O.BOTTOM), ("0_ #x", 7, -5, O.LEFT, O.TOP), ("", 1, 1, O.LEFT, O.TOP)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("overlay_host")), "test_overlay_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def _prim_words(prims):
    return "%d %s" % (len(prims), " ".join("%d %d %d %d %d %d %d %d %d %d %d" % (p[:4] + p[4] + p[5:]) for p in map(O.as_tuple, prims)))


def write_plan(tmp_path):
    """-> (bytes file, plan file, the bytes the program must write, counts)"""
    plan, data, want = [], [], []
    counts = dict(pictures=0, refused=0, texts=0)
    plan.append("font %d %d" % (K.FONT_W, K.FONT_H))
    data.append(K.FONT.tobytes())
    plan.append("glyphs %d %s" % (len(K.GLYPHS), " ".join(" ".join(str(g[k]) for k in ("id", "x", "y", "w", "h", "xoffset", "yoffset", "xadvance")) for g in K.GLYPHS)))
    from cubicsdr_amd.engine import overlay_prims
    for s, x, y, ha, va in TEXTS:
        plan.append("text %d %d %d %d %d 9 8 7 200 %d %s" % (x, y, ha, va, O.ADD, K.LINE_HEIGHT, s))
        want.append(overlay_prims(O.text(K.GLYPHS, K.LINE_HEIGHT, s, x, y, ha, va, (9, 8, 7, 200), O.ADD)).tobytes())
        counts["texts"] += 1
    for name, case in K.CASES.items():
        base = None if isinstance(case["base"], str) else case["base"]       # (the device base of a trace bank is the device tests')
        runs = case["runs"]
        plan.append("compose %d %d %d %d %d %s %s" % (case["W"], case["H"], case.get("cols", 1), base is not None, len(runs), " ".join("%d %d" % r for r in runs),
                                                      _prim_words(case["prims"])))
        if base is not None:
            data.append(base.tobytes())
        want.append(O.atlas(case["prims"], runs, case["W"], case["H"], case.get("cols", 1), base, K.FONT).tobytes())
        counts["pictures"] += 1
    ok, masked = "0 0 4 4 1 2 3 4 0 -1 0", "0 0 4 4 1 2 3 4 0 %d %d"
    for bad in ("0 8 1 0 1 0 1 1 " + ok, "8 16385 1 0 1 0 1 1 " + ok, "8 8 0 0 1 0 1 1 " + ok, "8 8 2 0 1 0 1 1 " + ok, "8 8 1 0 0 1 " + ok,
                "8 8 1 0 1 0 2 1 " + ok, "8 8 1 0 1 1 1 1 " + ok, "8 8 1 0 1 -1 1 1 " + ok, "8 8 1 0 1 0 1 1 0 0 4 4 1 2 3 4 3 -1 0", "8 8 1 0 1 0 1 1 0 0 -4 4 1 2 3 4 0 -1 0",
                "8 8 1 0 1 0 1 1 1048577 0 4 4 1 2 3 4 0 -1 0", "8 8 1 0 1 0 1 1 " + masked % (K.FONT_W - 3, 0), "8 8 1 0 1 0 1 1 " + masked % (0, K.FONT_H - 3),
                "8 8 1 0 1 0 1 1 " + masked % (0, -1), "8 8 1 0 17" + " 0 0" * 17 + " 1 " + ok):
        plan.append("badcompose " + bad)
        counts["refused"] += 1
    plan.append("font 0 0")
    plan.append("badcompose 8 8 1 0 1 0 1 1 " + masked % (0, 0))               # a mask and no font
    counts["refused"] += 1
    plan.append("compose 8 8 1 0 1 0 1 1 " + ok)
    want.append(O.atlas([(0, 0, 4, 4, (1, 2, 3, 4), 0)], [(0, 1)], 8, 8).tobytes())
    counts["pictures"] += 1
    p_d, p_plan = (os.path.join(str(tmp_path), n) for n in ("bytes.bin", "plan.txt"))
    with open(p_d, "wb") as f:
        f.write(b"".join(data))
    with open(p_plan, "w") as f:
        f.write("\n".join(plan) + "\n")
    return p_d, p_plan, b"".join(want), counts


def check_counts(stdout, counts, banks):
    st = next(ln for ln in stdout.splitlines() if ln.startswith("DONE ")).split()
    assert dict(zip(st[1::2], map(int, st[2::2]))) == dict(counts, banks=banks)


def test_host_bank_against_the_oracle(exe, tmp_path):
    p_d, p_plan, want, counts = write_plan(tmp_path)
    p_out = os.path.join(str(tmp_path), "out.bin")
    r = subprocess.run([exe, "cpu", p_d, p_plan, p_out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "overlay host test ok" in r.stdout
    check_counts(r.stdout, counts, 1)
    got = open(p_out, "rb").read()
    assert len(got) == len(want) and got == want, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)


@pytest.mark.gpu
def test_device_bank_and_host_bank_give_the_same_pictures(exe, tmp_path):
    p_d, p_plan, want, counts = write_plan(tmp_path)
    r = subprocess.run([exe, "gpu", p_d, p_plan], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "overlay host gpu ok" in r.stdout
    check_counts(r.stdout, counts, 2)


FNT = """info face="Synthetic Sans" size=16 bold=0 italic=0 charset="" unicode=0 stretchH=100 smooth=1 aa=1 padding=0,0,0,0 spacing=1,1
common lineHeight=19 base=15 scaleW=64 scaleH=32 pages=1 packed=0
page id=0 file="synthetic_0.png"
chars count=4
char id=48   x=10    y=2     width=7     height=11    xoffset=1     yoffset=4     xadvance=9     page=0  chnl=0
char id=32   x=0     y=0     width=0     height=0     xoffset=0     yoffset=0     xadvance=4     page=0  chnl=0
char id=74   x=58    y=21    width=6     height=11    xoffset=-2    yoffset=-1    xadvance=5     page=0  chnl=0

char id=46 x=3 y=30 width=2 height=2 xoffset=1 yoffset=13 xadvance=4 page=0 chnl=0
kernings count=1
kerning first=74 second=48 amount=-1
"""


def test_parse_bmfont():
    from cubicsdr_amd import engine as E
    f = E.parse_bmfont(FNT)
    assert (f["line_height"], f["base"], f["scale_w"], f["scale_h"], f["pages"]) == (19, 15, 64, 32, {0: "synthetic_0.png"})
    assert f["glyphs"].dtype == E.GLYPH_DTYPE
    assert [tuple(int(v) for v in g) for g in f["glyphs"]] == [(48, 10, 2, 7, 11, 1, 4, 9), (32, 0, 0, 0, 0, 0, 0, 4), (74, 58, 21, 6, 11, -2, -1, 5), (46, 3, 30, 2, 2, 1, 13, 4)]
    got = [O.as_tuple(p) for p in E.design_text(f["glyphs"], f["line_height"], "J 0.", 30, 20, "right", "bottom")]
    assert got == O.text([dict(zip(E.GLYPH_DTYPE.names, (int(v) for v in g))) for g in f["glyphs"]], 19, "J 0.", 30, 20, O.RIGHT, O.BOTTOM)
    assert got[0] == (30 - 22 - 2, 20 - 19 - 1, 6, 11, (255, 255, 255, 255), O.OVER, 58, 21)
    assert len(E.parse_bmfont("")["glyphs"]) == 0
