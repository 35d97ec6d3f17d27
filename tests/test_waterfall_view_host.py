"""The host mirror's viewport (cubicsdr_amd/host/WaterfallPanel.h: WaterfallPanel::renderView), compiled with g++ against libcsdr_hip.so and exercised by
tests/cpp/test_waterfall_view_host.cpp.  On the CPU: a host panel without a context, fed a plan of lines, gradients and views this test writes to a
file, every picture against the numpy model of tests/waterfall_view_cases.py, bit for bit.  On the GPU: a device panel and a host panel fed the same
plan hold the same views."""
import os
import subprocess

import numpy as np
import pytest

from tests import waterfall_view_cases as K
from tests.waterfall_cases import STOPS5, PanelModel, np_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_waterfall_view_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("waterfall_view_host")), "test_waterfall_view_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def write_plan(tmp_path, fft_size, lines):
    """the plan, and what the model shows for each of its views: (lines file, plan file, [(width, height, mode, picture)], refusals)"""
    rng = np.random.default_rng(fft_size + lines)
    half = fft_size // 2
    feeds = (3, lines - 4, lines - 2, 5)                    # first turn; ofs == lines; ...; across the wrap
    a = rng.uniform(-0.2, 1.2, (sum(feeds), fft_size)).astype(np.float32)
    a[:, rng.integers(0, fft_size, 3)] = 0.995
    m = PanelModel(fft_size, lines)
    m.step(); m.update()
    table = np_table()
    plan, want, refusals, at = [], [], 0, 0
    for k, n in enumerate(feeds):
        plan.append("feed %d" % n)
        for row in a[at:at + n]:
            m.set_points(row)
            m.step()
        m.update()
        at += n
        if k == 1:
            plan.append("grad " + " ".join(repr(float(c)) for row in STOPS5 for c in row))
            table = np_table(STOPS5)
        if k == 2:
            continue
        for W in (K.widths(half) if k == 3 else (17, 2 * half + 1)):
            for Hh in K.heights(lines):
                for _, mode in K.MODES:
                    plan.append("view %d %d %d" % (W, Hh, mode))
                    want.append((W, Hh, mode, K.np_view(m, table, W, Hh, mode)))
    for W, Hh, mode in ((1, 3, 0), (16385, 3, 1), (16, 0, 0), (16, 16385, 1), (16, 3, 2)):
        plan.append("refuse %d %d %d" % (W, Hh, mode))
        refusals += 1
    p_lines, p_plan = (os.path.join(str(tmp_path), n) for n in ("lines.bin", "plan.txt"))
    a.tofile(p_lines)
    with open(p_plan, "w") as f:
        f.write("\n".join(plan) + "\n")
    return p_lines, p_plan, want, refusals, m


@pytest.mark.parametrize("fft_size,lines", [(16, 7), (30, 12), (601, 7)])
def test_host_panel_views(exe, tmp_path, fft_size, lines):
    p_lines, p_plan, want, refusals, m = write_plan(tmp_path, fft_size, lines)
    prefix = os.path.join(str(tmp_path), "out")
    r = subprocess.run([exe, "cpu", p_lines, p_plan, prefix, str(fft_size), str(lines)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "waterfall view host test ok" in r.stdout
    st = next(ln for ln in r.stdout.splitlines() if ln.startswith("VIEWS ")).split()
    assert int(st[1]) == len(want) and int(st[3]) == refusals and int(st[5]) == m.ofs[0]
    for k, (W, Hh, mode, pic) in enumerate(want):
        got = np.fromfile("%s.%d.rgba" % (prefix, k), np.uint8).reshape(Hh, W, 4)
        assert np.array_equal(got, pic), (W, Hh, mode, np.argwhere(got != pic)[:8])


@pytest.mark.gpu
def test_device_panel_and_host_panel_hold_the_same_views(exe, tmp_path):
    fft_size, lines = 601, 12
    p_lines, p_plan, want, refusals, m = write_plan(tmp_path, fft_size, lines)
    r = subprocess.run([exe, "gpu", p_lines, p_plan, str(fft_size), str(lines)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "waterfall view host gpu ok" in r.stdout
    st = next(ln for ln in r.stdout.splitlines() if ln.startswith("VIEWS ")).split()
    assert int(st[1]) == len(want) and int(st[3]) == refusals and int(st[5]) == m.ofs[0] and int(st[7]) == 2
