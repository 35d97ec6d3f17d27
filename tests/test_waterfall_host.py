"""The host mirror's waterfall (cubicsdr_amd/host/WaterfallPanel.h: WaterfallPanel and the pacing rule WaterfallFeed::processInputQueue), compiled with g++
against libcsdr_hip.so and exercised by tests/cpp/test_waterfall_host.cpp.  On the CPU: a host panel behind the pacing rule, driven by a plan of
elapsed times and queue entries this test writes to a file, against the numpy model of tests/waterfall_cases.py -- steps taken, lpsIndex, offsets,
both textures and the picture, bit for bit.  On the GPU: FFTVisualDataThread's distributor and processor pumped block by block; every frame is stepped
HBM to HBM with stepFrom() and, from the fetched SpectrumVisualData, into a second device panel and a host panel; all three must agree."""
import os
import subprocess

import numpy as np
import pytest

from tests import waterfall_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_waterfall_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("waterfall_host")), "test_waterfall_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def pace(state, elapsed, queue, lps, on_entry):
    """WaterfallCanvas::processInputQueue :92-119 restated; state = [lpsIndex]; returns whether a line was stepped"""
    target = 1.0 / float(lps)
    state[0] += elapsed
    updated = False
    if lps and state[0] >= target:
        while state[0] >= target:
            if not queue:
                break
            e = queue.pop(0)
            if e != -1:
                on_entry(e)
                updated = True
            state[0] -= target
    return updated


@pytest.mark.parametrize("fft_size,lines,lps", [(64, 7, 30), (601, 5, 7), (30, 12, 100)])
def test_host_panel_behind_the_pacing_rule(exe, tmp_path, fft_size, lines, lps):
    rng = np.random.default_rng(fft_size)
    n_frames = 40
    y = rng.uniform(-0.2, 1.2, (n_frames, fft_size)).astype(np.float32)
    y[3, :8] = [np.nan, np.inf, -np.inf, -0.0, 0.99, 1.0, np.float32(0.98999995), 2.0 ** -9][:min(8, fft_size)]
    frames = np.stack([np.broadcast_to((np.arange(fft_size) / fft_size).astype(np.float32), y.shape), y], axis=2).reshape(n_frames, 2 * fft_size)
    # turns: elapsed seconds, then what is pushed in front of the turn (frame index, -1 null entry, -2 frame of the wrong size)
    turns = [(0.001, [0]), (1.0 / lps, [1]), (2.5 / lps, [2, 3, -2, 4]), (0.0, [5]), (0.3 / lps, []), (10.0 / lps, [6, -1, 7, 8]), (1.0, list(range(9, 9 + lines + 3))),
             (0.01, [30]), (5.0 / lps, []), (3.0 / lps, [31, 32, -2, -1, 33, 34])]
    m = K.PanelModel(fft_size, lines)
    state, queue, stepped, updates = [0.0], [], [0], 0

    def on_entry(e):
        if e >= 0:
            m.set_points(frames[e])
        m.step()
        stepped[0] += 1
    stopped_at_due_lines = stopped_at_empty_queue = 0
    for elapsed, pushed in turns:
        queue += pushed
        if pace(state, elapsed, queue, lps, on_entry):
            m.update()
            updates += 1
        stopped_at_due_lines += bool(queue)
        stopped_at_empty_queue += not queue and state[0] >= 1.0 / lps
    p_frames, p_plan, prefix = (os.path.join(str(tmp_path), n) for n in ("frames.bin", "plan.txt", "out"))
    frames.astype(np.float32).tofile(p_frames)
    with open(p_plan, "w") as f:
        f.write(" ".join(repr(float(c)) for row in K.STOPS5 for c in row) + "\n")
        for elapsed, pushed in turns:
            f.write(" ".join([repr(float(elapsed))] + [str(e) for e in pushed]) + "\n")
    r = subprocess.run([exe, "cpu", p_frames, p_plan, prefix, str(fft_size), str(lines), str(lps)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "waterfall host test ok" in r.stdout
    st = next(ln for ln in r.stdout.splitlines() if ln.startswith("STATE ")).split()
    got = dict(zip(st[1::2], st[2::2]))
    assert int(got["turns"]) == len(turns) and int(got["updates"]) == updates and int(got["stepped"]) == stepped[0]
    assert float(got["lpsIndex"]) == state[0]
    assert [int(got["ofs0"]), int(got["ofs1"])] == m.ofs
    assert int(got["buffered"]) == 0 and int(got["queued"]) == len(queue)
    half = fft_size // 2
    for j in range(2):
        t = np.fromfile(prefix + ".tex%d" % j, np.uint8).reshape(lines, half)
        assert np.array_equal(t, m.tex[j]), (j, np.argwhere(t != m.tex[j])[:8])
    pic = np.fromfile(prefix + ".rgba", np.uint8).reshape(lines, 2 * half, 4)
    assert np.array_equal(pic, m.rgba(K.np_table(K.STOPS5), 0, lines))
    assert stepped[0] > lines and stopped_at_due_lines and stopped_at_empty_queue      # the ring went round; turns ended both ways


@pytest.mark.gpu
def test_step_from_behind_the_fft_visual_data_thread(exe, tmp_path):
    from tests.util import synth_iq
    fs, block, nb, fft_size, lines = 2400000, 40000, 24, 512, 31
    x = synth_iq(nb * block, fs, 100000000, [("NBFM", 100000000 + 250000.0), ("AM", 100000000 - 400000.0)], seed=77)
    p_iq = os.path.join(str(tmp_path), "iq.bin")
    x.astype(np.complex64).tofile(p_iq)
    r = subprocess.run([exe, "gpu", p_iq, str(nb), str(block), str(fs), str(fft_size), str(lines)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "waterfall host gpu ok" in r.stdout
    wf = next(ln for ln in r.stdout.splitlines() if ln.startswith("WATERFALL ")).split()
    assert int(wf[2]) > lines and int(wf[4]) >= 3
