"""The host mirror's spectrum bank (cubicsdr_amd/host/DemodSpectra.h: DemodSpectrumBank), compiled with g++ against libcsdr_hip.so and exercised by
tests/cpp/test_specbank_host.cpp.  On the CPU: a host bank without a context, fed a plan of calls, setPeakHold, resetSlot and refused calls this test
writes to a file, every frame against one RefSpectrum per slot (tests/specbank_cases.py) within the project's TOL.  On the GPU: a device bank and a
host bank fed the same plan hold the same frames within that tolerance."""
import os
import subprocess

import numpy as np
import pytest

from tests import specbank_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_specbank_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("specbank_host")), "test_specbank_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def write_plan(tmp_path, F, peak):
    """-> (iq file, plan file, the model's frames in the order the program writes them, refusals, max_frames)"""
    calls = K.PEAK_CALLS if peak else K.CALLS
    n_items = sum(calls)
    data = K.make_inputs(F, n_items, nan=not peak)
    m = K.Model(F)
    plan, chunks, want, refusals, at = [], [], [], 0, 0
    max_frames = max(calls)
    for ci, per in enumerate(calls):
        if peak and at in (2, 5):
            plan.append("peak 1")
            m.set_peak_hold(True)
        if ci == 3:
            # slot 2 makes a frame per input: max_frames + 1 of them are refused as a whole, and so is a slot that does not exist
            plan.append("refuse " + " ".join("2 %d" % (2 * F) for _ in range(max_frames + 1)))
            plan.append("refuse %d 3" % K.SLOTS)
            refusals += 2
        items, per_slot = [], {s: [] for s in range(K.SLOTS)}
        for s in sorted(data):
            if data[s] is None:
                continue
            for k in range(at, at + per):
                items.append("%d %d" % (s, len(data[s][k])))
                chunks.append(data[s][k])
                w = m.feed(s, data[s][k])
                if w is not None:
                    per_slot[s].append(w)
        plan.append("call " + " ".join(items))
        for s in range(K.SLOTS):
            want += [(s, w) for w in per_slot[s]]
        at += per
    p_iq, p_plan = (os.path.join(str(tmp_path), n) for n in ("iq.bin", "plan.txt"))
    np.concatenate(chunks).astype(np.complex64).tofile(p_iq)
    with open(p_plan, "w") as f:
        f.write("\n".join(plan) + "\n")
    return p_iq, p_plan, want, refusals, max_frames


def read_frames(path, F):
    raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        slot, hold = np.frombuffer(raw, np.int32, 2, at)
        ce, fl = np.frombuffer(raw, np.float64, 2, at + 8)
        pts = np.frombuffer(raw, np.float32, 2 * F, at + 24).copy()
        at += 24 + 8 * F
        hp = None
        if hold:
            hp = np.frombuffer(raw, np.float32, 2 * F, at).copy()
            at += 8 * F
        out.append((int(slot), (pts, float(ce), float(fl), hp)))
    return out


@pytest.mark.parametrize("F,peak", [(16, False), (32, True), (256, False), (256, True), (2048, False)])
def test_host_bank_frames(exe, tmp_path, F, peak):
    p_iq, p_plan, want, refusals, max_frames = write_plan(tmp_path, F, peak)
    p_out = os.path.join(str(tmp_path), "out.bin")
    r = subprocess.run([exe, "cpu", p_iq, p_plan, p_out, str(F), str(K.SLOTS), str(max_frames)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "specbank host test ok" in r.stdout
    st = next(ln for ln in r.stdout.splitlines() if ln.startswith("FRAMES ")).split()
    assert int(st[1]) == len(want) and int(st[5]) == refusals
    got = read_frames(p_out, F)
    assert [s for s, _ in got] == [s for s, _ in want]
    for j, ((s, g), (_, w)) in enumerate(zip(got, want)):
        K.check_frame(g, w, (F, s, j))
    assert any(w[3] is not None for _, w in want) == peak


@pytest.mark.gpu
def test_device_bank_and_host_bank_hold_the_same_frames(exe, tmp_path):
    F = 256
    p_iq, p_plan, want, refusals, max_frames = write_plan(tmp_path, F, True)
    r = subprocess.run([exe, "gpu", p_iq, p_plan, str(F), str(K.SLOTS), str(max_frames)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "specbank host gpu ok" in r.stdout
    st = next(ln for ln in r.stdout.splitlines() if ln.startswith("FRAMES ")).split()
    assert int(st[1]) == len(want) and int(st[5]) == refusals and int(st[7]) == 2
