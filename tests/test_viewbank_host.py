"""The host mirror's view bank (cubicsdr_amd/host/DemodViews.h: DemodViewBank), compiled with g++ against libcsdr_hip.so and exercised by
tests/cpp/test_viewbank_host.cpp.  Without a device: the bank needs a context, and without one every call is refused and logged.  On the GPU: a
device bank fed a plan of setView, setPeakHold, process and refused calls this test writes to a file; every frame and every slot's integers behind
every call against one RefSpectrum in view mode per slot (tests/viewbank_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import viewbank_cases as K
from tests.specbank_cases import check_frame
from tests.test_specbank_host import read_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_viewbank_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("viewbank_host")), "test_viewbank_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def test_host_bank_needs_a_context(exe):
    r = subprocess.run([exe, "nodev"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "viewbank host nodev ok" in r.stdout


def write_plan(tmp_path, F):
    """-> (iq file, plan file, the model's frames in the order the program writes them, the INFO lines it must print, refusals, max_frames)"""
    w, data, want = K.walks(F), K.make_inputs(F), K.model_main(F)
    plan, chunks, frames, infos, refusals = [], [], [], [], 0
    for ci, (k0, call) in enumerate(K.call_plan(w, data, K.CALLS)):
        k1 = max(i for _, i in call) + 1
        for s, v in w.items():
            if k0 in v["views"]:
                plan.append("view %d %d %d" % ((s,) + v["views"][k0]))
        if ci == 3:
            bad = "%d %d %d %d" % (K.A, 6 * F, K.FREQ, K.RATE)
            plan.append("refuse " + " ".join([bad] * (max(K.CALLS) + 1)))          # (a) makes a frame per input: max_frames + 1 of them
            plan.append("refuse %d 8 %d %d" % (K.NOVIEW, K.FREQ, K.RATE))           # a slot without a view
            plan.append("refuse %d 8 %d -1" % (K.A, K.FREQ))                        # a negative rate
            plan.append("badview %d %d 0" % (K.A, K.FREQ))
            refusals += 4
        items = []
        for s, k in call:
            items.append("%d %d %d %d" % (s, len(data[s][k]), K.FREQ, w[s]["rates"][k]))
            chunks.append(data[s][k])
        plan.append("call " + " ".join(items))
        for s in range(K.SLOTS + 1):
            fed = [want[s][i] for i in range(k0, k1) if want[s][i] is not None] if s in want else []
            frames += [(s, it["frame"]) for it in fed if it["frame"] is not None]
            if fed:
                i = fed[-1]["info"]
                infos.append((ci, "INFO %d %d %d %d %d %d %d" % (s, i["desired_input_size"], i["resample_bw"], i["shift_frequency"], i["last_data_size"], i["peak_reset"], i["num_written"])))
    p_iq, p_plan = (os.path.join(str(tmp_path), n) for n in ("iq.bin", "plan.txt"))
    np.concatenate(chunks).astype(np.complex64).tofile(p_iq)
    with open(p_plan, "w") as f:
        f.write("\n".join(plan) + "\n")
    return p_iq, p_plan, frames, infos, refusals, max(K.CALLS)


@pytest.mark.gpu
@pytest.mark.parametrize("F", (32, 256))
def test_device_bank_against_the_model(exe, tmp_path, F):
    p_iq, p_plan, want, infos, refusals, max_frames = write_plan(tmp_path, F)
    p_out = os.path.join(str(tmp_path), "out.bin")
    r = subprocess.run([exe, "gpu", p_iq, p_plan, p_out, str(F), str(K.SLOTS + 1), str(max_frames), str(K.max_samples(F))], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "viewbank host gpu ok" in r.stdout
    st = next(ln for ln in r.stdout.splitlines() if ln.startswith("FRAMES ")).split()
    assert int(st[1]) == len(want) and int(st[3]) == len(K.CALLS) and int(st[5]) == refusals
    got = read_frames(p_out, F)
    assert [s for s, _ in got] == [s for s, _ in want]
    for j, ((s, g), (_, w)) in enumerate(zip(got, want)):
        check_frame(g, w, (F, s, j))
    # the slots' integers behind every call: the program prints one line per slot and call, the fed slots' lines are the model's
    printed = [ln for ln in r.stdout.splitlines() if ln.startswith("INFO ")]
    assert len(printed) == len(K.CALLS) * (K.SLOTS + 1)
    for ci, line in infos:
        assert line in printed[ci * (K.SLOTS + 1):(ci + 1) * (K.SLOTS + 1)], (ci, line)
