"""The host mirror's waterfall bank (cubicsdr_amd/host/DemodWaterfalls.h: DemodWaterfallBank), compiled with g++ against libcsdr_hip.so and
exercised by tests/cpp/test_wfbank_host.cpp.  On the CPU: a host bank without a context, fed a plan of steps, updates, a reset, gradients, renders and
refused calls this test writes to a file; lines taken, every slot's state and every picture against one PanelModel per slot and np_view
(tests/wfbank_cases.py), byte for byte.  On the GPU: a device bank and a host bank fed the same plan hold the same textures, offsets and atlas."""
import os
import subprocess

import numpy as np
import pytest

from tests import wfbank_cases as K
from tests.waterfall_cases import PanelModel, np_table, stops256

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_wfbank_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("wfbank_host")), "test_wfbank_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def write_plan(tmp_path, fft_size):
    """-> (floats file, plan file, the bytes the program must write, counts)"""
    models = [PanelModel(fft_size, K.LINES) for _ in range(K.SLOTS)]
    plan, floats, want = [], [], []
    counts = dict(steps=0, refused=0, states=0, pictures=0)
    table = np_table()

    def words(items):
        return " ".join("%d %d %d" % (s, 0 if a is None else a.shape[-1], n) for s, a, n in items)

    def state():
        plan.append("state")
        counts["states"] += 1
        for m in models:
            ofs = m.ofs if m.tex_init else [-1, -1]
            want.append(np.array([m.lines_buffered, ofs[0], ofs[1]], np.int32).tobytes())
            if m.tex_init:
                want.extend(m.tex[j].tobytes() for j in range(2))

    def render(mode, W, Hh, cols, slots):
        plan.append("render %d %d %d %d %s" % (mode, W, Hh, cols, " ".join(map(str, slots))))
        counts["pictures"] += 1
        want.append(K.np_atlas(models, table, slots, W, Hh, mode, cols).tobytes())
    half = fft_size // 2
    for k, turn in enumerate(K.plan(fft_size)):
        if k == 3:
            # 30 lines wait in slot 0: three more are refused as a whole, and so is a slot that does not exist; a reset of slot 1 with lines waiting
            fill = [(K.A, np.full((30, fft_size), 0.3, np.float32), 30), (K.B, np.full((2, fft_size), 0.6, np.float32), 2)]
            for items in (fill,):
                plan.append("step " + words(items))
                floats += [a.ravel() for _, a, _ in items]
                want.append(np.array([len(items)] + K.model_step(models, items), np.int32).tobytes())
                counts["steps"] += 1
            bad = np.full((3, fft_size), 0.9, np.float32)
            for items in ([(K.Cc, bad[:1], 1), (K.A, bad, 3)], [(K.B, bad[:1], 1), (K.SLOTS, bad[:1], 1)], [(K.A, None, 3)]):
                plan.append("refuse " + words(items))
                floats += [a.ravel() for _, a, _ in items if a is not None]
                counts["refused"] += 1
            plan.append("reset %d" % K.B)
            models[K.B] = PanelModel(fft_size, K.LINES)
            state()
            plan.append("update")
            for m in models:
                m.update()
            state()
            plan.append("gradient 256")
            floats.append(stops256().ravel())
            table = np_table(stops256())
        plan.append("step " + words(turn))
        floats += [a.ravel() for _, a, _ in turn if a is not None]
        want.append(np.array([len(turn)] + K.model_step(models, turn), np.int32).tobytes())
        counts["steps"] += 1
        plan.append("update")
        for m in models:
            m.update()
        state()
        if fft_size >= 4 and k >= 1:
            render(k % 2, (2, 3, half, 2 * half, 2 * half + 5)[k % 5], (1, K.LINES - 1, K.LINES, 2 * K.LINES + 1)[k % 4], (1, 2, 5)[k % 3], K.SLOT_LISTS[1])
            render(1 - k % 2, 7, 3, 2, K.SLOT_LISTS[2])
    if fft_size >= 4:
        for bad in ("0 7 3 0 1 2", "0 7 3 3 1 2", "1 1 3 1 1 2", "0 7 0 1 1 2", "2 7 3 1 1 2", "0 7 3 1 1 %d" % K.SLOTS):
            plan.append("badrender " + bad)
            counts["refused"] += 1
    else:
        plan.append("badrender 1 2 1 1 0")                  # one texel to a half: nothing to filter between
        counts["refused"] += 1
    p_f, p_plan = (os.path.join(str(tmp_path), n) for n in ("floats.bin", "plan.txt"))
    np.concatenate(floats).astype(np.float32).tofile(p_f)
    with open(p_plan, "w") as f:
        f.write("\n".join(plan) + "\n")
    return p_f, p_plan, b"".join(want), counts


def check_counts(stdout, counts, banks):
    st = next(ln for ln in stdout.splitlines() if ln.startswith("DONE ")).split()
    assert dict(zip(st[1::2], map(int, st[2::2]))) == dict(counts, banks=banks)


@pytest.mark.parametrize("fft_size", K.FFT_SIZES)
def test_host_bank_against_the_models(exe, tmp_path, fft_size):
    p_f, p_plan, want, counts = write_plan(tmp_path, fft_size)
    p_out = os.path.join(str(tmp_path), "out.bin")
    r = subprocess.run([exe, "cpu", p_f, p_plan, p_out, str(fft_size), str(K.LINES), str(K.SLOTS), str(K.MAX_PENDING)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wfbank host test ok" in r.stdout
    check_counts(r.stdout, counts, 1)
    got = open(p_out, "rb").read()
    assert len(got) == len(want) and got == want, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)


@pytest.mark.gpu
@pytest.mark.parametrize("fft_size", (30, 2048))
def test_device_bank_and_host_bank_hold_the_same_bytes(exe, tmp_path, fft_size):
    p_f, p_plan, want, counts = write_plan(tmp_path, fft_size)
    r = subprocess.run([exe, "gpu", p_f, p_plan, str(fft_size), str(K.LINES), str(K.SLOTS), str(K.MAX_PENDING)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wfbank host gpu ok" in r.stdout
    check_counts(r.stdout, counts, 2)
