"""The host mirror's trace bank (cubicsdr_amd/host/DemodTraces.h: DemodTraceBank), compiled with g++ against libcsdr_hip.so and exercised by
tests/cpp/test_tracebank_host.cpp.  On the CPU: a host bank without a context renders the shared cases (tests/tracebank_cases.py) from a plan this
test writes to a file; every picture against tests/trace_oracle.py, byte for byte, and refused renders.  On the GPU: a device bank and a host bank
fed the same plan give the same pictures."""
import os
import subprocess

import numpy as np
import pytest

from tests import trace_oracle as O
from tests import tracebank_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_tracebank_host.cpp")
PLAN_CASES = [n for n in K.CASES if n != "past_2_31"]          # (the bank of the program holds 2^16 points per item)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("tracebank_host")), "test_tracebank_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def write_plan(tmp_path):
    """-> (floats file, plan file, the bytes the program must write, counts)"""
    plan, floats, want = [], [np.zeros(1, np.float32)], []
    counts = dict(pictures=0, refused=0)

    def words(items):
        w = []
        for it in items:
            if it is None or it["points"] is None:
                w.append("0 0 0 0")
                continue
            kind, layout = O.KINDS[it["kind"]], it.get("layout", 0)
            p = np.asarray(it["points"], np.float32).ravel()
            n = p.size if kind == O.SCOPE_XY else p.size // (1 + layout)
            floats.append(p[:n if kind == O.SCOPE_XY else n * (1 + layout)])
            if it.get("hold") is not None:
                floats.append(np.asarray(it["hold"], np.float32).ravel())
            w.append("%d %d %d %d" % (kind, n, layout, it.get("hold") is not None))
        return " ".join(w)
    plan.append("render 2 1 1 0 1 0 0")                    # (the one float in front of the cases)
    want.append(O.atlas([dict(kind="spectrum", points=floats[0])], 2, 1).tobytes())
    counts["pictures"] += 1
    for name in PLAN_CASES:
        case = K.CASES[name]
        col = dict(O.DEFAULT_COLORS, **case.get("colors", {}))
        plan.append("colors " + " ".join(str(v) for key in ("bg", "line", "hold", "axis_major", "axis_minor") for v in col[key]))
        plan.append("render %d %d %d %s" % (case["W"], case["H"], case.get("cols", 1), words(case["items"])))
        want.append(K.expected(case).tobytes())
        counts["pictures"] += 1
    for bad in ("1 8 1 0 0 0 0", "8 0 1 0 0 0 0", "8 8 0 0 0 0 0", "8 8 2 0 0 0 0", "8 8 1 4 0 0 0", "8 8 1 0 0 2 0", "8 8 1 0 -1 0 0", "8 1 1 2 0 0 0",
                "8 8 1" + " 0 0 0 0" * 17):                        # (17 items into a bank set up for 16)
        plan.append("badrender " + bad)
        counts["refused"] += 1
    p_f, p_plan = (os.path.join(str(tmp_path), n) for n in ("floats.bin", "plan.txt"))
    np.concatenate(floats).astype(np.float32).tofile(p_f)
    with open(p_plan, "w") as f:
        f.write("\n".join(plan) + "\n")
    return p_f, p_plan, b"".join(want), counts


def check_counts(stdout, counts, banks):
    st = next(ln for ln in stdout.splitlines() if ln.startswith("DONE ")).split()
    assert dict(zip(st[1::2], map(int, st[2::2]))) == dict(counts, banks=banks)


def test_host_bank_against_the_oracle(exe, tmp_path):
    p_f, p_plan, want, counts = write_plan(tmp_path)
    p_out = os.path.join(str(tmp_path), "out.bin")
    r = subprocess.run([exe, "cpu", p_f, p_plan, p_out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tracebank host test ok" in r.stdout
    check_counts(r.stdout, counts, 1)
    got = open(p_out, "rb").read()
    assert len(got) == len(want) and got == want, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)


@pytest.mark.gpu
def test_device_bank_and_host_bank_give_the_same_pictures(exe, tmp_path):
    p_f, p_plan, want, counts = write_plan(tmp_path)
    r = subprocess.run([exe, "gpu", p_f, p_plan], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tracebank host gpu ok" in r.stdout
    check_counts(r.stdout, counts, 2)
