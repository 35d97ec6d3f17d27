"""The host mirror's table-driven modems (ModemAPSK / ModemSQAM / ModemST of cubicsdr_amd/host/ModemDigital.h and Modem::registerDigitalTables),
compiled with g++ against libcsdr_hip.so and exercised by tests/cpp/test_table_host.cpp: the registry and settings on the CPU with a
formula-built ConstellationSource; on the GPU an APSK and an ST instance through SDRPostThread, their tables from a file this test writes from the
oracle's modulator, against the same blocks through the bank's C ABI (tests/test_gpu_table.py holds that to the reference)."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_table_host.cpp")
FS, M, BLOCK, CENTER, NB = 2400000, 4, 40000, 100000000, 6
F_APSK, F_ST = CENTER + 620000, CENTER - 550000


def _build(tmp):
    from cubicsdr_amd import build
    build.build(verbose=False)
    exe = os.path.join(str(tmp), "test_table_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", exe, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return exe


def test_table_registry_and_settings(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "table host test ok" in r.stdout


def blocks():
    """faint noise -- in the APSK demodulator's channel nothing else, so that APSK4, whose first ring is a point at the centre, locks and APSK16,
    which has none, does not -- and a wandering tone in the ST demodulator's channel"""
    rng = np.random.default_rng(23)
    n = np.arange(NB * BLOCK, dtype=np.float64)
    x = 1e-4 * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
    ph = 2 * np.pi * np.cumsum((F_ST - CENTER) + 3000.0 * np.sin(2 * np.pi * n / 70000)) / FS
    return (x + 0.2 * (1 + 0.5 * np.sin(2 * np.pi * n / 9000)) * np.exp(1j * ph)).astype(np.complex64)


@pytest.mark.gpu
def test_table_instances_through_the_pipeline(tmp_path):
    from cubicsdr_amd.engine import Context, DemodBank, SDRPost
    from tests import table_oracle as T
    if not T.available():
        pytest.skip("the oracle (oracle/_ref) did not travel")
    libs = T.Libs(tmp_path)
    exe = _build(tmp_path)
    names = {"APSK": ["APSK4", "APSK8", "APSK16", "APSK32", "APSK64", "APSK128", "APSK256"], "ST": ["V29"]}
    pts = {n: T.constellation(libs, n) for v in names.values() for n in v}
    tpath = os.path.join(str(tmp_path), "tables.bin")
    with open(tpath, "wb") as f:
        for modem, v in names.items():
            for n in v:
                f.write(struct.pack("<i", len(modem)) + modem.encode() + struct.pack("<i", pts[n].size) + pts[n].astype(np.complex64).tobytes())
    x = blocks()
    path = os.path.join(str(tmp_path), "blocks.bin")
    x.tofile(path)
    r = subprocess.run([exe, "gpu", path, str(NB), tpath], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    slots = [int(v) for v in next(ln for ln in lines if ln.startswith("SLOTS ")).split()[1:]]
    lock = [[int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("LOCK ")]
    sym = {(int(ln.split()[1]), int(ln.split()[2])): np.array(ln.split()[3:], np.uint32) for ln in lines if ln.startswith("SYM ")}
    # the same blocks through the bank (the arithmetic the pipeline binds), the "cons" write before block 3 included
    ctx = Context(0)
    post = SDRPost(ctx, FS, M, BLOCK, 1)
    bank = DemodBank(ctx, 2, 1)
    bank.configure_table(0, post, [T.product_table(n, pts[n]) for n in names["APSK"]], 200000, F_APSK)
    bank.configure_table(1, post, T.product_table("V29", pts["V29"]), 200000, F_ST)
    want_lock = []
    for b in range(NB):
        if b == 3:
            bank.set_digital_cons(0, 16)
        post.execute(x[b * BLOCK:(b + 1) * BLOCK], 1, BLOCK, CENTER)
        bank.execute(post)
        res = [bank.digital_results(i)[0] for i in range(2)]
        want_lock.append([r.lock for r in res])
        assert res[0].cons == (16 if b >= 3 else 4) and res[1].cons == 16
        for i in range(2):
            got = sym[(b, slots[i])]
            assert got.size == res[i].n_symbols > 1000 and np.array_equal(got, bank.symbols(i)), (b, i)
    bank.close(); post.close(); ctx.close()
    print("APSK / ST lock per block", lock)
    assert lock == want_lock
    # |x| far below 0.005 sits on APSK4's centre point and locks; after the write to 16 the nearest point is a ring away; V.29 has no centre point
    assert [l[0] for l in lock] == [1, 1, 1, 0, 0, 0] and [l[1] for l in lock] == [0] * NB
