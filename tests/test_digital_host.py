"""The host mirror's digital lab (cubicsdr_amd/host/ModemDigital.h and the digital branch of HipPipeline.h's finishDemod), compiled with g++
against libcsdr_hip.so and exercised by tests/cpp/test_digital_host.cpp: the registry and settings on the CPU; on the GPU an FSK instance's
console text and a QPSK instance's lock through SDRPostThread, against the same blocks through the bank's C ABI (tests/test_gpu_digital.py
holds those to the reference)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_digital_host.cpp")
FS, M, BLOCK, CENTER, NB = 2400000, 4, 40000, 100000000, 8
F_FSK, F_QPSK = CENTER + 620000, CENTER - 550000


def _build(tmp):
    from cubicsdr_amd import build
    build.build(verbose=False)
    exe = os.path.join(str(tmp), "test_digital_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", exe, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return exe


def test_digital_registry_and_settings(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "digital host test ok" in r.stdout


def blocks():
    """a QPSK demodulator's carrier (blocks 0 - 3 only, at its centre: one constellation point at unit amplitude behind the analyzer's gain of
    M) and FSK tones 2 kHz either side of the FSK demodulator's centre, switching every 500 samples, over faint noise"""
    rng = np.random.default_rng(17)
    n = np.arange(NB * BLOCK, dtype=np.float64)
    x = 0.005 * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
    q = 0.25 * np.exp(1j * (2 * np.pi * (F_QPSK - CENTER) * n / FS + np.pi / 4))
    q[4 * BLOCK:] = 0
    sym = rng.integers(0, 2, n.size // 500 + 1)
    fi = (F_FSK - CENTER) + np.where(sym[(n // 500).astype(int)] > 0, 2000.0, -2000.0)
    ph = 2 * np.pi * np.cumsum(fi) / FS
    return (x + q + 0.25 * np.exp(1j * ph)).astype(np.complex64)


@pytest.mark.gpu
def test_digital_instances_through_the_pipeline(tmp_path):
    from cubicsdr_amd.engine import Context, DemodBank, SDRPost
    exe = _build(tmp_path)
    x = blocks()
    path = os.path.join(str(tmp_path), "blocks.bin")
    x.tofile(path)
    r = subprocess.run([exe, "gpu", path, str(NB)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    lock = [int(ln.split()[2]) for ln in lines if ln.startswith("LOCK ")]
    fsk_lock = [int(ln.split()[2]) for ln in lines if ln.startswith("FSKLOCK ")]
    text = next(ln[5:] for ln in lines if ln.startswith("TEXT "))
    writes = int(next(ln.split()[1] for ln in lines if ln.startswith("WRITES ")))
    # the same blocks through the bank (the arithmetic the pipeline binds): hex of every FSK symbol, the QPSK lock after every block
    ctx = Context(0)
    post = SDRPost(ctx, FS, M, BLOCK, 1)
    bank = DemodBank(ctx, 2, 1)
    bank.configure_digital(0, post, "FSK", 19200, F_FSK)
    bank.configure_digital(1, post, "QPSK", 200000, F_QPSK)
    want_text, want_lock, want_writes = "", [], 0
    for b in range(NB):
        post.execute(x[b * BLOCK:(b + 1) * BLOCK], 1, BLOCK, CENTER)
        bank.execute(post)
        s = bank.symbols(0)
        want_text += "".join("%x" % int(v) for v in s)
        want_writes += s.size > 0
        want_lock.append(bank.digital_results(1)[0].lock)
    bank.close(); post.close(); ctx.close()
    print("QPSK lock per block", lock, "FSK symbols", len(text))
    assert len(text) == len(want_text) > NB * 100 and text == want_text
    assert writes == want_writes == NB                    # one write per block with text (digitalFinish)
    assert lock == want_lock
    assert lock[1:4] == [1, 1, 1] and lock[5:] == [0, 0, 0]   # a clean constellation point locks, noise does not
    assert fsk_lock == [0] * NB                               # ModemFSK never updates the lock
