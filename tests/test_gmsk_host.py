"""The host mirror's GMSK (cubicsdr_amd/host/ModemDigital.h ModemGMSK, Modem::registerDigitalGMSK, the GMSK branch of HipPipeline.h's
finishDigital), compiled with g++ against libcsdr_hip.so and exercised by tests/cpp/test_gmsk_host.cpp: on the CPU the opt-in registration beside
registerDigitalLab's unchanged 17 factories, the settings, rates and rebuild requests; on the GPU a GMSK instance through SDRPostThread, whose
console text and lock must be the bank's symbols and 0, a settings write included (tests/test_gpu_gmsk.py holds the bank to the reference)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_gmsk_host.cpp")
FS, M, BLOCK, CENTER, NB, SWITCH = 2400000, 4, 40000, 100000000, 40, 24
F_GMSK = CENTER + 430000


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("gmsk_host")), "test_gmsk_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


@pytest.mark.parametrize("mode", ["lab", "gmsk"])
def test_gmsk_host_registry_and_settings(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gmsk host test ok" in r.stdout


def blocks():
    """a 2-FSK-like carrier at F_GMSK (+-2.4 kHz, 4800 symbols per second) over faint noise"""
    rng = np.random.default_rng(23)
    n = np.arange(NB * BLOCK, dtype=np.float64)
    x = 0.005 * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
    sym = rng.integers(0, 2, n.size // 500 + 1)
    fi = (F_GMSK - CENTER) + np.where(sym[(n // 500).astype(int)] > 0, 2400.0, -2400.0)
    return (x + 0.25 * np.exp(2j * np.pi * np.cumsum(fi) / FS)).astype(np.complex64)


@pytest.mark.gpu
def test_gmsk_instance_through_the_pipeline(exe, tmp_path):
    from cubicsdr_amd.engine import Context, DemodBank, SDRPost
    x = blocks()
    path = os.path.join(str(tmp_path), "blocks.bin")
    x.tofile(path)
    r = subprocess.run([exe, "gpu", path, str(NB), str(SWITCH)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    lock = [int(ln.split()[2]) for ln in lines if ln.startswith("LOCK ")]
    textlen = [int(ln.split()[2]) for ln in lines if ln.startswith("TEXTLEN ")]
    text = next(ln[5:] for ln in lines if ln.startswith("TEXT "))
    writes = int(next(ln.split()[1] for ln in lines if ln.startswith("WRITES ")))
    # the same blocks through the bank: 0 / 1 per symbol, the settings write as a reconfiguration
    ctx = Context(0)
    post = SDRPost(ctx, FS, M, BLOCK, 1)
    bank = DemodBank(ctx, 1, 1)
    bank.configure_digital(0, post, "GMSK", 19200, F_GMSK)
    want_text, want_len, want_writes = "", [], 0
    for b in range(NB):
        if b == SWITCH:
            bank.configure_digital(0, post, "GMSK", 19200, F_GMSK, sps=8)
        post.execute(x[b * BLOCK:(b + 1) * BLOCK], 1, BLOCK, CENTER)
        bank.execute(post)
        s = bank.symbols(0)
        assert bank.digital_results(0)[0].lock == 0
        want_text += "".join("%x" % int(v) for v in s)
        want_len.append(len(want_text))
        want_writes += s.size > 0
    bank.close(); post.close(); ctx.close()
    assert set(text) == {"0", "1"} and len(text) > NB * 40
    assert text == want_text and textlen == want_len
    assert writes == want_writes                          # one write per block with text (digitalFinish)
    assert lock == [0] * NB                               # ModemGMSK never updates the lock
