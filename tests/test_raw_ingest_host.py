"""The host mirror's native-format ingest (cubicsdr_amd/host/Adapters.h RawIQStreamSource, RawStreamReblocker, the raw DeviceIngest and the host
fall-back convertRawIQ), compiled with g++ against libcsdr_hip.so and exercised by tests/cpp/test_raw_ingest_host.cpp.  On the CPU: reads that do not
divide the block, 3-byte carries, an I/Q option change inside a block and a full output queue, the fall-back's `data` against the numpy conversion
this test writes to a file, bit for bit.  On the GPU: a raw CS16 source through SDRPostThread, with the waterfall bound to its output queue, gives the
audio, the waterfall lines and the waterfall frames of the same samples fed as CF32, in the channelized and in the single-channel branch."""
import os
import subprocess

import numpy as np
import pytest

from tests import raw_ingest_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_raw_ingest_host.cpp")
FORMAT_ID = {"CS16": 1, "CS8": 2, "CU8": 3, "CS12": 4}
BLOCK = 800                                             # BlockGeometry of 48 kS/s


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("raw_ingest_host")), "test_raw_ingest_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


@pytest.mark.parametrize("fmt,full_scale,offset,mtu", [("CS16", 32768.0, 0.0, 300), ("CS12", 2047.0, 0.0, 301), ("CU8", 128.0, 127.4, 333), ("CS8", 127.0, 0.0, 799)])
def test_raw_reblocker_and_host_fallback(exe, tmp_path, fmt, full_scale, offset, mtu):
    rng = np.random.default_rng(31)
    n = 7 * BLOCK + 2 * mtu
    raw = K.random_raw(fmt, n, rng)
    # the I/Q option is on from the read that holds sample 1200 (inside block 1) up to the read that holds sample 2900 (inside block 3)
    on, off = 1200 // mtu, 2900 // mtu
    want = K.np_convert(fmt, raw, full_scale, offset)
    lo, hi = on * mtu, off * mtu
    want[lo:hi] = (want[lo:hi].imag + 1j * want[lo:hi].real).astype(np.complex64)
    assert lo % BLOCK and hi % BLOCK and lo // BLOCK != hi // BLOCK
    p_raw, p_want = os.path.join(str(tmp_path), "raw.bin"), os.path.join(str(tmp_path), "want.bin")
    raw.tofile(p_raw)
    want.tofile(p_want)
    r = subprocess.run([exe, "cpu", p_raw, p_want, str(FORMAT_ID[fmt]), repr(full_scale), repr(offset), str(mtu), str(on), str(off)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "raw ingest host test ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("fs,block,demod_offset,channels", [(2400000, 40000, 250000, 4), (480000, 8000, 50000, 1)])
def test_raw_cs16_source_through_the_pipeline(exe, tmp_path, fs, block, demod_offset, channels):
    """audio, waterfall lines and waterfall frames of a raw CS16 source equal those of the CF32 feed; at 480 kS/s SDRPostThread runs its
    single-channel branch"""
    from tests.util import synth_iq
    center, nb = 100000000, 8
    x = synth_iq((nb + 2) * block + 16384, fs, center, [("NBFM", center + float(demod_offset))], seed=41)
    s = 30000.0 / float(np.max(np.abs(np.concatenate([x.real, x.imag]))))
    raw = K.pack("CS16", np.round(x.real * s).astype(np.int64), np.round(x.imag * s).astype(np.int64))
    p_raw, p_cf = os.path.join(str(tmp_path), "raw.bin"), os.path.join(str(tmp_path), "cf32.bin")
    raw.tofile(p_raw)
    K.np_convert("CS16", raw, 32768.0).tofile(p_cf)
    r = subprocess.run([exe, "gpu", p_raw, p_cf, str(nb), str(fs), str(demod_offset)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "raw ingest host gpu ok" in r.stdout
    blocks, samples = [int(v) for v in next(ln for ln in r.stdout.splitlines() if ln.startswith("AUDIO ")).split()[1::2]]
    assert blocks == nb and samples >= nb * 700                 # 1/60 s of 48 kHz audio per block
    wf = next(ln for ln in r.stdout.splitlines() if ln.startswith("WATERFALL ")).split()
    assert int(wf[1]) >= 20 and int(wf[3]) >= 20 and int(wf[6]) == channels
