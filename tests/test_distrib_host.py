"""The host mirror's device route for the waterfall feed (cubicsdr_amd/host/HipPipeline.h: DeviceFFTDataDistributor, FFTVisualDataThread::setDeviceRoute,
SDRPostThread::setVisualReadback, SpectrumVisualProcessor::processLines), compiled with g++ against libcsdr_hip.so and exercised by
tests/cpp/test_distrib_host.cpp.  On the GPU: a raw CS16 source through SDRPostThread into FFTVisualDataThread, once by the default host route and once
with both switches on; the waterfall frames the thread distributes at its own cadence (30 lines/s), and the panel textures made of them, are identical
bit for bit, and with both switches on no channelized block comes back to the host; at ten lines per block the two routes make the same number of
frames from the same pacing state (tests/cpp/test_distrib_host.cpp says why the frames of that cadence are not compared).  On the CPU the program
is only compiled: the route needs a device."""
import os
import subprocess

import numpy as np
import pytest

from tests import raw_ingest_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_distrib_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("distrib_host")), "test_distrib_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def test_device_route_compiles_and_is_off_by_default(exe):
    """the mirror with the device route builds without warnings turned into errors, and the program refuses to run without its arguments"""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stdout
    src = open(os.path.join(ROOT, "cubicsdr_amd", "host", "HipPipeline.h")).read()
    assert "bool deviceRoute_ = false;" in src and "std::atomic_bool visualReadback_{true};" in src


@pytest.mark.gpu
@pytest.mark.parametrize("fs,block,demod_offset,channels", [(2400000, 40000, 250000, 4), (480000, 8000, 50000, 1)])
def test_device_route_equals_the_host_route(exe, tmp_path, fs, block, demod_offset, channels):
    """the frames FFTVisualDataThread distributes by the device route equal the default route's; at 480 kS/s SDRPostThread runs its single-channel
    branch, whose visual block is the DC-corrected one it read back: the device distributor stages it from the host"""
    from tests.util import synth_iq
    center, nb = 100000000, 48                             # a line every other block: 24 frames
    x = synth_iq((nb + 2) * block + 16384, fs, center, [("NBFM", center + float(demod_offset))], seed=43)
    s = 30000.0 / float(np.max(np.abs(np.concatenate([x.real, x.imag]))))
    raw = K.pack("CS16", np.round(x.real * s).astype(np.int64), np.round(x.imag * s).astype(np.int64))
    p_raw = os.path.join(str(tmp_path), "raw.bin")
    raw.tofile(p_raw)
    r = subprocess.run([exe, "gpu", p_raw, str(nb), str(fs), str(demod_offset)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "distrib host gpu ok" in r.stdout
    fr = next(ln for ln in r.stdout.splitlines() if ln.startswith("FRAMES ")).split()
    assert int(fr[1]) == int(fr[3]) >= 20 and int(fr[6]) == 0 and int(fr[8]) == channels
    assert int(fr[10]) == (nb if channels > 1 else 0)
    busy = next(ln for ln in r.stdout.splitlines() if ln.startswith("BUSY ")).split()
    assert int(busy[1]) == int(busy[3]) >= 50 and int(busy[6]) >= 7
