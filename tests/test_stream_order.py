"""cubicsdr_amd/csrc/stream_order.hpp (ReadGate, SideStream, SlotOrder) on the CPU: tests/cpp/test_stream_order.cpp defines the HIP calls the header
makes as a happens-before model of streams and events, and checks the contracts against it -- one reader, two readers releasing in either order,
parities that do not see each other, a gate nobody passes, teardown with a mark pending, the side stream's three edges and its unwinding after a
create that failed at each step, the slot order of a call.  Built plain and once more with AddressSanitizer and UBSan: a stand-alone program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_stream_order.cpp")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_stream_order_contracts(tmp_path, sanitize):
    exe = os.path.join(str(tmp_path), "test_stream_order")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g"] if sanitize else []
    subprocess.run(["g++", "-O1", "-std=c++20", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-pthread", *flags,
                    "-I" + os.path.join(ROOT, "tests", "emu"), SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stream order ok" in r.stdout
