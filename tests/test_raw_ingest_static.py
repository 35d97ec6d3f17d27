"""Static properties of the format-conversion kernels (kernels_io.hpp ingest_convert), from the gfx950 code hipcc emits (profiles/isa_stats.py; no GPU
needed): one instance per integer format, no scratch, no LDS, no barrier, 16-byte loads and stores only beside the scalar tail."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conversion_kernels_use_no_scratch_and_no_lds():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "isa_stats.py"), "csdr_io", "ingest_convert"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    head = next(ln for ln in lines if ln.startswith("kernel"))
    cols = head.replace("|", " ").split()
    rows = [ln.replace("|", " ").split() for ln in lines if "ingest_convert" in ln]
    assert len(rows) == 4, r.stdout                                   # CS16, CS8, CU8, CS12
    for row in rows:
        v = dict(zip(cols[1:], (int(x) for x in row[1:])))
        assert v["scr"] == 0 and v["scratch"] == 0 and v["lds"] == 0 and v["s_barrier"] == 0, row
        assert v["vm_load"] >= 2 and v["vm_store"] >= 3, row           # the wide body and the scalar tail
