"""Static properties of the trace bank's kernels (kernels_tracebank.hpp: trace_lines, trace_xy), from the gfx950 code hipcc emits
(profiles/isa_stats.py; no GPU needed): exactly two kernels, no scratch in either."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tracebank_kernels_keep_out_of_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "isa_stats.py"), "csdr_tracebank", "trace_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    cols = next(ln for ln in lines if ln.startswith("kernel")).replace("|", " ").split()
    rows = [ln.replace("|", " ").split() for ln in lines if "trace_" in ln and not ln.startswith("kernel")]
    assert len(rows) == 2 and sum("trace_lines" in row[0] for row in rows) == 1 and sum("trace_xy" in row[0] for row in rows) == 1, r.stdout
    for row in rows:
        v = dict(zip(cols[1:], (int(x) for x in row[1:])))
        assert v["scr"] == 0 and v["scratch"] == 0, (row[0], v)
