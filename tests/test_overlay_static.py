"""Static properties of the overlay bank's kernel (kernels_overlay.hpp: overlay_compose), from the gfx950 code hipcc emits
(profiles/isa_stats.py; no GPU needed): exactly one kernel, no scratch."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_overlay_kernel_keeps_out_of_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "isa_stats.py"), "csdr_overlay", "overlay_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    cols = next(ln for ln in lines if ln.startswith("kernel")).replace("|", " ").split()
    rows = [ln.replace("|", " ").split() for ln in lines if "overlay_" in ln and not ln.startswith("kernel")]
    assert len(rows) == 1 and "overlay_compose" in rows[0][0], r.stdout
    v = dict(zip(cols[1:], (int(x) for x in rows[0][1:])))
    assert v["scr"] == 0 and v["scratch"] == 0, (rows[0][0], v)
