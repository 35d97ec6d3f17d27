"""Static properties of the density bank's kernels (kernels_density.hpp: density_cover, density_fold, density_render), from the gfx950 code hipcc
emits (profiles/isa_stats.py; no GPU needed): exactly the three kernels DESIGN 27 names, no scratch in any."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("density_cover", "density_fold", "density_render")


def test_density_kernels_keep_out_of_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "isa_stats.py"), "csdr_density", "density_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    cols = next(ln for ln in lines if ln.startswith("kernel")).replace("|", " ").split()
    rows = [ln.replace("|", " ").split() for ln in lines if "density_" in ln and not ln.startswith("kernel")]
    assert len(rows) == len(KERNELS) and all(sum(k in row[0] for row in rows) == 1 for k in KERNELS), r.stdout
    for row in rows:
        v = dict(zip(cols[1:], (int(x) for x in row[1:])))
        assert v["scr"] == 0 and v["scratch"] == 0, (row[0], v)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert all(k in design for k in KERNELS)
