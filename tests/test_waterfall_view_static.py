"""Static properties of the viewport kernels (kernels_waterfall.hpp: wf_view_linear, wf_view_peak), from the gfx950 code hipcc emits
(profiles/isa_stats.py; no GPU needed): no scratch in either, 16-byte global loads and one barrier in wf_view_peak."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_kernels_keep_out_of_scratch_and_peak_streams_in_16_byte_loads():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "isa_stats.py"), "csdr_waterfall", "wf_view"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    head = next(ln for ln in lines if ln.startswith("kernel"))
    cols = head.replace("|", " ").split()
    stats = {}
    for name in ("wf_view_linear", "wf_view_peak"):
        rows = [ln.replace("|", " ").split() for ln in lines if name in ln]
        assert len(rows) == 1, r.stdout
        stats[name] = dict(zip(cols[1:], (int(x) for x in rows[0][1:])))
    for name, v in stats.items():
        assert v["scr"] == 0 and v["scratch"] == 0, (name, v)
    assert stats["wf_view_peak"]["ld128"] >= 1 and stats["wf_view_peak"]["s_barrier"] == 1, stats["wf_view_peak"]
