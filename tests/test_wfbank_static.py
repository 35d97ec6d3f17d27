"""Static properties of the waterfall bank's kernels (kernels_wfbank.hpp: wfb_quantize, wfb_update, wfb_view_linear, wfb_view_peak), from the
gfx950 code hipcc emits (profiles/isa_stats.py; no GPU needed): no scratch in any of the four, LDS and one barrier only in the two view kernels,
16-byte global loads and stores in wfb_quantize and wfb_update."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wfbank_kernels_stay_out_of_scratch_and_stream_in_16_byte_accesses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "isa_stats.py"), "csdr_wfbank", "wfb_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    head = next(ln for ln in lines if ln.startswith("kernel"))
    cols = head.replace("|", " ").split()
    stats = {}
    for name in ("wfb_quantize", "wfb_update", "wfb_view_linear", "wfb_view_peak"):
        rows = [ln.replace("|", " ").split() for ln in lines if name in ln]
        assert len(rows) == 1, r.stdout
        stats[name] = dict(zip(cols[1:], (int(x) for x in rows[0][1:])))
    for name, v in stats.items():
        assert v["scr"] == 0 and v["scratch"] == 0, (name, v)
        if name.startswith("wfb_view"):
            assert v["lds"] >= 1 and v["s_barrier"] == 1, (name, v)
        else:
            assert v["lds"] == 0 and v["s_barrier"] == 0, (name, v)
            assert v["st128"] >= 1 and v["ld128"] >= 1, (name, v)
