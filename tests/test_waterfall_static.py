"""Static properties of the waterfall kernels (kernels_waterfall.hpp: wf_quantize, wf_update, wf_rgba), from the gfx950 code hipcc emits
(profiles/isa_stats.py; no GPU needed): no scratch in any of the three, LDS and a barrier only in wf_rgba (its colour table), 16-byte global loads and
stores in each."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_waterfall_kernels_stream_in_16_byte_accesses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "isa_stats.py"), "csdr_waterfall", "wf_"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    head = next(ln for ln in lines if ln.startswith("kernel"))
    cols = head.replace("|", " ").split()
    stats = {}
    for name in ("wf_quantize", "wf_update", "wf_rgba"):
        rows = [ln.replace("|", " ").split() for ln in lines if name in ln]
        assert len(rows) == 1, r.stdout
        stats[name] = dict(zip(cols[1:], (int(x) for x in rows[0][1:])))
    for name, v in stats.items():
        assert v["scr"] == 0 and v["scratch"] == 0, (name, v)
        assert v["st128"] >= 1 and v["ld128"] >= 1, (name, v)
        if name == "wf_rgba":
            assert v["lds"] >= 5 and v["s_barrier"] == 1, (name, v)      # one table write, four look-ups
        else:
            assert v["lds"] == 0 and v["s_barrier"] == 0, (name, v)
    assert stats["wf_quantize"]["ld128"] == 12                           # four loads of the plain layout, eight of the pair layout
    assert stats["wf_update"]["ld128"] == stats["wf_update"]["vm_load"] == 1 and stats["wf_update"]["st128"] == stats["wf_update"]["vm_store"] == 1
