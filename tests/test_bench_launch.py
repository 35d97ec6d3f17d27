"""bench.py's own launcher and its reporting helpers.  `python bench.py --gpus N` (the driver's command shape) must produce the N-rank line
unaided: it re-runs itself under torch.distributed.run, one rank per GPU; rank 0 prints ONE JSON line with n_gpus = N, the replica (weak)
value of the default configuration and a `strong` object (ONE C4 stream over all ranks, time slabs + all-to-all).  On a one-GPU box the same
control flow runs as a dry run: both ranks on the one device, collectives over gloo (staged through the host)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spread_and_sensors_without_a_gpu():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.spread([3.0, 1.0, 2.0]) == {"n": 3, "min": 1.0, "median": 2.0, "max": 3.0}
    assert bench.spread([]) == {}
    s = bench.Sensors(0)               # no HIP device here: no files, start / stop are no-ops
    s.start()
    assert s.stop().get("samples", 0) == 0 or s.files


def test_only_the_json_line_reaches_stdout():
    """libraries under bench.py write to file descriptor 1 (RCCL's version banner, gloo's connection notes): after claim_stdout() such writes land
    on stderr and the stream it returns is the only way to the caller's stdout"""
    code = ("import os, sys; sys.path.insert(0, %r); import bench\n"
            "out = bench.claim_stdout()\n"
            "os.write(1, b'banner from a library\\n'); print('a stray print')\n"
            "out.write('{\"ok\": 1}\\n'); out.flush()\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == '{"ok": 1}\n', r.stdout
    assert "banner from a library" in r.stderr and "a stray print" in r.stderr


def test_dump_outputs_without_a_gpu(tmp_path):
    """--dump-outputs at the default configuration's sizes (256 demodulators, 128 blocks, ~1000 frames of a 65536-point spectrum), on stand-ins
    for the bank and the spectrum: float32 / float64 files within the 64 MB budget, every demodulator's counts and tails, the whole batch of a
    fixed sample of demodulators, a fixed sample of frames with the last among them -- the same files on a second call"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench

    class Block:
        def __init__(self, n_iq, n_audio):
            self.n_iq, self.n_audio = n_iq, n_audio

    class Bank:
        def results(self, i):
            return [Block(200 + i % 3, 800)] * 128

        def iq(self, i):
            return (np.arange(128 * (200 + i % 3), dtype=np.float32) * (1 - 0.5j) + i).astype(np.complex64)

        def audio(self, i):
            return np.arange(128 * 800, dtype=np.float32) + i

    class Spec:
        fft_size = 65536

        def fetch(self, f):
            return np.full(2 * self.fft_size, f, np.float32), 1e8 + f, -90.0 - f

    n = bench.dump_outputs(str(tmp_path / "a"), Bank(), 256, Spec(), 1000)
    assert n == bench.dump_outputs(str(tmp_path / "b"), Bank(), 256, Spec(), 1000)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    d = {f[:-4]: np.load(tmp_path / "a" / f) for f in names}
    assert all(f.endswith(".npy") for f in names) and all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert n == sum(a.nbytes for a in d.values()) <= 64 << 20
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 << 20
    for f in names:
        assert np.array_equal(d[f[:-4]], np.load(tmp_path / "b" / f))
    assert d["demod_counts"].shape == (256, 128, 2) and d["demod_counts"][5, 7].tolist() == [202, 800]
    assert d["iq_tail"].shape == (256, 256, 2) and d["audio_tail"].shape == (256, 1024)
    assert d["audio_tail"][3, -1] == 128 * 800 - 1 + 3
    picked = [int(i) for i in d["demods_sampled"]]
    assert len(picked) == 16 and picked == sorted(set(picked))
    for i in picked:
        assert np.array_equal(d["audio_d%d" % i], Bank().audio(i))
        assert np.array_equal(d["iq_d%d" % i], Bank().iq(i).view(np.float32).reshape(-1, 2))
    idx = d["spectrum_frame_index"].astype(int).tolist()
    assert len(idx) == 16 and idx[-1] == 999 and idx == sorted(set(idx))
    assert d["spectrum_frames"].shape == (16, 2 * 65536) and d["spectrum_frames"][:, 0].tolist() == idx
    assert d["spectrum_center_floor"][:, 0].tolist() == [1e8 + f for f in idx]


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_its_outputs(tmp_path):
    """a plain run (no --full) prints the headline line only: `steps` timed steps, `ms_per_step` = the timed region / steps; --dump-outputs
    writes the last step's outputs, consistent with the bank's own counts"""
    import numpy as np
    dump = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--blocks", "8", "--batches", "2",
           "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["value"] > 0
    assert abs(out["ms_per_step"] * 3 - 1e3 * out["config"]["timed_region_s"]) <= 1e-6 * out["ms_per_step"]
    assert not {"roofline", "cpu_baseline", "strong"} & set(out)
    assert not {"step_ms", "clocks", "library_default_streams", "small_batches", "host_fed"} & set(out["config"])
    d = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    assert sum(a.nbytes for a in d.values()) == out["config"]["dump_outputs"]["bytes"] <= 64 << 20
    counts = d["demod_counts"]
    assert counts.shape == (256, 8, 2) and (counts >= 0).all() and (counts[:, :, 1].sum(axis=1) > 0).all()
    for i in d["demods_sampled"].astype(int):
        assert d["iq_d%d" % i].shape == (counts[i, :, 0].sum(), 2) and d["audio_d%d" % i].shape == (counts[i, :, 1].sum(),)
    assert d["spectrum_frames"].shape[1] == 2 * 65536 and np.isfinite(d["spectrum_frames"]).all()


@pytest.mark.gpu
def test_bench_gpus_2_launches_its_own_ranks_dry_run():
    import torch
    env = dict(os.environ)
    if torch.cuda.device_count() < 2:
        env["CSDR_DIST_BACKEND"] = "gloo"      # two ranks on the one GPU: RCCL refuses that, gloo carries the collectives
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--blocks", "8", "--batches", "2",
           "--full", "--cpu-seconds", "0", "--no-latency", "--ring", "noise"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert out["config"]["step_ms"]["n"] == 1
    st = out["strong"]
    assert st.get("value"), st
    assert st["scaling"] == "strong" and st["n_gpus"] == 2
    if torch.cuda.device_count() >= 2:
        assert st["rccl_ranks"] == 2
