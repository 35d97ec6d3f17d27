"""The host mirror's scope bank (cubicsdr_amd/host/DemodScopes.h: DemodScopeBank), compiled with g++ -Wall against libcsdr_hip.so and exercised by
tests/cpp/test_scopebank_host.cpp.  On the CPU: the header compiles and links, and without a context the constructor throws (the mirror has no host
arithmetic).  On the GPU: a DemodScopeBank behind a small pipeline holds, item by item, the bytes engine.ScopeBank holds for the same executes."""
import os
import subprocess

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests.util import demod_frequencies, synth_iq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_scopebank_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("scopebank_host")), "test_scopebank_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def test_header_links_and_needs_a_context(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scopebank host test ok" in r.stdout


def read_items(path):
    raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        head = np.frombuffer(raw, np.int32, 12, at)
        fc = np.frombuffer(raw, np.float64, 2, at + 48)
        n = int(head[4])
        pts = np.frombuffer(raw, np.float32, n, at + 64).copy()
        at += 64 + 4 * n
        out.append((tuple(int(v) for v in head[:4]),
                    dict(points=pts, mode=int(head[5]), spectrum=bool(head[6]), channels=int(head[7]), input_rate=int(head[8]), sample_rate=int(head[9]),
                         fft_size=int(head[10]), fft_floor=float(fc[0]), fft_ceil=float(fc[1]))))
    return out


@pytest.mark.gpu
def test_host_bank_holds_the_engine_banks_bytes(exe, tmp_path):
    from cubicsdr_amd.engine import Context, DemodBank, ScopeBank, SDRPost
    from tests.scopebank_cases import same_item
    fs, M, block, center, nb, nexec, L = 2400000, 4, 40000, 100000000, 2, 5, 1024
    kinds = [("NBFM", 12500), ("AM", 100000), ("I/Q", 48000), ("FMS", 200000), ("USB", 5400)]
    freqs = demod_frequencies(center, fs, len(kinds))
    x = synth_iq(nexec * nb * block, fs, center, [("NBFM", freqs[0]), ("AM", freqs[1]), ("NBFM", freqs[2]), ("FMS", freqs[3]), ("USB", freqs[4])], seed=91)
    p_iq, p_slots, p_out = (os.path.join(str(tmp_path), n) for n in ("iq.bin", "slots.txt", "out.bin"))
    x.astype(np.complex64).tofile(p_iq)
    with open(p_slots, "w") as f:
        for (k, bw), fr in zip(kinds, freqs):
            f.write("%d %d %d\n" % (H.MODEM_BY_NAME[k], bw, fr))
    r = subprocess.run([exe, "gpu", p_iq, p_slots, p_out] + [str(v) for v in (fs, M, block, nb, nexec, center, L)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scopebank host gpu ok" in r.stdout
    got = read_items(p_out)
    ctx = Context(0)
    post, bank, sb = SDRPost(ctx, fs, M, block, nb), DemodBank(ctx, len(kinds), nb), ScopeBank(ctx, L, len(kinds), 1, 4096)
    want = []
    try:
        for i, ((k, bw), fr) in enumerate(zip(kinds, freqs)):
            bank.configure(i, post, k, bw, fr)
        for e in range(nexec):
            post.execute(x[e * nb * block:(e + 1) * nb * block], nb, block, center)
            bank.execute(post)
            sb.set_enabled(e != 2, e != 3)
            sb.process_bank(bank)
            for s in range(len(kinds)):
                for j in range(sb.frames(s)):
                    for which in (0, 1):
                        it = sb.fetch(s, j, bool(which))
                        if it is not None:
                            want.append(((e, s, j, which), it))
    finally:
        for o in (sb, bank, post, ctx):
            o.close()
    assert [k for k, _ in got] == [k for k, _ in want]
    assert len(got) == len(kinds) * (2 * nexec - 2) == int(next(ln for ln in r.stdout.splitlines() if ln.startswith("ITEMS ")).split()[1])
    for (k, g), (_, w) in zip(got, want):
        assert same_item(g, w), k
