"""The host mirror's squelch bank (cubicsdr_amd/host/DemodSquelch.h: DemodSquelchBank), compiled with g++ -Wall against libcsdr_hip.so and exercised by
tests/cpp/test_squelch_host.cpp.  On the CPU: the header compiles and links, and without a context the constructor throws (the mirror has no host
arithmetic).  On the GPU: a DemodSquelchBank behind a small pipeline holds, slot by slot, the items, the meters and the recorder bytes
engine.SquelchBank holds for the same executes."""
import os
import subprocess

import numpy as np
import pytest

import cubicsdr_amd.hip as H
from tests.util import demod_frequencies, synth_iq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_squelch_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from cubicsdr_amd import build
    build.build(verbose=False)
    out = os.path.join(str(tmp_path_factory.mktemp("squelch_host")), "test_squelch_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", SRC, "-o", out, "-L" + os.path.join(ROOT, "cubicsdr_amd"), "-lcsdr_hip", "-ldl",
                    "-Wl,-rpath," + os.path.join(ROOT, "cubicsdr_amd")], check=True)
    return out


def test_header_links_and_needs_a_context(exe):
    r = subprocess.run([exe, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "squelch host test ok" in r.stdout


def read_records(path):
    from cubicsdr_amd.engine import SQUELCH_ITEM
    raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        e, slot, n_items, n_pcm = (int(v) for v in np.frombuffer(raw, np.int32, 4, at))
        at += 16
        items = np.frombuffer(raw, SQUELCH_ITEM, n_items, at).copy()
        at += 16 * n_items
        meters = np.frombuffer(raw, np.float32, 3, at).copy()
        brk = int(np.frombuffer(raw, np.int32, 1, at + 12)[0])
        at += 16
        pcm = np.frombuffer(raw, np.int16, n_pcm, at).copy()
        at += 2 * ((n_pcm + 1) & ~1)
        out.append(((e, slot), items, meters, brk, pcm))
    return out


@pytest.mark.gpu
def test_host_bank_holds_the_engine_banks_bytes(exe, tmp_path):
    from cubicsdr_amd.engine import Context, DemodBank, SDRPost, SquelchBank
    fs, M, block, center, nb, nexec = 2400000, 4, 40000, 100000000, 6, 4
    kinds = [("NBFM", 12500), ("AM", 6000), ("I/Q", 48000), ("FMS", 200000), ("USB", 5400)]
    setting = [(-6.0, 0, 0), (-17.0, 0, 1), (-6.0, 1, 2), (-12.0, 0, 0), (-10.0, 0, 1)]          # squelch level, muted, recorder option
    freqs = demod_frequencies(center, fs, len(kinds))
    x = synth_iq(nexec * nb * block, fs, center, [("NBFM", freqs[0]), ("AM", freqs[1]), ("NBFM", freqs[2]), ("FMS", freqs[3]), ("USB", freqs[4])], seed=91)
    x = x * np.repeat(np.where((np.arange(nexec * nb) // 6) % 2 == 0, 1.0, 0.05).astype(np.float32), block)
    p_iq, p_slots, p_out = (os.path.join(str(tmp_path), n) for n in ("iq.bin", "slots.txt", "out.bin"))
    x.astype(np.complex64).tofile(p_iq)
    with open(p_slots, "w") as f:
        for (k, bw), fr, (lv, mu, opt) in zip(kinds, freqs, setting):
            f.write("%d %d %d %.1f %d %d\n" % (H.MODEM_BY_NAME[k], bw, fr, lv, mu, opt))
    r = subprocess.run([exe, "gpu", p_iq, p_slots, p_out] + [str(v) for v in (fs, M, block, nb, nexec, center)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "squelch host gpu ok" in r.stdout
    got = read_records(p_out)
    ctx = Context(0)
    post, bank, sq = SDRPost(ctx, fs, M, block, nb), DemodBank(ctx, len(kinds), nb), SquelchBank(ctx, len(kinds), nb)
    want = []
    try:
        for i, ((k, bw), fr, (lv, mu, opt)) in enumerate(zip(kinds, freqs, setting)):
            bank.configure(i, post, k, bw, fr)
            sq.set_slot(i, True, lv, bool(mu), opt)
        for e in range(nexec):
            post.execute(x[e * nb * block:(e + 1) * nb * block], nb, block, center)
            bank.execute(post)
            sq.process_bank(bank)
            pcm, offs = sq.record()
            for s in range(len(kinds)):
                want.append(((e, s), sq.fetch(s), sq.state(s), pcm[offs[s]:offs[s + 1]]))
    finally:
        for o in (sq, bank, post, ctx):
            o.close()
    assert [g[0] for g in got] == [w[0] for w in want]
    assert len(got) == len(kinds) * nexec == int(next(ln for ln in r.stdout.splitlines() if ln.startswith("RECORDS ")).split()[1])
    n_pcm = 0
    for (k, items, meters, brk, pcm), (_, w_items, w_state, w_pcm) in zip(got, want):
        assert items.size == nb and items.tobytes() == w_items.tobytes(), k
        assert meters.tobytes() == np.array(w_state[:3], np.float32).tobytes() and bool(brk) == w_state[3], k
        assert pcm.tobytes() == w_pcm.tobytes(), k
        n_pcm += pcm.size
    assert n_pcm > 0 and any((items["flags"] & 1).any() for _, items, _, _, _ in got) and any(not (items["flags"] & 1).all() for _, items, _, _, _ in got)
