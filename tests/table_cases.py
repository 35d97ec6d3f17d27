"""Parity cases of the table-driven decision kernel (csdr_table_run) against the reference binary's APSK / SQAM / V.29 / arb objects, shared by
tests/test_table_emu.py (the host-thread emulation of the HIP sources) and tests/test_gpu_table.py (the device).  Recipe and bounds are those of
tests/digital_cases.py::check_constellation."""
import numpy as np

from cubicsdr_amd.engine import table_run
from tests import table_oracle as T
from tests.digital_cases import BOUNDARY_SHARE, N_SAMPLES, evm_close, uniform_plane
from tests.digital_oracle import min_distance

NEAREST_MUST_FAIL = "APSK64"          # the case that also shows nearest-point is not the APSK rule


def noisy_points(pts, n, seed):
    """random symbols of the reference's own constellation plus complex noise of 0.1 x half the minimum distance"""
    rng = np.random.default_rng(seed)
    sig = 0.1 * min_distance(pts) / 2
    sym = rng.integers(0, pts.size, n).astype(np.uint32)
    noise = sig * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    return (pts[sym] + noise).astype(np.complex64)


def check_table(ctx, libs, name, seed=7):
    """noisy points in two halves, the second continued from the returned state: every decision and the last-sample EVM; an empty run repeats
    the EVM; uniform points: mismatches only on the reference's own decision boundaries, at most 0.1 %.  Prints every figure before it asserts."""
    pts = T.constellation(libs, name)
    tab = T.product_table(name, pts)
    x = noisy_points(pts, N_SAMPLES, seed)
    half = N_SAMPLES // 2
    ref = T.Modem(libs, name)
    want1 = ref.demodulate(x[:half])
    e1 = ref.evm()
    want2 = ref.demodulate(x[half:])
    e2 = ref.evm()
    ref.close()
    got1, g1, st = table_run(ctx, tab, x[:half])
    got2, g2, st = table_run(ctx, tab, x[half:], state=st)
    got0, g0, st = table_run(ctx, tab, np.zeros(0, np.complex64), state=st)
    u = uniform_plane(N_SAMPLES, seed + 1)
    ref = T.Modem(libs, name)
    want = ref.demodulate(u)
    ref.close()
    got, _, _ = table_run(ctx, tab, u)
    bad = np.nonzero(got != want)[0]
    edge = T.boundary_mask(libs, name, u, want) if bad.size else np.zeros(u.size, bool)
    print("table %-9s noisy mismatches %d + %d, evm %.9g / %.9g (ref %.9g / %.9g), empty %.9g; plane mismatches %d of %d, off the boundaries %d"
          % (name, int((got1 != want1).sum()), int((got2 != want2).sum()), g1, g2, e1, e2, g0, bad.size, u.size, int((~edge[bad]).sum())))
    # samples far below the points' scale, in every quadrant and on the axes (a front end's first outputs after a reset are such): x - p rounds
    # to -p, and what decides is the object's own order of tests
    rng = np.random.default_rng(seed + 2)
    tiny = ((rng.standard_normal(256) + 1j * rng.standard_normal(256)) * 10.0 ** rng.uniform(-30, -8, 256)).astype(np.complex64)
    tiny[:8] = np.array([0, 1e-20, -1e-20, 1e-20j, -1e-20j, complex(-0.0, 0.0), complex(0.0, -0.0), complex(-0.0, -0.0)], np.complex64)
    ref = T.Modem(libs, name)
    want_t = ref.demodulate(tiny)
    ref.close()
    got_t, _, _ = table_run(ctx, tab, tiny)
    print("table %-9s tiny samples: %d of %d differ" % (name, int((got_t != want_t).sum()), tiny.size))
    assert np.array_equal(got1, want1), (name, np.nonzero(got1 != want1)[0][:8])
    assert np.array_equal(got_t, want_t), (name, tiny[got_t != want_t][:4], got_t[got_t != want_t][:4], want_t[got_t != want_t][:4])
    assert np.array_equal(got2, want2), (name, np.nonzero(got2 != want2)[0][:8])
    assert evm_close(g1, e1) and evm_close(g2, e2), (name, g1, e1, g2, e2)
    assert got0.size == 0 and evm_close(g0, e2)
    assert edge[bad].all(), (name, bad[~edge[bad]][:8], u[bad[~edge[bad]][:4]])
    assert bad.size <= BOUNDARY_SHARE * u.size, (name, bad.size)
    if name == NEAREST_MUST_FAIL:       # the wrong rule would not have passed: nearest-point leaves the binary's decisions off its boundaries
        wrong = np.nonzero(T.nearest_restated(pts, u) != want)[0]
        off = wrong[~T.boundary_mask(libs, name, u, want)[wrong]]
        print("table %-9s nearest-point restatement differs from the binary on %d samples, %d of them off the boundaries" % (name, wrong.size, off.size))
        assert off.size > BOUNDARY_SHARE * u.size, (name, wrong.size, off.size)
    return bad.size


def check_refusals(ctx, libs):
    """csdr_table_run / csdr_bank_configure_table_slot refuse tables that are not well formed (CSDR_EINVAL)"""
    import ctypes as C
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import DemodBank, SDRPost, nearest_table
    l = H.lib()
    pts = T.constellation(libs, "APSK16")
    good = T.product_table("APSK16", pts)
    x = np.zeros(8, np.complex64)
    out = np.zeros(8, np.uint32)
    n = C.c_int()

    def run(tab):
        return l.csdr_table_run(ctx.h, C.byref(tab), x.ctypes.data, x.size, H.DigitalState(), out.ctypes.data, out.size, n, None)
    assert run(good) == 0
    for edit in ("rule", "n_points", "n_rings", "ring_size", "ring_map", "slicer", "nan"):
        t = H.Constellation.from_buffer_copy(good)
        if edit == "rule": t.rule = 2
        elif edit == "n_points": t.n_points = 12
        elif edit == "n_rings": t.n_rings = 9
        elif edit == "ring_size": t.ring_size[0] += 1
        elif edit == "ring_map": t.ring_map[0] = t.ring_map[1]
        elif edit == "slicer": t.ring_slicer[0] = 0.0
        else: t.points[3] = float("nan")
        assert run(t) == -1, edit
    post = SDRPost(ctx, 2400000, 4, 40000, 1)
    bank = DemodBank(ctx, 2, 1)
    try:
        p = H.DemodParams(H.CSDR_MODEM_DIGITAL, 200000, 48000, 0, 100000000)
        two = (H.Constellation * 2)(good, good)
        assert l.csdr_bank_configure_table_slot(bank.h, 0, p, two, 2, post.h) == -1          # the same size twice
        assert l.csdr_bank_configure_table_slot(bank.h, 0, p, two, 0, post.h) == -1
        q = H.DemodParams(H.CSDR_MODEM_NBFM, 12500, 48000, 0, 100000000)
        assert l.csdr_bank_configure_table_slot(bank.h, 0, q, two, 1, post.h) == -1
        d = H.DigitalParams(H.CSDR_DIGITAL_TABLE, 16, 0, 0, 0.0)
        assert l.csdr_bank_configure_digital_slot(bank.h, 0, p, d, post.h) == -1             # a table slot needs its own call
        bank.configure_table(1, post, [good, nearest_table(T.constellation(libs, "V29")[:8])], 200000, 100000000)
        assert l.csdr_bank_set_digital_cons(bank.h, 1, 8) == 0 and l.csdr_bank_set_digital_cons(bank.h, 1, 16) == 0
        assert l.csdr_bank_set_digital_cons(bank.h, 1, 64) == -6
    finally:
        bank.close()
        post.close()


FS, M, BLOCK, CENTER = 2400000, 4, 40000, 100000000
CHAIN = [(["APSK16", "APSK64"], 200000), (["SQAM32", "SQAM128"], 200000), (["V29"], 200000), (["ARB64VT"], 150000), (["USER64"], 200000),
         (["APSK256", "APSK8"], 100000), (["ARB256OPT"], 200000)]


def run_chain(ctx, libs, specs, executes, switches=None, skip=None, reject=()):
    """specs: [(scheme names, rate)] one table slot each, holding one table per name, the first active; executes: blocks per execute.  Every
    block goes through the reference front end (RefDemod.pre) and the reference binary's objects (RefTable); a second set of reference objects is
    fed the bank's own resampled IQ, to tell the front end's last-place differences from the kernel's.  switches: {execute: [(slot, cons)]} a
    "cons" write before that execute.  skip: {execute: [slot]} slots tuned out of the band for that execute (the reference then never calls
    demodulate: the block results must repeat the deciding object's own EVM).  reject: executes before which a batch is refused because a slot
    behind the table slots was built for another channel rate (the table slots must carry on as if it never came)."""
    import pytest
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import DemodBank, SDRPost
    from oracle.cubicsdr_chain import RefDemod, RefSDRPost
    from tests.util import demod_frequencies, synth_iq
    nbmax = max(executes)
    post = SDRPost(ctx, FS, M, BLOCK, nbmax)
    bank = DemodBank(ctx, len(specs) + 1, nbmax)
    rp = RefSDRPost("ref", FS, M)
    freqs = demod_frequencies(CENTER, FS, len(specs))
    rds, rms, rgs = [], [], []
    by_cons = []
    for i, (names, rate) in enumerate(specs):
        bank.configure_table(i, post, [T.product_table(n, T.constellation(libs, n)) for n in names], rate, freqs[i])
        rds.append(RefDemod("ref", "NBFM", rate, freqs[i], rp.chan_bw))          # the front end of any slot: NCO + msresamp_crcf to the modem rate
        rms.append(T.RefTable(libs, names))
        rgs.append(T.RefTable(libs, names))
        by_cons.append({T.n_points(n): n for n in names})
    # a frequency the channelizer still routes (within a channel's width of the outermost centre) and DemodulatorPreThread drops (more than
    # 0.75 of the channel rate off it)
    f_out = CENTER + FS // 2 + int(0.9 * rp.chan_bw)          # (the outermost centre is the wrap channel's, CENTER + FS / 2)
    flips = total = kernel_edges = skipped_blocks = 0
    t0 = 0
    for e, nb in enumerate(executes):
        for slot, cons in (switches or {}).get(e, []):
            bank.set_digital_cons(slot, cons)
            rms[slot].set_cons(cons)
            rgs[slot].set_cons(cons)
        if e in reject:
            other = SDRPost(ctx, 2 * FS, M, BLOCK, nbmax)
            bank.configure(len(specs), other, "NBFM", 12500, freqs[0])
            xr = [synth_iq(BLOCK, FS, CENTER, [("NBFM", f + 3000) for f in freqs], seed=5000 + 7 * e + b, t0=t0 + b * BLOCK) for b in range(nb)]
            post.execute(np.concatenate(xr), nb, BLOCK, CENTER)
            with pytest.raises(H.CsdrError):
                bank.execute(post)
            for i in range(len(specs)):
                assert bank.digital_results(i) == [] and bank.symbols(i).size == 0
            bank.set_active(len(specs), 0)
            other.close()
            for b in range(nb):                    # the channelizer did see the batch; no demodulator did
                rp.run_block(xr[b], CENTER)
            t0 += nb * BLOCK
        out = set((skip or {}).get(e, []))
        for i in range(len(specs)):
            bank.set_frequency(i, f_out if i in out else freqs[i])
        xs = [synth_iq(BLOCK, FS, CENTER, [("NBFM", f + 3000) for f in freqs], seed=900 + 7 * e + b, t0=t0 + b * BLOCK) for b in range(nb)]
        t0 += nb * BLOCK
        post.execute(np.concatenate(xs), nb, BLOCK, CENTER)
        bank.execute(post)
        want = [[] for _ in specs]
        for b in range(nb):
            rp.run_block(xs[b], CENTER)
            for i, rd in enumerate(rds):
                if i in out:
                    continue
                riq = rd.pre(*rp.channel_data(rp.channel_at(rd.frequency)))
                want[i].append((riq,) + rms[i].demodulate(riq) + (rms[i].lock,))
        for i, (names, rate) in enumerate(specs):
            res, br, syms = bank.digital_results(i), bank.results(i), bank.symbols(i)
            assert len(res) == nb and len(br) == nb
            cons = rgs[i].cons
            if i in out:        # DemodulatorPreThread drops the block: the object keeps its state, whatever the other tables of the slot did since
                own = rgs[i].objs[cons].evm()
                for b in range(nb):
                    r = res[b]
                    assert br[b].skipped == 1 and (r.n_symbols, r.cons) == (0, cons), (i, b)
                    assert evm_close(r.evm, own) and r.lock == int(own <= np.float32(T.SENSITIVITY)), (i, b, r.evm, own)
                    for other_cons, m in rgs[i].objs.items():
                        if other_cons != cons and m.evm() > 0:
                            assert not evm_close(r.evm, m.evm()), "the test cannot tell the two objects' states apart"
                assert syms.size == 0
                skipped_blocks += nb
                continue
            giq = bank.iq(i)
            off = 0
            for b in range(nb):
                riq, wsym, wevm, wlock = want[i][b]
                r = res[b]
                assert br[b].n_iq == riq.size and br[b].n_audio == 0 and br[b].level_count == 0 and br[b].audio_peak == 0.0, (i, b)
                assert (r.n_symbols, r.symbol_offset, r.carry, r.cons) == (wsym.size, off, 0, cons), (i, b, r.n_symbols, wsym.size, r.cons)
                got = syms[off: off + r.n_symbols]
                gseg = giq[sum(x.n_iq for x in br[:b]): sum(x.n_iq for x in br[:b + 1])]
                gsym, gevm = rgs[i].demodulate(gseg)
                # the kernel against the reference on identical input: a difference only where the reference's own decision moves when the
                # input moves by 1e-6 relative
                kbad = got != gsym
                edge = np.zeros(got.size, bool)
                if kbad.any():
                    edge = T.boundary_mask(libs, by_cons[i][cons], gseg, gsym)
                    assert edge[kbad].all(), (names, i, b, np.nonzero(kbad & ~edge)[0][:8])
                kernel_edges += np.count_nonzero(kbad)
                # against the reference front end: a difference only where the reference's decision itself moves between the two front ends'
                # outputs or on one of those boundaries
                diff = got != wsym
                assert np.all((gsym != wsym)[diff] | edge[diff]), (names, i, b, np.nonzero(diff)[0][:8])
                flips += np.count_nonzero(diff)
                total += got.size
                if got.size and not kbad[-1]:
                    assert evm_close(r.evm, gevm), (names, i, b, r.evm, gevm)
                    assert r.lock == rgs[i].lock, (names, i, b, r.lock, gevm)          # the reference's lock on the same samples
                    if abs(wevm - T.SENSITIVITY) > 1e-3:
                        assert r.lock == wlock, (names, i, b, r.lock, wevm)           # ... and behind the reference front end
                off += r.n_symbols
            assert syms.size == off
    for m in rms + rgs:
        m.close()
    bank.close()
    post.close()
    print("table chain: %d of %d decisions differ from the reference front end's, %d from the reference on the bank's own IQ (all on boundaries); "
          "%d skipped blocks repeated their object's EVM" % (flips, total, kernel_edges, skipped_blocks))
    assert flips <= BOUNDARY_SHARE * max(total, 1) and kernel_edges <= BOUNDARY_SHARE * max(total, 1)
    return flips, total, skipped_blocks
