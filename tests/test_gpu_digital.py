"""The digital lab on the MI355X: the decision kernel alone against the reference binary (the cases of tests/test_digital_emu.py), the whole
chain SDRPost + DemodBank against the reference front end + the reference binary's modemcf / fskdem objects, and a C3-shaped bank whose
analog demodulators must not notice 32 digital slots beside them."""
import numpy as np
import pytest

from tests import digital_cases as D
from tests import digital_oracle as O
from tests.test_digital_emu import CONSTELLATIONS
from tests.util import demod_frequencies, synth_iq

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not O.available(), reason="the oracle (oracle/_ref) did not travel")]


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return O.shim(tmp_path_factory.mktemp("digital_shim"))


@pytest.mark.parametrize("kind,cons", CONSTELLATIONS)
def test_digital_constellation(ctx, ref, kind, cons):
    D.check_constellation(ctx, ref, kind, cons)


@pytest.mark.parametrize("bps,k,bw", D.FSK_CASES)
def test_digital_fsk(ctx, ref, bps, k, bw):
    D.check_fsk(ctx, ref, bps, k, bw)


@pytest.mark.parametrize("bps,k,bw", D.FSK_REFUSED)
def test_digital_fsk_refused(ctx, ref, capfd, bps, k, bw):
    D.check_fsk_refused(ctx, ref, capfd, bps, k, bw)


def test_digital_configure_routes(ctx):
    D.check_configure_routes(ctx)


FS, M, BLOCK, CENTER = 2400000, 4, 40000, 100000000


def run_chain(ctx, ref, specs, executes, switches=None):
    """specs: [(kind, rate, settings)] one digital slot each; executes: blocks per execute.  Every block goes through the reference front end
    (RefDemod.pre) and the reference modem objects (RefDigital), and -- to tell the front end's last-place differences from the kernel's -- a
    second set of reference objects is fed the bank's own resampled IQ.  Returns the count of decisions that differ from the reference."""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    from oracle.cubicsdr_chain import RefDemod, RefSDRPost
    nbmax = max(executes)
    post = SDRPost(ctx, FS, M, BLOCK, nbmax)
    bank = DemodBank(ctx, len(specs), nbmax)
    rp = RefSDRPost("ref", FS, M)
    freqs = demod_frequencies(CENTER, FS, len(specs))
    rds, rms, rgs = [], [], []
    for i, (kind, rate, kw) in enumerate(specs):
        bank.configure_digital(i, post, kind, rate, freqs[i], **kw)
        rds.append(RefDemod("ref", "NBFM", rate, freqs[i], rp.chan_bw))          # the front end of any slot: NCO + msresamp_crcf to the modem rate
        fsk = {k: v for k, v in kw.items() if k in ("bps", "sps", "bw")}
        rms.append(O.RefDigital(ref, kind, cons=kw.get("cons", 0), rate=rate, **fsk))
        rgs.append(O.RefDigital(ref, kind, cons=kw.get("cons", 0), rate=rate, **fsk))
    flips = total = kernel_edges = 0
    t0 = 0
    last_g = [None] * len(specs)                  # the previous block's last resampled sample (a DPSK decision also reads it)
    for e, nb in enumerate(executes):
        for slot, cons in (switches or {}).get(e, []):
            bank.set_digital_cons(slot, cons)
            rms[slot].set_cons(cons)
            rgs[slot].set_cons(cons)
        xs = [synth_iq(BLOCK, FS, CENTER, [("NBFM", f + 3000) for f in freqs], seed=900 + 7 * e + b, t0=t0 + b * BLOCK) for b in range(nb)]
        t0 += nb * BLOCK
        post.execute(np.concatenate(xs), nb, BLOCK, CENTER)
        bank.execute(post)
        want = [[] for _ in specs]
        for b in range(nb):
            rp.run_block(xs[b], CENTER)
            for i, rd in enumerate(rds):
                riq = rd.pre(*rp.channel_data(rp.channel_at(rd.frequency)))
                want[i].append((riq,) + rms[i].demodulate(riq) + (rms[i].buf.size if specs[i][0] == "FSK" else 0, rms[i].lock if specs[i][0] != "FSK" else 0))
        for i, (kind, rate, kw) in enumerate(specs):
            res, br, syms, giq = bank.digital_results(i), bank.results(i), bank.symbols(i), bank.iq(i)
            assert len(res) == nb and len(br) == nb
            off = 0
            for b in range(nb):
                riq, wsym, wevm, wtext, wcarry, wlock = want[i][b]
                r = res[b]
                assert br[b].n_iq == riq.size and br[b].n_audio == 0 and br[b].level_count == 0 and br[b].audio_peak == 0.0, (i, b)
                assert (r.n_symbols, r.symbol_offset, r.carry) == (wsym.size, off, wcarry), (i, b, r.n_symbols, wsym.size, r.carry, wcarry)
                got = syms[off: off + r.n_symbols]
                gseg = giq[sum(x.n_iq for x in br[:b]): sum(x.n_iq for x in br[:b + 1])]
                gsym, gevm, _ = rgs[i].demodulate(gseg)
                # the kernel against the reference on identical input: a difference only where the reference's own decision moves when the
                # input moves by 1e-6 relative (fresh objects; for DPSK the previous block's last sample goes in front)
                kbad = got != gsym
                edge = np.zeros(got.size, bool)
                if kind == "FSK":
                    assert not kbad.any(), (kind, i, b, np.nonzero(kbad)[0][:8])
                elif kbad.any():
                    pre = gseg if last_g[i] is None else np.concatenate([last_g[i], gseg])
                    cons = rgs[i].cons
                    m = O.Modem(ref, kind, cons)
                    base = m.demodulate(pre)
                    m.close()
                    edge = O.boundary_mask(ref, kind, cons, pre, base)[pre.size - gseg.size:]
                    assert edge[kbad].all(), (kind, i, b, np.nonzero(kbad & ~edge)[0][:8])
                kernel_edges += np.count_nonzero(kbad)
                if gseg.size:
                    last_g[i] = gseg[-1:]
                # against the reference front end: a difference only where the reference's decision itself moves between the two front ends'
                # outputs (a perturbation as large as the measured front-end difference) or on one of those boundaries
                diff = got != wsym
                assert np.all((gsym != wsym)[diff] | edge[diff]), (kind, i, b, np.nonzero(diff)[0][:8])
                flips += np.count_nonzero(diff)
                total += got.size
                if kind == "FSK":
                    assert "".join("%x" % int(s) for s in got) == wtext or np.any(diff)
                elif got.size and not kbad[-1]:
                    assert abs(r.evm - gevm) <= 1e-6 + 1e-5 * gevm, (kind, i, b, r.evm, gevm)
                    assert r.lock == rgs[i].lock, (kind, i, b, r.lock, gevm)          # the reference's lock on the same samples
                    if abs(wevm - O.SENSITIVITY[kind]) > 1e-3:
                        assert r.lock == wlock, (kind, i, b, r.lock, wevm)           # ... and behind the reference front end
                off += r.n_symbols
            assert syms.size == off
    for m in rms + rgs:
        m.close()
    bank.close()
    post.close()
    print("digital chain: %d of %d decisions differ from the reference front end's, %d from the reference on the bank's own IQ (all on boundaries)"
          % (flips, total, kernel_edges))
    assert flips <= D.BOUNDARY_SHARE * max(total, 1) and kernel_edges <= D.BOUNDARY_SHARE * max(total, 1)
    return flips


SPECS = [("PSK", 200000, dict(cons=8)), ("DPSK", 200000, dict(cons=4)), ("QAM", 200000, dict(cons=16)), ("ASK", 200000, dict(cons=4)),
         ("BPSK", 200000, {}), ("QPSK", 200000, {}), ("OOK", 200000, {}), ("FSK", 19200, dict(bps=2, sps=1000, bw=0.45))]


def test_digital_chain_one_block(ctx, ref):
    run_chain(ctx, ref, SPECS, [1, 1, 1])


def test_digital_chain_multi_block(ctx, ref):
    """batches of 3 and 2 blocks: the FSK carry crosses blocks and executes, DPSK's phase crosses executes"""
    run_chain(ctx, ref, SPECS, [3, 2, 3])


def test_digital_chain_cons_switch(ctx, ref):
    """writeSetting("cons") between executes, then back: each constellation resumes its own object's state"""
    specs = [("PSK", 200000, dict(cons=8)), ("DPSK", 200000, dict(cons=4)), ("QAM", 200000, dict(cons=16)), ("ASK", 200000, dict(cons=2))]
    run_chain(ctx, ref, specs, [2, 1, 2, 1], switches={1: [(0, 4), (1, 8), (2, 64), (3, 8)], 3: [(0, 8), (1, 4), (2, 16), (3, 2)]})


def test_digital_fsk_default_settings(ctx, ref):
    """ModemFSK's defaults (bps 1, sps 9600, bw 0.45) at its default rate 19200: k = 2"""
    run_chain(ctx, ref, [("FSK", 19200, {}), ("FSK", 48000, dict(bps=4, sps=1200, bw=0.3))], [2, 1])


def test_c3_bank_with_digital_slots(ctx):
    """C3 shape (61.44 MS/s, M = 122, 256 NBFM / AM / USB) with 32 digital slots in the same bank: the analog audio, block results and bit-exact
    words are those of the bank without them"""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    fs, Mc, block, center, nb = 61_440_000, 122, 1_024_068, 100_000_000, 2
    kinds = ["NBFM", "AM", "USB"]
    bws = {"NBFM": 12_500, "AM": 6_000, "USB": 5_400}
    freqs = demod_frequencies(center, fs, 256)
    post = SDRPost(ctx, fs, Mc, block, nb)
    plain, mixed = DemodBank(ctx, 256, nb), DemodBank(ctx, 256 + 32, nb)
    for i, f in enumerate(freqs):
        k = kinds[i % 3]
        plain.configure(i, post, k, bws[k], f)
        mixed.configure(i, post, k, bws[k], f)
    dk = ["PSK", "DPSK", "ASK", "QAM", "BPSK", "QPSK", "OOK", "FSK"]
    for j in range(32):
        k = dk[j % 8]
        f = freqs[(8 * j + 3) % 256] + 20_000
        if k == "FSK":
            mixed.configure_digital(256 + j, post, k, 19200, f, bps=2, sps=1200)
        else:
            mixed.configure_digital(256 + j, post, k, 200000, f, cons=16 if k in ("PSK", "QAM") else 0)
    rng = np.random.default_rng(5)
    for e in range(2):
        x = (rng.standard_normal(nb * block) + 1j * rng.standard_normal(nb * block)).astype(np.complex64) * np.float32(0.1)
        post.execute(x, nb, block, center)
        plain.execute(post)
        mixed.execute(post)
        for i in range(256):
            a, b = plain.results(i), mixed.results(i)
            for ra, rb in zip(a, b):
                assert bytes(ra) == bytes(rb), (e, i)
            assert np.array_equal(plain.audio(i), mixed.audio(i)), (e, i)
        for j in range(32):
            res = mixed.digital_results(256 + j)
            assert len(res) == nb
            assert mixed.symbols(256 + j).size == sum(r.n_symbols for r in res)
    plain.close(); mixed.close(); post.close()
