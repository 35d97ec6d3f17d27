"""GMSK on the MI355X: the kernels alone against the reference binary's gmskdem (the cases of tests/test_gmsk_emu.py), the chain SDRPost +
DemodBank against ModemGMSK::demodulate's framing around the binary's object fed the bank's own resampled IQ, a settings change, and a
C3-shaped bank whose analog and constellation slots must not notice 16 GMSK slots beside them."""
import numpy as np
import pytest

from tests import gmsk_cases as K
from tests import gmsk_oracle as G
from tests.util import demod_frequencies, synth_iq

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not G.available(), reason="the oracle (oracle/_ref) did not travel")]


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return G.shim(tmp_path_factory.mktemp("gmsk_shim"))


@pytest.mark.parametrize("k,m,bt", K.SETTINGS)
def test_gmsk_modulated(ctx, ref, k, m, bt):
    K.check_modulated(ctx, ref, k, m, bt)


@pytest.mark.parametrize("k,m,bt", K.SETTINGS)
def test_gmsk_noise(ctx, ref, k, m, bt):
    K.check_noise(ctx, ref, k, m, bt)


@pytest.mark.parametrize("k,m,bt", K.SETTINGS)
def test_gmsk_split_stream(ctx, ref, k, m, bt):
    K.check_split(ctx, ref, k, m, bt)


@pytest.mark.parametrize("k,m,bt", [(4, 3, 0.3), (2, 1, 0.5), (5, 2, 0.25), (16, 8, 0.3)])
def test_gmsk_signed_zeros(ctx, ref, k, m, bt):
    K.check_signed_zeros(ctx, ref, k, m, bt)


def test_gmsk_refused(ctx, ref):
    K.check_refused(ctx, ref)


FS, M, BLOCK, CENTER = 2400000, 4, 40000, 100000000
# (rate, sps, fdelay, ebf): the defaults at the default rate (320 samples a block: a multiple of sps) and at 19000 (316 / 317: reads past the end
# occur), a long filter, and sps 16
CHAIN = [(19200, 4, 3, 0.3), (19000, 0, 0, 0.0), (19000, 4, 8, 0.25), (47000, 16, 3, 0.3)]


class Seen:
    def __init__(self):
        self.prefix = self.steady = self.past_end = False

    def note(self, n, n_sym, k):
        read = n_sym * k
        self.prefix |= 0 < read < n - k + 1 if n else False          # only a prefix of the block is demodulated
        self.steady |= n - k < read <= n                               # the block is (about) all demodulated, nothing past its end
        self.past_end |= read > n                                      # the last symbol reads past the block's end


def run_chain(ctx, ref, specs, executes, change=None, reject=()):
    """specs: [(rate, sps, fdelay, ebf)] one GMSK slot each; executes: blocks per execute; change: {execute: (slot, (sps, fdelay, ebf))} a settings
    write (a rebuild) before that execute; reject: executes before which a batch is refused because a slot after the GMSK ones was built for
    another channel rate (the refused batch must leave every GMSK slot as it was).  RefGMSK is fed the bank's own resampled IQ block by block."""
    import cubicsdr_amd.hip as H
    from cubicsdr_amd.engine import DemodBank, SDRPost
    nbmax = max(executes)
    post = SDRPost(ctx, FS, M, BLOCK, nbmax)
    bank = DemodBank(ctx, len(specs) + 1, nbmax)
    freqs = demod_frequencies(CENTER, FS, len(specs))
    sets = [tuple(v or d for v, d in zip(s[1:], (4, 3, 0.3))) for s in specs]
    refs, fed = [], []
    for i, (rate, k, m, bt) in enumerate(specs):
        bank.configure_digital(i, post, "GMSK", rate, freqs[i], sps=k, fdelay=m, ebf=bt)
        refs.append(G.RefGMSK(ref, *sets[i]))
        fed.append([])
    seen = [Seen() for _ in specs]
    t0 = 0
    compared = exempt = 0
    for e, nb in enumerate(executes):
        if change and e in change:
            slot, s = change[e]
            bank.configure_digital(slot, post, "GMSK", specs[slot][0], freqs[slot], sps=s[0], fdelay=s[1], ebf=s[2])
            refs[slot].close()
            refs[slot] = G.RefGMSK(ref, *s)
            sets[slot] = s
            fed[slot] = []
        if e in reject:
            other = SDRPost(ctx, 2 * FS, M, BLOCK, nbmax)
            bank.configure(len(specs), other, "NBFM", 12500, freqs[0])
            xr = synth_iq(BLOCK, FS, CENTER, [("NBFM", f + 3000) for f in freqs], seed=5000 + e, t0=t0)
            post.execute(np.concatenate([xr] * nb), nb, BLOCK, CENTER)
            with pytest.raises(H.CsdrError):
                bank.execute(post)
            bank.set_active(len(specs), 0)
            other.close()
            t0 += nb * BLOCK
        xs = [synth_iq(BLOCK, FS, CENTER, [("NBFM", f + 3000) for f in freqs], seed=300 + 7 * e + b, t0=t0 + b * BLOCK) for b in range(nb)]
        t0 += nb * BLOCK
        post.execute(np.concatenate(xs), nb, BLOCK, CENTER)
        bank.execute(post)
        for i in range(len(specs)):
            k, m, bt = sets[i]
            res, br, syms, giq = bank.digital_results(i), bank.results(i), bank.symbols(i), bank.iq(i)
            assert len(res) == nb and syms.size == sum(r.n_symbols for r in res)
            off = a = 0
            for b in range(nb):
                n = br[b].n_iq
                seg = giq[a:a + n]
                a += n
                wsym, wtext, wcarry = refs[i].demodulate(seg)
                r = res[b]
                assert (r.n_symbols, r.symbol_offset, r.carry, r.lock, r.evm, r.cons) == (wsym.size, off, wcarry, 0, 0.0, 2), (e, i, b, r.n_symbols, wsym.size, r.carry, wcarry)
                seen[i].note(n, wsym.size, k)
                buf = np.zeros(wsym.size * k, np.complex64)
                buf[:min(n, buf.size)] = seg[:buf.size]
                fed[i].append(buf)
                got = syms[off:off + r.n_symbols]
                # near-zero rule: the float64 filter output over everything this object was fed
                _, h_ref = G.taps(ref, k, m, bt)
                d64 = G.soft(h_ref, G.phase_differences(np.concatenate(fed[i])), k)[-wsym.size:] if wsym.size else np.zeros(0)
                bnd, _ = K.bound(ref, k, m, bt)
                firm = np.abs(d64) > bnd
                assert np.array_equal(got[firm], wsym[firm]), (e, i, b, np.flatnonzero(firm & (got != wsym))[:8])
                if firm.all():
                    assert "".join("%x" % int(s) for s in got) == wtext
                compared += got.size
                exempt += np.count_nonzero(~firm)
                off += r.n_symbols
    for rg in refs:
        rg.close()
    bank.close()
    post.close()
    print("gmsk chain: %d decisions, %d exempt" % (compared, exempt))
    return seen


def test_gmsk_chain_one_block(ctx, ref):
    """one block per execute, enough of them for the prefix-only transient, the steady state and reads past the block's end"""
    seen = run_chain(ctx, ref, CHAIN, [1] * 90)
    for i, s in enumerate(seen[1:], 1):
        assert s.prefix and s.steady and s.past_end, (i, vars(s))


def test_gmsk_chain_multi_block(ctx, ref):
    seen = run_chain(ctx, ref, CHAIN, [3, 5, 2, 4] * 6 + [1, 3])
    for i, s in enumerate(seen[1:], 1):
        assert s.prefix and s.steady and s.past_end, (i, vars(s))


def test_gmsk_chain_settings_change(ctx, ref):
    """a settings write rebuilds the kit: a fresh object and an empty inputBuffer"""
    run_chain(ctx, ref, CHAIN[:2], [2] * 30, change={10: (1, (4, 3, 0.4)), 20: (0, (8, 2, 0.3))})


def test_gmsk_chain_refused_batch(ctx, ref):
    """a batch refused by another slot (built for another channel rate) after the GMSK slots were planned: their counts, symbols and history
    carry on as if it never came -- ModemGMSK never saw it"""
    run_chain(ctx, ref, CHAIN, [1, 2, 1, 3, 1, 2, 1, 1, 2, 1], reject=(3, 6, 8))


def test_c3_bank_with_gmsk_slots(ctx):
    """C3 shape (61.44 MS/s, M = 122) with 256 analog and 32 constellation slots, with and without 16 GMSK slots: the analog results and audio and
    the constellation slots' symbols are byte-identical"""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    fs, Mc, block, center, nb = 61_440_000, 122, 1_024_068, 100_000_000, 2
    kinds = ["NBFM", "AM", "USB"]
    bws = {"NBFM": 12_500, "AM": 6_000, "USB": 5_400}
    freqs = demod_frequencies(center, fs, 256)
    post = SDRPost(ctx, fs, Mc, block, nb)
    plain, mixed = DemodBank(ctx, 256 + 32, nb), DemodBank(ctx, 256 + 32 + 16, nb)
    dk = ["PSK", "DPSK", "ASK", "QAM", "BPSK", "QPSK", "OOK", "FSK"]
    for bank in (plain, mixed):
        for i, f in enumerate(freqs):
            k = kinds[i % 3]
            bank.configure(i, post, k, bws[k], f)
        for j in range(32):
            k = dk[j % 8]
            f = freqs[(8 * j + 3) % 256] + 20_000
            if k == "FSK":
                bank.configure_digital(256 + j, post, k, 19200, f, bps=2, sps=1200)
            else:
                bank.configure_digital(256 + j, post, k, 200000, f, cons=16 if k in ("PSK", "QAM") else 0)
    for j in range(16):
        s = [(0, 0, 0.0), (16, 8, 0.25), (2, 1, 0.5), (5, 3, 0.3)][j % 4]
        mixed.configure_digital(288 + j, post, "GMSK", 19200 + 100 * j, freqs[(16 * j + 5) % 256] - 15_000, sps=s[0], fdelay=s[1], ebf=s[2])
    rng = np.random.default_rng(6)
    for e in range(2):
        x = (rng.standard_normal(nb * block) + 1j * rng.standard_normal(nb * block)).astype(np.complex64) * np.float32(0.1)
        post.execute(x, nb, block, center)
        plain.execute(post)
        mixed.execute(post)
        for i in range(256):
            for ra, rb in zip(plain.results(i), mixed.results(i)):
                assert bytes(ra) == bytes(rb), (e, i)
            assert np.array_equal(plain.audio(i), mixed.audio(i)), (e, i)
        for j in range(256, 288):
            assert np.array_equal(plain.symbols(j), mixed.symbols(j)), (e, j)
            assert [bytes(r) for r in plain.digital_results(j)] == [bytes(r) for r in mixed.digital_results(j)], (e, j)
        for j in range(288, 304):
            res = mixed.digital_results(j)
            assert len(res) == nb and mixed.symbols(j).size == sum(r.n_symbols for r in res)
    plain.close(); mixed.close(); post.close()
