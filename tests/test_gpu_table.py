"""The table-driven constellations on the MI355X: the decision kernel alone against the reference binary (the cases of tests/test_table_emu.py),
the whole chain SDRPost + DemodBank against the reference front end + the reference binary's APSK / SQAM / V.29 / arb objects, and a C3-shaped
bank whose analog, constellation and GMSK slots must not notice 16 table slots beside them."""
import numpy as np
import pytest

from tests import table_cases as D
from tests import table_oracle as T
from tests.util import demod_frequencies

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not T.available(), reason="the oracle (oracle/_ref) did not travel")]


@pytest.fixture(scope="module")
def ctx():
    from cubicsdr_amd.engine import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return T.Libs(tmp_path_factory.mktemp("table_shim"))


@pytest.mark.parametrize("name", T.NAMES)
def test_table(ctx, libs, name):
    D.check_table(ctx, libs, name)


def test_table_refusals(ctx, libs):
    D.check_refusals(ctx, libs)


def test_table_chain_one_block(ctx, libs):
    D.run_chain(ctx, libs, D.CHAIN, [1, 1, 1])


def test_table_chain_multi_block(ctx, libs):
    D.run_chain(ctx, libs, D.CHAIN, [3, 2, 3])


def test_table_chain_cons_switch(ctx, libs):
    """APSK 16 -> 64 -> 16 (and SQAM 32 -> 128 -> 32, APSK 256 -> 8 -> 256): back on 16, a block the front end drops reports the 16-point object's
    own EVM -- not that of the 64-point object that decided in between -- and the blocks after it carry on from there"""
    flips, total, skipped = D.run_chain(ctx, libs, D.CHAIN, [2, 1, 1, 2], switches={1: [(0, 64), (1, 128), (5, 8)], 2: [(0, 16), (1, 32), (5, 256)]},
                                        skip={2: [0, 1, 5]})
    assert skipped == 3 and total > 0


def test_table_chain_refused_batch(ctx, libs):
    """a batch refused by another slot (built for another channel rate) after the table slots were planned: their objects carry on as if it
    never came -- the reference classes never saw it"""
    D.run_chain(ctx, libs, D.CHAIN, [1, 2, 1, 3, 1, 2], reject=(2, 4, 5))


def test_c3_bank_with_table_slots(ctx, libs):
    """C3 shape (61.44 MS/s, M = 122) with 256 analog, 32 constellation and 16 GMSK slots, with and without 16 table slots: the results, audio and
    symbols of the first three groups are byte-identical"""
    from cubicsdr_amd.engine import DemodBank, SDRPost
    fs, Mc, block, center, nb = 61_440_000, 122, 1_024_068, 100_000_000, 2
    kinds = ["NBFM", "AM", "USB"]
    bws = {"NBFM": 12_500, "AM": 6_000, "USB": 5_400}
    freqs = demod_frequencies(center, fs, 256)
    post = SDRPost(ctx, fs, Mc, block, nb)
    plain, mixed = DemodBank(ctx, 304, nb), DemodBank(ctx, 320, nb)
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
            bank.configure_digital(288 + j, post, "GMSK", 19200 + 100 * j, freqs[(16 * j + 5) % 256] - 15_000, sps=s[0], fdelay=s[1], ebf=s[2])
    names = ["APSK256", "ARB256OPT", "APSK16", "SQAM128", "V29", "USER64", "APSK64", "ARB64VT"]
    tabs = {n: T.product_table(n, T.constellation(libs, n)) for n in names}
    for j in range(16):
        mixed.configure_table(304 + j, post, tabs[names[j % 8]], 200000, freqs[(16 * j + 9) % 256] + 10_000)
    rng = np.random.default_rng(8)
    for e in range(2):
        x = (rng.standard_normal(nb * block) + 1j * rng.standard_normal(nb * block)).astype(np.complex64) * np.float32(0.1)
        post.execute(x, nb, block, center)
        plain.execute(post)
        mixed.execute(post)
        for i in range(256):
            for ra, rb in zip(plain.results(i), mixed.results(i)):
                assert bytes(ra) == bytes(rb), (e, i)
            assert np.array_equal(plain.audio(i), mixed.audio(i)), (e, i)
        for j in range(256, 304):
            assert np.array_equal(plain.symbols(j), mixed.symbols(j)), (e, j)
            assert [bytes(r) for r in plain.digital_results(j)] == [bytes(r) for r in mixed.digital_results(j)], (e, j)
        for j in range(304, 320):
            res = mixed.digital_results(j)
            n = sum(r.n_symbols for r in res)
            assert len(res) == nb and n > 0 and mixed.symbols(j).size == n and all(r.cons == T.n_points(names[(j - 304) % 8]) for r in res)
            assert int(mixed.symbols(j).max()) < res[0].cons
    plain.close(); mixed.close(); post.close()
