# C3-shaped bank: 256 analog + 32 constellation / FSK + 16 GMSK + 16 table slots, 20 batches (run from the repository root under rocprofv3
# --kernel-trace --stats; profiles/table_mixed_bank.txt).  The tables are built from formulas of the right shape, not from anybody's modem: eight
# slots decide nearest-point among 256 points (a 16 x 16 grid: the longest scan there is), eight by rings (8 rings of 32 points through
# csdr_design_rings: 256 points, the most rings).
import sys
sys.path.insert(0, ".")
import numpy as np
from cubicsdr_amd.engine import Context, DemodBank, SDRPost, design_rings, nearest_table
from tests.util import demod_frequencies
fs, Mc, block, center, nb = 61_440_000, 122, 1_024_068, 100_000_000, 4
ctx = Context(0)
post = SDRPost(ctx, fs, Mc, block, nb)
bank = DemodBank(ctx, 320, nb)
freqs = demod_frequencies(center, fs, 256)
kinds, bws = ["NBFM", "AM", "USB"], {"NBFM": 12_500, "AM": 6_000, "USB": 5_400}
for i, f in enumerate(freqs):
    bank.configure(i, post, kinds[i % 3], bws[kinds[i % 3]], f)
dk = ["PSK", "DPSK", "ASK", "QAM", "BPSK", "QPSK", "OOK", "FSK"]
for j in range(32):
    k = dk[j % 8]
    f = freqs[(8 * j + 3) % 256] + 20_000
    if k == "FSK":
        bank.configure_digital(256 + j, post, k, 19200, f, bps=2, sps=1200)
    else:
        bank.configure_digital(256 + j, post, k, 200000, f, cons=16 if k in ("PSK", "QAM") else 0)
for j in range(16):        # GMSK: the defaults at 19200, sps 16 / fdelay 8, sps 2 / fdelay 1, sps 5 / fdelay 3
    s = [(0, 0, 0.0), (16, 8, 0.25), (2, 1, 0.5), (5, 3, 0.3)][j % 4]
    bank.configure_digital(288 + j, post, "GMSK", 19200 + 100 * j, freqs[(16 * j + 5) % 256] - 15_000, sps=s[0], fdelay=s[1], ebf=s[2])
g = (np.arange(16) - 7.5) / 7.5
grid = nearest_table((g[None, :] + 1j * g[:, None]).reshape(-1) * 0.1)
rings = design_rings(np.concatenate([(l + 1) / 8 * 0.1 * np.exp(2j * np.pi * np.arange(32) / 32) for l in range(8)]))
for j in range(16):
    bank.configure_table(304 + j, post, grid if j < 8 else rings, 200000, freqs[(16 * j + 9) % 256] + 10_000)
rng = np.random.default_rng(5)
x = (rng.standard_normal(nb * block) + 1j * rng.standard_normal(nb * block)).astype(np.complex64) * np.float32(0.1)
for e in range(20):
    post.execute(x, nb, block, center)
    bank.execute(post)
print("symbols slot 256:", bank.symbols(256).size, "slot 288:", bank.symbols(288).size, "slot 304:", bank.symbols(304).size, "slot 312:", bank.symbols(312).size)
bank.close(); post.close(); ctx.close()
