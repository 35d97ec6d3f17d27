# C3-shaped bank: 256 analog + 32 constellation / FSK + 16 GMSK slots, 20 batches (run from the repository root under rocprofv3 --kernel-trace
# --stats; profiles/gmsk_mixed_bank.txt)
import sys
sys.path.insert(0, ".")
import numpy as np
from cubicsdr_amd.engine import Context, DemodBank, SDRPost
from tests.util import demod_frequencies
fs, Mc, block, center, nb = 61_440_000, 122, 1_024_068, 100_000_000, 4
ctx = Context(0)
post = SDRPost(ctx, fs, Mc, block, nb)
bank = DemodBank(ctx, 304, nb)
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
rng = np.random.default_rng(5)
x = (rng.standard_normal(nb * block) + 1j * rng.standard_normal(nb * block)).astype(np.complex64) * np.float32(0.1)
for e in range(20):
    post.execute(x, nb, block, center)
    bank.execute(post)
print("symbols slot 256:", bank.symbols(256).size, "slot 288:", bank.symbols(288).size)
bank.close(); post.close(); ctx.close()
