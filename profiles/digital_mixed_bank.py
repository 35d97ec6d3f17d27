# C3-shaped bank: 256 analog + 32 digital slots, 20 batches (run from the repository root under rocprofv3 --kernel-trace --stats; profiles/r07_digital_mixed_bank.txt)
import sys
sys.path.insert(0, ".")
import numpy as np
from cubicsdr_amd.engine import Context, DemodBank, SDRPost
from tests.util import demod_frequencies
fs, Mc, block, center, nb = 61_440_000, 122, 1_024_068, 100_000_000, 4
ctx = Context(0)
post = SDRPost(ctx, fs, Mc, block, nb)
bank = DemodBank(ctx, 288, nb)
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
rng = np.random.default_rng(5)
x = (rng.standard_normal(nb * block) + 1j * rng.standard_normal(nb * block)).astype(np.complex64) * np.float32(0.1)
for e in range(20):
    post.execute(x, nb, block, center)
    bank.execute(post)
ctx.synchronize() if hasattr(ctx, "synchronize") else None
print("symbols slot 256:", bank.symbols(256).size)
bank.close(); post.close(); ctx.close()
