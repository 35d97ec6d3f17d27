# The waterfall bank's kernels alone at the shape of wfbank_rate.py (256 slots, fft_size 1024, 256 lines, four device lines per slot and turn,
# 128 x 64 LINEAR thumbnails as a 16-column atlas): 200 turns of step + update + render under the HIP-event profile (csdr_ctx_profile_*), i.e. 200
# launches per kernel and process where wfbank_rate.py has three.  It uses nothing newer than csdr_wfbank itself, so it runs unchanged in a
# checkout of an older commit.  Run from the repository root on an MI355X:   python profiles/wfbank_kernel_rate.py
import sys
sys.path.insert(0, ".")
import torch
from cubicsdr_amd.engine import Context, WaterfallBank
SLOTS, F, LINES, W, HH, COLS, N = 256, 1024, 256, 128, 64, 16, 200
ctx = Context(0)
wb = WaterfallBank(ctx, F, LINES, SLOTS, 8)
g = torch.Generator(device="cuda:0").manual_seed(7)
v = torch.rand(SLOTS, 4, F, device="cuda:0", generator=g).contiguous()
torch.cuda.synchronize()
items = [(s, v[s]) for s in range(SLOTS)]
def turn():
    wb.step(items); wb.update(); wb.view(SLOTS, W, HH, "linear", COLS, fetch=False); wb.device_view(); ctx.synchronize()
for _ in range(5):
    turn()
ctx.profile_enable(True)
for _ in range(N):
    turn()
prof = ctx.profile()
ctx.profile_enable(False)
for k in ("wfb_quantize", "wfb_update", "wfb_view_linear"):
    ms, n, _ = prof[k]
    print("%-16s %.2f us per launch (%d launches)" % (k, ms / n * 1e3, n))
wb.close(); ctx.close()
