"""The waterfall feed -- from a block that lies in HBM to finished spectrum lines -- timed two ways at 61.44 MS/s with blocks of 1 024 000 samples
(1/60 s), at the reference cadence (30 lines/s of 4096 samples, fftSize 2048) and at a heavy one (1000 lines/s of 131072 samples, the C3 spectrum's
fftSize 65536).  Run on the GPU box from the repo root:

    python profiles/distributor_rate.py a   route (a), what exists WITHOUT csdr_distrib: csdr_dev_download of every block, FFTDataDistributor's line
                                            cutting on the host, one host csdr_spec_process per line.  It uses nothing but the API of the commit before
                                            the distributor, and is measured on a checkout of that commit.
    python profiles/distributor_rate.py b   route (b): csdr_distrib_push of the device block + csdr_spec_process_distrib, and distrib_gather alone by
                                            HIP events (bytes read + written per second) beside the plain-copy figures of profiles/r05_copy_rate.txt.

A pass is NB blocks; the host clock runs around work that ends in a device synchronise; two warm-up passes, then REPEATS timed passes; median,
extremes and spread are printed."""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, '.')
import cubicsdr_amd.hip as H
from cubicsdr_amd.engine import Context, SpectrumProcessor

RATE, BLOCK, NB, REPEATS, FREQ = 61440000, 1024000, 8, 9, 100000000
CADENCES = [("reference: 30 lines/s of 4096 samples", 2048, 30), ("heavy: 1000 lines/s of 131072 samples", 65536, 1000)]
route = sys.argv[1] if len(sys.argv) > 1 else ""
if route not in ("a", "b"):
    sys.exit(__doc__)

import torch

ctx = Context(0)
g = torch.Generator(device="cuda:0").manual_seed(5)
x = (torch.randn(NB * BLOCK, 2, device="cuda:0", generator=g) * 0.05).contiguous()
torch.cuda.synchronize()


def report(label, times, extra=""):
    t = sorted(times)
    med = t[len(t) // 2]
    print("%-52s median %9.3f ms   min %9.3f   max %9.3f   spread %4.1f %%   (%d passes)%s" % (label, med * 1e3, t[0] * 1e3, t[-1] * 1e3, 100 * (t[-1] - t[0]) / t[0], len(t), extra), flush=True)
    return med


def timed(one_pass):
    times = []
    for k in range(2 + REPEATS):
        t0 = time.perf_counter()
        one_pass()
        ctx.synchronize()
        if k >= 2:
            times.append(time.perf_counter() - t0)
    return times


class HostCutter:
    """FFTDataDistributor's take() and cutLines() on a numpy buffer (cubicsdr_amd/host/FFTDataDistributor.h restated): the host stage route (a) needs"""

    def __init__(self, fft, lps, rate):
        self.fft, self.lps, self.rate = fft, lps, rate
        self.cap = max(int(rate * 0.25), int(1.2 * fft))
        self.buf = np.empty(self.cap, np.complex64)
        self.head = self.count = 0
        self.accum = 0.0

    def push(self, blk):
        n = blk.size
        if self.head + self.count + n > self.cap:
            self.buf[:self.count] = self.buf[self.head:self.head + self.count].copy()
            self.head = 0
            n = min(n, self.cap - self.count)
        self.buf[self.head + self.count:self.head + self.count + n] = blk[:n]
        self.count += n
        fft, lines = self.fft, []
        if self.count < fft:
            return lines
        step = (self.lps * (self.count / self.rate)) / (self.count / fft)
        if self.accum + step * (self.count / fft) < 1.0:
            self.accum += step * (self.count / fft)
            used = self.count
        else:
            used = 0
            while used + fft <= self.count:
                self.accum += step
                if self.accum >= 1.0:
                    lines.append(self.buf[self.head + used:self.head + used + fft].copy())
                    while self.accum >= 1.0:
                        self.accum -= 1.0
                used += fft
        self.count -= used
        self.head = 0 if self.count == 0 else self.head + used
        return lines


for label, F, lps in CADENCES:
    line = 2 * F
    print("## %s (fftSize %d), %d blocks of %d samples per pass" % (label, F, NB, BLOCK))
    if route == "a":
        spec = SpectrumProcessor(ctx, F, max_frames=1)
        cut = HostCutter(line, lps, RATE)
        host = np.empty(BLOCK, np.complex64)
        made = [0]

        def one_pass():
            for b in range(NB):
                H.check(H.lib().csdr_dev_download(ctx.h, host.ctypes.data_as(C.c_void_p), C.c_void_p(x.data_ptr() + 8 * b * BLOCK), host.nbytes))
                for ln in cut.push(host):
                    spec.process(ln, 1, line)
                    made[0] += 1

        med = report("(a) download + host cutting + process per line", timed(one_pass))
        print("    per block %.1f us; %d bytes per block over the link and through a host core; %.1f lines per pass" % (med / NB * 1e6, 8 * BLOCK, made[0] / (2 + REPEATS)))
        spec.close()
    else:
        from cubicsdr_amd.engine import Distributor
        spec = SpectrumProcessor(ctx, F, max_frames=16)
        dist = Distributor(ctx, 16, line, lps)
        made, moved = [0], [0]

        def one_pass():
            for b in range(NB):
                n = dist.push(x[b * BLOCK:(b + 1) * BLOCK], FREQ, RATE)
                dist.process_into(spec)
                made[0] += n
                moved[0] += 16 * (n * line + int(dist.state.buffered_items))        # bytes read + written by the push's gather

        med = report("(b) csdr_distrib_push + csdr_spec_process_distrib", timed(one_pass))
        print("    per block %.1f us; nothing crosses the link; %.1f lines per pass" % (med / NB * 1e6, made[0] / (2 + REPEATS)))
        ctx.profile_enable(1)
        moved[0] = 0
        for _ in range(REPEATS):
            one_pass()
        ctx.synchronize()
        dist.fetch_buffered()                                        # (synchronises the distributor's own stream)
        prof = ctx.profile()
        ctx.profile_enable(False)
        ms, launches, _ = prof["distrib_gather"]
        per = ms / launches
        print("distrib_gather %8.1f us per launch, %7.2f MB read + written per launch -> %5.2f TB/s   (%d launches)" % (per * 1e3, moved[0] / launches / 1e6, moved[0] / launches / (per * 1e-3) / 1e12, launches))
        dist.close()
        spec.close()

if route == "b":
    # the kernel away from the launch floor: one push that cuts 112 lines of 131072 samples (235 MB read + written)
    from cubicsdr_amd.engine import Distributor
    n_big = 112 * 131072 + 4096
    big = torch.randn(n_big, 2, device="cuda:0", generator=g).contiguous()
    torch.cuda.synchronize()
    dist = Distributor(ctx, 128, 131072, 1000000)
    dist.push(big[:8], FREQ, RATE)                                  # sets rate and frequency: bufferMax = 0.25 s = 15.36 M samples
    ctx.profile_enable(1)
    for k in range(REPEATS):
        dist.push(big, FREQ + 1 + k, RATE)                          # (a retune per push: everything buffered is dropped, the block is taken whole)
        assert dist.state.n_lines == 112
        dist.fetch_buffered()
    prof = ctx.profile()
    ctx.profile_enable(False)
    ms, launches, _ = prof["distrib_gather"]
    per, moved = ms / launches, 16 * n_big
    print("## distrib_gather on one large push: 112 lines of 131072 samples + a carry of 4096")
    print("distrib_gather %8.1f us per launch, %7.2f MB read + written per launch -> %5.2f TB/s   (%d launches)" % (per * 1e3, moved / 1e6, moved / (per * 1e-3) / 1e12, launches))
    print("plain float4 copy on these boxes (profiles/r05_copy_rate.txt): 5.2 - 5.7 TB/s, nt loads + stores 5.9 - 6.2")
    dist.close()
ctx.close()
