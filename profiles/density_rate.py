#!/usr/bin/env python3
"""What the density bank costs on the device, beside a plain device-to-device copy that moves the bytes the launches MUST read and write (points,
state in and out for a step; state in and picture out for a render), measured in the same run:

  (a) one 1920 x 256 slot stepped through step_spec with the 953 frames of a 65536-point spectrum (one C3 batch: 61.44 MS/s, every sample FFT'ed);
  (b) 256 slots of 512 x 128 stepped through step_specbank behind a 256-slot spectrum bank of fftSize 1024 -- a STAND-IN for the spectrum bank
      behind the C3 demodulator bank: the bank is fed 8 host inputs of 2048 samples per slot, not a C3 execute, and the frames it made of them are
      counted in the output (`frames`);
  (c) the render of each: one 1920 x 256 tile, and a 16 x 16 atlas of the 256 tiles.

The points are what the spectrum objects left in HBM (noise, a carrier and a DC spike), so the intervals have the lengths a real trace has.  Per
shape, after warm-up, over N calls: the median, shortest and longest sum of the call's kernel times by HIP events on the object's stream (the
library's per-kernel profile, read after every call), and the median of N copies timed by HIP events.  A copy of B bytes reads B and writes B, so
the copy is made over half the bytes the launches read and write.  python profiles/density_rate.py [N] > profiles/density_rate.txt"""
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cubicsdr_amd.hip as H                                                                   # noqa: E402
from cubicsdr_amd.engine import Context, DensityBank, SpectrumBank, SpectrumProcessor           # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
WARM = 3


def main():
    import torch
    ctx = Context(0)
    lib = H.lib()
    hip = C.CDLL("libamdhip64.so")

    def copy_ms(n_bytes):
        a, b = C.c_void_p(), C.c_void_p()
        H.check(lib.csdr_dev_alloc(ctx.h, n_bytes, C.byref(a)))
        H.check(lib.csdr_dev_alloc(ctx.h, n_bytes, C.byref(b)))
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        ms = []
        for k in range(WARM + N):
            assert hip.hipEventRecord(e0, None) == 0
            assert hip.hipMemcpyAsync(b, a, C.c_size_t(n_bytes), 3, None) == 0          # hipMemcpyDeviceToDevice
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            if k >= WARM:
                ms.append(t.value)
        hip.hipEventDestroy(e0), hip.hipEventDestroy(e1)
        H.check(lib.csdr_dev_free(ctx.h, a)), H.check(lib.csdr_dev_free(ctx.h, b))
        return statistics.median(ms)

    def kernels(prefixes):
        return sum(v[0] for k, v in ctx.profile().items() if k in prefixes)

    def measure(name, call, sync, names, moved_bytes, extra):
        for _ in range(WARM):
            call()
        sync()
        ctx.profile_enable(True)
        kern, last = [], kernels(names)
        for _ in range(N):
            call()
            sync()                                        # (the profile's drain does not wait for an object's own stream)
            now = kernels(names)
            kern.append(now - last)
            last = now
        ctx.profile_enable(False)
        cp = copy_ms(moved_bytes // 2)
        med = statistics.median(kern)
        print(json.dumps(dict(shape=name, calls=N, kernel_ms_median=round(med, 5), kernel_ms_min=round(min(kern), 5), kernel_ms_max=round(max(kern), 5),
                              bytes_read_and_written=moved_bytes, copy_ms_median=round(cp, 5), kernel_over_copy=round(med / cp, 2),
                              gb_per_s=round(moved_bytes / med / 1e6, 1), **extra)), flush=True)

    step_k, render_k = ("density_cover", "density_fold"), ("density_render",)
    # ---- (a) and its render
    F, frames, W, Hh = 65536, 953, 1920, 256
    sp = SpectrumProcessor(ctx, F, max_frames=frames)
    sp.set_hide_dc(True, center_freq=100000000, bandwidth=61440000, input_freq=100000000)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    n = frames * 2 * F
    x = torch.view_as_complex((torch.randn(n, 2, device="cuda:0", generator=g) * 0.05).contiguous())
    x = (x + 0.3 * torch.exp(2j * np.pi * 0.0371 * torch.arange(n, device="cuda:0", dtype=torch.float64)).to(torch.complex64) + 0.3).contiguous()
    torch.cuda.synchronize()
    assert sp.process(x, 1, n, contiguous=True) == frames
    db = DensityBank(ctx, W, Hh, 1, frames, F)
    measure("a: step_spec, one 1920 x 256 slot, 953 frames of 65536 points", lambda: db.step_spec(0, sp, 0, frames, keep_q16=60000), lambda: db.peak(0), step_k,
            frames * F * 4 + 2 * W * Hh * 4, dict(points_bytes=frames * F * 4, state_bytes=W * Hh * 4))
    print(json.dumps(dict(shape="a: the slot after the timed steps", peak=db.peak(0), lit_cells=int((db.fetch(0) > 0).sum()))), flush=True)
    measure("c1: render of (a), one 1920 x 256 tile", lambda: db.render([(0, 0)], fetch=False), lambda: (db.device_view(), ctx.synchronize()), render_k,
            2 * W * Hh * 4, dict(picture_bytes=W * Hh * 4))
    db.close(), sp.close()
    del x
    # ---- (b) and its render
    Fb, S, per = 1024, 256, 8
    W, Hh = 512, 128
    sb = SpectrumBank(ctx, Fb, S, per)
    r = np.random.default_rng(2)
    t = np.arange(2 * Fb)
    items = [(s, (0.3 * np.exp(2j * np.pi * (0.01 + 0.003 * s) * t) + 0.05 * (r.standard_normal(2 * Fb) + 1j * r.standard_normal(2 * Fb))).astype(np.complex64))
             for s in range(S) for _ in range(per)]
    sb.process(items)
    got = sum(sb.frames(s) for s in range(S))
    db = DensityBank(ctx, W, Hh, S, per, Fb)
    measure("b: step_specbank, 256 slots of 512 x 128, fftSize 1024", lambda: db.step_specbank(sb, keep_q16=60000), lambda: db.peak(0), step_k,
            got * Fb * 4 + 2 * S * W * Hh * 4, dict(points_bytes=got * Fb * 4, state_bytes=S * W * Hh * 4, frames=got))
    measure("c2: render of (b), 16 x 16 atlas of 512 x 128 tiles", lambda: db.render([(s, 0) for s in range(S)], 16, fetch=False),
            lambda: (db.device_view(), ctx.synchronize()), render_k, 2 * S * W * Hh * 4, dict(picture_bytes=S * W * Hh * 4))
    db.close(), sb.close()
    ctx.close()


if __name__ == "__main__":
    main()
