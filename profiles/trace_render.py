#!/usr/bin/env python3
"""What a trace bank render costs on the device, beside a hipMemsetAsync of the same picture bytes in the same run (the kernel is bound by writing
the picture, so the ratio to the fill is the honest figure):

  (a) a 256-slot atlas of 256 x 64 tiles from spectrum points of F = 2048, with hold;
  (b) one 1920 x 256 tile from 65536 points;
  (c) a 256-slot scope atlas of 256 x 64 tiles from 1024-sample Y frames ((x, y) pairs, as the scope bank holds them).

All points lie in device memory.  Per shape, after warm-up, over N renders: the median, shortest and longest kernel time by HIP events on the
object's stream (the library's per-kernel profile, read after every render), the median wall time of a render call that leaves the picture on the
device and ends in a synchronise, and the median of N fills timed by HIP events.  python profiles/trace_render.py [N] > profiles/trace_render.txt"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cubicsdr_amd.hip as H                                           # noqa: E402
from cubicsdr_amd.engine import Context, DevicePointer, TraceBank      # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARM = 5


def main():
    ctx = Context(0)
    lib = H.lib()
    hip = C.CDLL("libamdhip64.so")
    rng = np.random.default_rng(1)
    allocs = []

    def dev(a):
        a = np.ascontiguousarray(a, np.float32).ravel()
        p = C.c_void_p()
        H.check(lib.csdr_dev_alloc(ctx.h, a.nbytes, C.byref(p)))
        H.check(lib.csdr_dev_upload(ctx.h, p, a.ctypes.data_as(C.c_void_p), a.nbytes))
        allocs.append(p)
        return p.value

    def fill_ms(n_bytes):
        p = C.c_void_p()
        H.check(lib.csdr_dev_alloc(ctx.h, n_bytes, C.byref(p)))
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        ms = []
        for k in range(WARM + N):
            assert hip.hipEventRecord(e0, None) == 0
            assert hip.hipMemsetAsync(p, 0, C.c_size_t(n_bytes), None) == 0
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            if k >= WARM:
                ms.append(t.value)
        hip.hipEventDestroy(e0), hip.hipEventDestroy(e1)
        H.check(lib.csdr_dev_free(ctx.h, p))
        return statistics.median(ms)

    def kernel_total():
        return sum(v[0] for k, v in ctx.profile().items() if k.startswith("trace_"))

    def measure(name, tb, items, W, Hh, cols):
        for _ in range(WARM):
            tb.render(items, W, Hh, cols, fetch=False)
        tb.device_view(), ctx.synchronize()
        wall = []
        for _ in range(N):
            t0 = time.perf_counter()
            tb.render(items, W, Hh, cols, fetch=False)
            tb.device_view(), ctx.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.profile_enable(True)
        kern, last = [], kernel_total()
        for _ in range(N):
            tb.render(items, W, Hh, cols, fetch=False)
            tb.device_view(), ctx.synchronize()                       # (the profile's drain does not wait for an object's own stream)
            now = kernel_total()
            kern.append(now - last)
            last = now
        ctx.profile_enable(False)
        n_bytes = 4 * W * Hh * len(items)
        fill = fill_ms(n_bytes)
        out = dict(shape=name, picture_bytes=n_bytes, renders=N, kernel_ms_median=round(statistics.median(kern), 5), kernel_ms_min=round(min(kern), 5),
                   kernel_ms_max=round(max(kern), 5), fill_ms_median=round(fill, 5), kernel_over_fill=round(statistics.median(kern) / fill, 2),
                   render_call_wall_ms_median=round(statistics.median(wall), 4),
                   picture_gb_per_s=round(n_bytes / statistics.median(kern) / 1e6, 1))
        print(json.dumps(out), flush=True)

    tb = TraceBank(ctx, max_items=256, max_points=1 << 16)
    F = 2048
    pts, hold = dev(rng.uniform(0, 1, (256, F))), dev(rng.uniform(0, 1, (256, F)))
    measure("a: 256 spectrum tiles of 256 x 64, F = 2048, with hold", tb,
            [dict(kind="spectrum", points=DevicePointer(pts + 4 * F * s, F), hold=DevicePointer(hold + 4 * F * s, F), n=F) for s in range(256)], 256, 64, 16)
    big = dev(rng.uniform(0, 1, 65536))
    measure("b: one spectrum tile of 1920 x 256, 65536 points", tb, [dict(kind="spectrum", points=DevicePointer(big, 65536), n=65536)], 1920, 256, 1)
    L = 1024
    xy = np.stack([np.tile(np.linspace(-1, 1, L, dtype=np.float32), (256, 1)), rng.uniform(-1, 1, (256, L)).astype(np.float32)], axis=2)
    sc = dev(xy)
    measure("c: 256 scope Y tiles of 256 x 64, 1024-sample frames", tb,
            [dict(kind="y", points=DevicePointer(sc + 8 * L * s, 2 * L), n=L, layout=1) for s in range(256)], 256, 64, 16)
    tb.close()
    for p in allocs:
        H.check(lib.csdr_dev_free(ctx.h, p))
    ctx.close()


if __name__ == "__main__":
    main()
