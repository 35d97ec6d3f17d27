#!/usr/bin/env python3
"""What an overlay compose costs on the device, beside a device-to-device copy of the same picture measured in the same run (the kernel reads the
picture once and writes it once, as the copy does, so the ratio to the copy is the honest figure):

  (a) a 256-tile atlas of 512 x 128 tiles over a device base, every tile with a full annotation list of its own (engine.spectrum_annotations: dB
      grid, frequency ticks, MHz labels, dB labels, three demodulator markers with labels);
  (a') the same lists moved 2^19 pixels to the right, so that every primitive is read and culled and none is painted;
  (b) the same atlas and base with empty lists;
  (c) one 1920 x 256 tile with such a list.

The font is synthetic (a random coverage plane, 12 x 16 glyphs): the product ships none.  Per shape, after warm-up, over N composes: the median,
shortest and longest kernel time by HIP events on the object's stream (the library's per-kernel profile, read after every compose), the median wall
time of a compose call that leaves the picture on the device and ends in a synchronise, and the median of N copies timed by HIP events.
python profiles/overlay_compose.py [N] > profiles/overlay_compose.txt"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cubicsdr_amd.hip as H                                           # noqa: E402
from cubicsdr_amd import engine as E                                   # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARM = 5


def synthetic_font():
    rng = np.random.default_rng(2)
    plane = rng.integers(0, 256, (64, 256), dtype=np.uint8)
    chars = "0123456789.-dB[]VRMS "
    glyphs = np.array([(ord(c), 12 * (k % 21), 16 * (k // 21), 0 if c == " " else 10, 14, 1, 1, 12) for k, c in enumerate(chars)], E.GLYPH_DTYPE)
    return plane, glyphs, 16


def main():
    ctx = E.Context(0)
    lib = H.lib()
    hip = C.CDLL("libamdhip64.so")
    plane, glyphs, line_height = synthetic_font()

    def copy_ms(src, n_bytes):
        dst = C.c_void_p()
        H.check(lib.csdr_dev_alloc(ctx.h, n_bytes, C.byref(dst)))
        e0, e1 = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        ms = []
        for k in range(WARM + N):
            assert hip.hipEventRecord(e0, None) == 0
            assert hip.hipMemcpyAsync(dst, C.c_void_p(src), C.c_size_t(n_bytes), 3, None) == 0          # hipMemcpyDeviceToDevice
            assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
            t = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(t), e0, e1) == 0
            if k >= WARM:
                ms.append(t.value)
        hip.hipEventDestroy(e0), hip.hipEventDestroy(e1)
        H.check(lib.csdr_dev_free(ctx.h, dst))
        return statistics.median(ms)

    def kernel_total():
        return sum(v[0] for k, v in ctx.profile().items() if k.startswith("overlay_"))

    def measure(name, ov, prims, runs, W, Hh, cols):
        n_bytes = 4 * W * Hh * len(runs)
        pic = np.random.default_rng(3).integers(0, 256, n_bytes, dtype=np.uint8)
        p = C.c_void_p()
        H.check(lib.csdr_dev_alloc(ctx.h, n_bytes, C.byref(p)))
        H.check(lib.csdr_dev_upload(ctx.h, p, pic.ctypes.data_as(C.c_void_p), n_bytes))
        base = E.DevicePointer(p.value, n_bytes // 4)

        def once():
            ov.compose(prims, runs, W, Hh, cols, base=base, fetch=False)
            ov.device_view(), ctx.synchronize()                       # (the profile's drain does not wait for an object's own stream)
        for _ in range(WARM):
            once()
        wall = []
        for _ in range(N):
            t0 = time.perf_counter()
            once()
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.profile_enable(True)
        kern, last = [], kernel_total()
        for _ in range(N):
            once()
            now = kernel_total()
            kern.append(now - last)
            last = now
        ctx.profile_enable(False)
        copy = copy_ms(p.value, n_bytes)
        H.check(lib.csdr_dev_free(ctx.h, p))
        med = statistics.median(kern)
        print(json.dumps(dict(shape=name, picture_bytes=n_bytes, primitives=int(len(prims)), primitives_per_tile=round(sum(c for _, c in runs) / len(runs), 1), composes=N,
                              kernel_ms_median=round(med, 5), kernel_ms_min=round(min(kern), 5), kernel_ms_max=round(max(kern), 5), copy_ms_median=round(copy, 5),
                              kernel_over_copy=round(med / copy, 2), compose_call_wall_ms_median=round(statistics.median(wall), 4),
                              read_plus_write_gb_per_s=round(2 * n_bytes / med / 1e6, 1))), flush=True)

    def annotations(W, Hh, k):
        centre = 100000000 + 37000 * k
        markers = [dict(freq=centre - 400000 + 10000 * k, bandwidth=200000, label="10%d" % k, flags=H.MARKER_CENTERLINE, rgb=(200, 60, 60)),
                   dict(freq=centre + 300000, bandwidth=12500, label="9", flags=H.MARKER_CENTERLINE | H.MARKER_MUTED, rgb=(60, 200, 60)),
                   dict(freq=centre + 700000, bandwidth=3000, sideband="usb", label="7", flags=H.MARKER_CENTERLINE | H.MARKER_RECORDING, rgb=(60, 60, 200))]
        return E.spectrum_annotations(W, Hh, centre, 2400000, 1.0, 126.0, 1024, glyphs, line_height, markers=markers)

    ov = E.OverlayBank(ctx, max_tiles=256, max_prims=1 << 17)
    ov.set_font(plane)
    prims, runs = E.OverlayBank.pack([annotations(512, 128, k) for k in range(256)])
    measure("a: 256 tiles of 512 x 128, a full annotation list per tile", ov, prims, runs, 512, 128, 16)
    away = prims.copy()
    away["x"] += 1 << 19
    measure("a': the lists of a, every primitive outside its tile", ov, away, runs, 512, 128, 16)
    measure("b: 256 tiles of 512 x 128, empty lists", ov, E.overlay_prims(), [(0, 0)] * 256, 512, 128, 16)
    one = annotations(1920, 256, 0)
    measure("c: one tile of 1920 x 256, a full annotation list", ov, one, [(0, len(one))], 1920, 256, 1)
    ov.close()
    ctx.close()


if __name__ == "__main__":
    main()
