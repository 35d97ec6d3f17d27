"""Float64 restatements of the sample path in front of the modems, from the PRODUCT's own plan (cubicsdr_amd/libcsdr_design.so: the taps,
phase words and tables the library uploads): NCO mix, decimating and interpolating msresamp cascades, firpfbch and firpfbch2.  Each evaluates
a whole stream at once -- the filters are time invariant, blocks matter only for the per-block counts (bit-exact in the parity tests), the
oscillator's phase is theta0 + n dtheta mod 2^32 over the stream -- and each comes with its absolute-value twin (|taps| applied to |x|), the
scale the rounding bounds of tests/util.py are stated in.  numpy only; used by tests/test_gpu_sample_path_exact.py and tests/test_host_design.py."""
import ctypes as C
import math

import numpy as np

_D = None


def design():
    global _D
    if _D is None:
        from cubicsdr_amd import build
        _D = C.CDLL(build.build_design(verbose=False))
        _D.csdr_design_nco_word.restype = C.c_uint
    return _D


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def msresamp_plan(rate, As=60.0):
    """csdr_design_msresamp(rate): dict(interp, S, step, m [S] and h1 [S][2 m] by design index (0 = the lowest-rate stage), arms [256][14])"""
    interp, S, pinned = C.c_int(), C.c_int(), C.c_int()
    step, ra = C.c_uint(), C.c_float()
    m = (C.c_int * 16)()
    h1, arms = np.zeros(16 * 20, np.float32), np.zeros(256 * 14, np.float32)
    rc = design().csdr_design_msresamp(C.c_float(rate), C.c_float(As), C.byref(interp), C.byref(S), C.byref(step), C.byref(ra), m, _ptr(h1), _ptr(arms), C.byref(pinned))
    assert rc == 0
    ms = list(m)[:S.value]
    return dict(interp=interp.value, S=S.value, step=step.value, m=ms, h1=[h1.reshape(16, 20)[i, :2 * ms[i]].astype(np.float64) for i in range(S.value)],
                arms=arms.reshape(256, 14).astype(np.float64))


def nco_word(shift, rate):
    """the oscillator's phase increment for a demodulator `shift` Hz off its channel's centre at channel rate `rate` (csdr_bank_execute)"""
    return int(design().csdr_design_nco_word(C.c_float(float(np.float32((2.0 * math.pi) * (float(abs(shift)) / float(rate)))))))


def sine_table():
    t = np.zeros(1024, np.float32)
    design().csdr_design_sine_table(_ptr(t))
    return t.astype(np.float64)


def channelizer_taps(M, oversampled=False):
    """taps[c][n] (commutator position, frames back) of firpfbch / firpfbch2 as uploaded, float64 [M, 8]"""
    t = np.zeros(M * 8, np.float32)
    (design().csdr_design_channelizer2 if oversampled else design().csdr_design_channelizer)(C.c_uint(M), C.c_uint(4), C.c_float(60.0), _ptr(t))
    return t.reshape(M, 8).astype(np.float64)


# ----------------------------------------------------------------------------------------------- front-end
def mix(x, shift, rate, theta0=0):
    """x[n] (c -+ j s)(theta0 + n dtheta): table oscillator without interpolation, mixing down for shift > 0 and up for shift < 0"""
    x = np.asarray(x, np.complex128)
    if shift == 0:
        return x
    tab = sine_table()
    th = (np.uint64(theta0) + np.arange(x.size, dtype=np.uint64) * np.uint64(nco_word(shift, rate))) & np.uint64(0xFFFFFFFF)
    idx = (((th + np.uint64(1 << 21)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)).astype(np.int64)
    s, c = tab[idx & 1023], tab[(idx + 256) & 1023]
    return x * (c - 1j * s) if shift > 0 else x * (c + 1j * s)


def _arm_stage(z, plan, absolute):
    """the arbitrary stage over the whole stream: output j at phase j step, arm (P mod 2^24) >> 16 over the 14 inputs ending at P >> 24"""
    arms = np.abs(plan["arms"]) if absolute else plan["arms"]
    step = plan["step"]
    J = (int(z.size) * (1 << 24) + step - 1) // step
    P = np.arange(J, dtype=np.int64) * step
    zp = np.concatenate([np.zeros(13, z.dtype), z])
    out = np.zeros(J, z.dtype)
    k, arm = P >> 24, (P & 0xFFFFFF) >> 16
    for t in range(14):
        out += arms[arm, t] * zp[k + t]
    return out


def decimate(z, plan, absolute=False):
    """msresamp, rate < 1: S half-band /2 stages (y[k] = x[2 (k - m) + 1] + sum_j h1[j] x[2 (k - j)], the highest-rate stage first), 2^-S, the
    arbitrary stage.  absolute = True: the absolute-value cascade of a non-negative stream"""
    assert not plan["interp"]
    S = plan["S"]
    for g in range(S - 1, -1, -1):
        m = plan["m"][g]
        h1 = np.abs(plan["h1"][g]) if absolute else plan["h1"][g]
        n = z.size // 2
        evp = np.concatenate([np.zeros(2 * m - 1, z.dtype), z[0:2 * n:2]])
        odp = np.concatenate([np.zeros(m, z.dtype), z[1:2 * n:2]])
        y = odp[:n].copy()
        for j in range(2 * m):
            y += h1[j] * evp[2 * m - 1 - j:2 * m - 1 - j + n]
        z = y
    return _arm_stage(z / (1 << S), plan, absolute)


def interpolate(z, plan, absolute=False):
    """msresamp, rate > 1: the arbitrary stage, then S x2 stages (w'[2 q] = w[q - m], w'[2 q + 1] = sum_j h1[j] w[q - j]) in design order"""
    assert plan["interp"]
    w = _arm_stage(z, plan, absolute)
    for s in range(plan["S"]):
        m = plan["m"][s]
        h1 = np.abs(plan["h1"][s]) if absolute else plan["h1"][s]
        wp = np.concatenate([np.zeros(2 * m, w.dtype), w])
        out = np.empty(2 * w.size, w.dtype)
        out[0::2] = wp[m:m + w.size]
        acc = np.zeros(w.size, w.dtype)
        for j in range(2 * m):
            acc += h1[j] * wp[2 * m - j:2 * m - j + w.size]
        out[1::2] = acc
        w = out
    return w


def frontend(row, shift, rate, plan):
    """(y, A): the exact front-end output of a channel row (the float32 samples the kernel read) and its absolute-value cascade"""
    run = interpolate if plan["interp"] else decimate
    return run(mix(row, shift, rate), plan), run(np.abs(np.asarray(row, np.complex128)), plan, absolute=True)


# ----------------------------------------------------------------------------------------------- channelizers
def firpfbch(x, M, oversampled=False):
    """(X, v, a), each [frames, M]: the exact rows of firpfbch (frames hop by M) or firpfbch2 (hop M / 2, design.hpp: channelizer2_taps / _post),
    the commutator sums in front of the transform and their absolute-value twins, from a stream that starts behind an all-zero history"""
    taps = channelizer_taps(M, oversampled)
    x = np.asarray(x, np.complex128)
    hop = M // 2 if oversampled else M
    F = x.size // hop
    # frame t, position c, n frames back: x[t M + c - n M]  |  x[(t - 1) M / 2 + c - n M]
    xp = np.concatenate([np.zeros(8 * M, np.complex128), x])
    base = 8 * M + (np.arange(F) * hop - (hop if oversampled else 0))[:, None] + np.arange(M)[None, :]
    v = np.zeros((F, M), np.complex128)
    a = np.zeros((F, M))
    for n in range(8):
        seg = xp[base - n * M]
        v += taps[:, n][None, :] * seg
        a += np.abs(taps[:, n])[None, :] * np.abs(seg)
    X = np.fft.fft(v, axis=1)
    if oversampled:
        k = np.arange(M)
        post = np.exp(-2j * np.pi * k / M) / M
        X = X * post[None, :]
        X[1::2, 1::2] *= -1.0
        v, a = v / M, a / M
    return X, v, a
