"""Thin Python host objects over the C ABI (tests, bench, smoke).  Names follow the reference objects whose
arithmetic each handle replaces: SDRPostThread (src/sdr/SDRPostThread.cpp), DemodulatorInstance's Pre/Demod
threads + Modem (src/demod/, src/modules/modem/), SpectrumVisualProcessor and FFTDataDistributor (src/process/), WaterfallPanel (src/panel/).

Inputs may be numpy complex64 arrays (host, staged by the library) or torch CUDA tensors (HBM resident, passed by
device pointer).  No computation happens in Python; without the HIP library or a GPU everything raises.
"""
import ctypes as C

import numpy as np

from . import hip as H


def _as_iq_arg(iq):
    """-> (pointer, is_dev, n_complex, keepalive)"""
    if isinstance(iq, np.ndarray):
        if iq.dtype == np.float32 and iq.ndim == 2 and iq.shape[1] == 2:          # interleaved (re, im) pairs
            iq = np.ascontiguousarray(iq).view(np.complex64).reshape(-1)
        a = np.ascontiguousarray(iq, dtype=np.complex64)
        return a.ctypes.data_as(C.c_void_p), 0, a.size, a
    if isinstance(iq, DevicePointer):
        return C.c_void_p(iq.ptr), 1, iq.n, iq
    # torch tensor on the GPU: complex64 [n] or float32 [n, 2] / [2n]
    import torch
    if not isinstance(iq, torch.Tensor) or not iq.is_cuda:
        raise TypeError("iq must be a numpy array or a CUDA torch tensor")
    t = iq.contiguous()
    if t.dtype == torch.complex64:
        n = t.numel()
    elif t.dtype == torch.float32:
        n = t.numel() // 2
    else:
        raise TypeError("iq tensor must be complex64 or float32")
    return C.c_void_p(t.data_ptr()), 1, n, t


class Context:
    """device + streams (csdr_ctx): one internal HIP stream per pipeline stage; `stream` is the boundary stream the
    caller's own GPU work is ordered on: None creates a private one; a raw hipStream_t handle (e.g. torch's
    `torch.cuda.Stream.cuda_stream`) chains with the caller's work -- 0 is the device's null stream (torch's default
    stream), passed on as CSDR_STREAM_NULL."""

    def __init__(self, device=0, stream=None):
        self._l = H.lib()
        self.h = C.c_void_p()
        if stream is None:
            arg = None
        elif int(stream) == 0:
            arg = C.c_void_p(-1)                                  # CSDR_STREAM_NULL
        else:
            arg = C.c_void_p(int(stream))
        H.check(self._l.csdr_ctx_create(device, arg, C.byref(self.h)))

    @property
    def owns_stream(self):
        """True when the boundary stream is private to the library (nothing the caller enqueues is ordered against it)"""
        return bool(self._l.csdr_ctx_owns_stream(self.h))

    def synchronize(self):
        H.check(self._l.csdr_ctx_synchronize(self.h))

    def join(self):
        """the boundary stream waits for everything enqueued on the internal stage streams so far"""
        H.check(self._l.csdr_ctx_join(self.h))

    def timer_start(self):
        H.check(self._l.csdr_ctx_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        H.check(self._l.csdr_ctx_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def profile_enable(self, on=True):
        """True / 1: time every launch; an integer P > 1: every P-th launch of each kernel; False: off"""
        H.check(self._l.csdr_ctx_profile_enable(self.h, int(on)))

    def profile(self):
        """-> {kernel name: (total_ms of the bracketed launches, bracketed launches, ALL launches)} since profile_enable(...)"""
        out = {}
        for i in range(self._l.csdr_ctx_profile_num_kernels()):
            ms, n, seen = C.c_double(), C.c_int64(), C.c_int64()
            H.check(self._l.csdr_ctx_profile_fetch(self.h, i, C.byref(ms), C.byref(n)))
            H.check(self._l.csdr_ctx_profile_launches(self.h, i, C.byref(seen)))
            if n.value:
                out[self._l.csdr_ctx_profile_kernel_name(i).decode()] = (ms.value, n.value, seen.value)
        return out

    def profile_range(self):
        """-> {kernel name: (shortest, longest) bracketed launch in ms} since profile_enable(...)"""
        out = {}
        for i in range(self._l.csdr_ctx_profile_num_kernels()):
            lo, hi = C.c_double(), C.c_double()
            H.check(self._l.csdr_ctx_profile_range(self.h, i, C.byref(lo), C.byref(hi)))
            if hi.value > 0.0:
                out[self._l.csdr_ctx_profile_kernel_name(i).decode()] = (lo.value, hi.value)
        return out

    def close(self):
        if self.h:
            self._l.csdr_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SDRPost:
    """SDRPostThread's arithmetic (csdr_post): DC blocker (1 channel) or firpfbch analyzer (M channels)."""

    def __init__(self, ctx, sample_rate, num_channels, max_block_len, max_blocks=1, oversampled=False):
        """oversampled=True: SDRPostPFBCH2 (firpfbch2, channels at twice the channel spacing)"""
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_post_create(ctx.h, C.byref(self.h)))
        mode = H.CSDR_POST_SINGLE if num_channels == 1 else (H.CSDR_POST_PFBCH2 if oversampled else H.CSDR_POST_PFBCH)
        self.hop = 1 if num_channels == 1 else (num_channels // 2 if oversampled else num_channels)
        H.check(self._l.csdr_post_configure(self.h, int(sample_rate), int(num_channels), mode, int(max_block_len), int(max_blocks)))
        self.num_channels = num_channels
        self.sample_rate = sample_rate

    def set_active_channels(self, channels=None):
        if channels is None:
            H.check(self._l.csdr_post_set_active_channels(self.h, None, 0))
        else:
            a = np.ascontiguousarray(channels, dtype=np.int32)
            H.check(self._l.csdr_post_set_active_channels(self.h, a.ctypes.data_as(C.c_void_p), a.size))

    def set_row_order(self, channels=None):
        """time-slab producers: rows stored in this channel order (csdr_post_set_row_order); None = row is the channel"""
        a = np.ascontiguousarray(channels if channels is not None else [], dtype=np.int32)
        H.check(self._l.csdr_post_set_row_order(self.h, a.ctypes.data_as(C.c_void_p) if a.size else None, a.size))

    def execute(self, iq, n_blocks, block_len, frequency):
        p, is_dev, n, keep = _as_iq_arg(iq)
        if n < n_blocks * block_len:
            raise ValueError("iq holds %d samples, need %d" % (n, n_blocks * block_len))
        H.check(self._l.csdr_post_execute(self.h, p, is_dev, int(n_blocks), int(block_len), int(frequency)))
        self._keep = keep
        self._last = (n_blocks, block_len)

    # ---- time-slab sharding (csdr_hip.h: producer / owner halves; parallel.SlabStream drives them).  `buf` arguments are DEVICE
    # buffers: torch tensors on the context's GPU (float32 [.., 2] or complex64); numpy arrays only when the library in use runs its kernels on the host (the test suite has such a build)
    @staticmethod
    def _dev_ptr(buf):
        if isinstance(buf, np.ndarray):
            return buf.ctypes.data_as(C.c_void_p)
        return C.c_void_p(buf.data_ptr())

    @property
    def kernel_name(self):
        """which kernel the channel count maps to (csdr_post_kernel_name)"""
        return self._l.csdr_post_kernel_name(self.h).decode()

    @property
    def history_length(self):
        return self._l.csdr_post_history_length(self.h)

    def set_history(self, tail, n_samples):
        H.check(self._l.csdr_post_set_history(self.h, self._dev_ptr(tail), int(n_samples)))
        self._keep_hist = tail

    def set_dc_blocker(self, enabled):
        H.check(self._l.csdr_post_set_dc_blocker(self.h, 1 if enabled else 0))

    def export_rows(self, channels, dst, dst_stride):
        a = np.ascontiguousarray(channels, dtype=np.int32)
        H.check(self._l.csdr_post_export_rows(self.h, a.ctypes.data_as(C.c_void_p), a.size, self._dev_ptr(dst), int(dst_stride)))

    def import_begin(self, n_blocks, block_len, frequency):
        H.check(self._l.csdr_post_import_begin(self.h, int(n_blocks), int(block_len), int(frequency)))
        self._last = (n_blocks, block_len)

    def import_rows(self, channels, src, src_stride, frame0, n_frames):
        a = np.ascontiguousarray(channels, dtype=np.int32)
        H.check(self._l.csdr_post_import_rows(self.h, a.ctypes.data_as(C.c_void_p), a.size, self._dev_ptr(src), int(src_stride), int(frame0), int(n_frames)))

    def import_commit(self):
        H.check(self._l.csdr_post_import_commit(self.h))

    @property
    def channel_bandwidth(self):
        return self._l.csdr_post_channel_bandwidth(self.h)

    @property
    def channel_rate(self):
        return self._l.csdr_post_channel_rate(self.h)

    def channel_center(self, i):
        return self._l.csdr_post_channel_center(self.h, i)

    def channel_at(self, f):
        return self._l.csdr_post_channel_at(self.h, int(f))

    def read_channel(self, ch):
        nb, bl = self._last
        cap = nb * (bl // self.hop)
        out = np.empty(cap, np.complex64)
        n = C.c_int()
        H.check(self._l.csdr_post_read_channel(self.h, int(ch), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value]

    def close(self):
        if self.h:
            self._l.csdr_post_destroy(self.h)
            self.h = C.c_void_p()


def digital_params(kind, cons=0, bps=0, sps=0, bw=0.0, fdelay=0):
    k = H.DIGITAL_BY_NAME[kind] if isinstance(kind, str) else int(kind)
    return H.DigitalParams(k, int(cons), int(bps), int(sps), float(bw), int(fdelay))


def digital_run(ctx, kind, iq, sample_rate, state=None, cons=0, bps=0, sps=0, bw=0.0):
    """csdr_digital_run: the decision kernel alone on `iq` (complex64) at the modem rate `sample_rate`, through one modem object whose state is
    `state` (an H.DigitalState, updated in place; None = a fresh object).  Returns (symbols uint32, evm after the last sample, state)."""
    d = digital_params(kind, cons, bps, sps, bw)
    x = np.ascontiguousarray(iq, dtype=np.complex64)
    st = state if state is not None else H.DigitalState()
    out = np.empty(max(1, x.size + st.n_carry), np.uint32)
    n, evm = C.c_int(), C.c_float()
    H.check(H.lib().csdr_digital_run(ctx.h, C.byref(d), int(sample_rate), x.ctypes.data_as(C.c_void_p), int(x.size), C.byref(st),
                                     out.ctypes.data_as(C.c_void_p), int(out.size), C.byref(n), C.byref(evm)))
    return out[:n.value].copy(), evm.value, st


def gmsk_run(ctx, iq, state=None, sps=0, fdelay=0, ebf=0.0):
    """csdr_gmsk_run: the GMSK kernels alone on `iq` (complex64, whole symbols of `sps` samples), len(iq) / sps consecutive gmskdem_demodulate
    calls of one object; 0 = the reference default (sps 4, fdelay 3, ebf 0.3).  `state`: (H.GmskState, history float32[2 sps fdelay]) from an
    earlier call, None = a fresh object.  Returns (symbols uint32, soft float32: the filter output each was decided from, state)."""
    d = digital_params("GMSK", sps=sps, bw=ebf, fdelay=fdelay)
    k, m = d.sps or 4, d.fdelay or 3
    x = np.ascontiguousarray(iq, dtype=np.complex64)
    st, hist = state if state is not None else (H.GmskState(), np.zeros(max(1, 2 * k * m), np.float32))
    if not isinstance(hist, np.ndarray) or hist.dtype != np.float32 or not hist.flags.c_contiguous or hist.size != max(1, 2 * k * m):
        raise ValueError("gmsk_run: the state's history must be float32[2 sps fdelay] = %d for these settings" % (2 * k * m))
    n_sym = x.size // k
    sym, soft = np.empty(max(1, n_sym), np.uint32), np.empty(max(1, n_sym), np.float32)
    n = C.c_int()
    H.check(H.lib().csdr_gmsk_run(ctx.h, C.byref(d), x.ctypes.data_as(C.c_void_p), int(x.size), C.byref(st), hist.ctypes.data_as(C.c_void_p),
                                  sym.ctypes.data_as(C.c_void_p), soft.ctypes.data_as(C.c_void_p), int(sym.size), C.byref(n)))
    return sym[:n.value].copy(), soft[:n.value].copy(), (st, hist)


def design_rings(points, sensitivity=0.0):
    """csdr_design_rings: the ring description (H.Constellation, rule RINGS) of an APSK constellation from its points by symbol (complex64,
    what liquid's modemcf_modulate returns); raises CsdrError for anything that is not concentric, evenly spaced rings.  Host only."""
    x = np.ascontiguousarray(points, dtype=np.complex64)
    c = H.Constellation()
    H.check(H.lib().csdr_design_rings(x.ctypes.data_as(C.c_void_p), int(x.size), C.byref(c)))
    c.sensitivity = float(sensitivity)
    return c


def nearest_table(points, sensitivity=0.0, quadrant=False):
    """an H.Constellation decided by the first nearest point (liquid's arb demodulator; V.29) from its points by symbol; quadrant = True: behind
    a fold into the first quadrant (liquid's SQAM demodulators)"""
    x = np.ascontiguousarray(points, dtype=np.complex64)
    if x.size > H.CSDR_TABLE_MAX_POINTS:
        raise ValueError("a constellation holds at most %d points" % H.CSDR_TABLE_MAX_POINTS)
    c = H.Constellation()
    c.rule, c.n_points, c.sensitivity = H.CSDR_TABLE_QUADRANT if quadrant else H.CSDR_TABLE_NEAREST, int(x.size), float(sensitivity)
    C.memmove(c.points, x.ctypes.data, x.nbytes)
    return c


def table_run(ctx, table, iq, state=None):
    """csdr_table_run: the table kernel alone on `iq` (complex64) through one modem object whose state is `state` (an H.DigitalState, updated in
    place; None = a fresh object).  Returns (symbols uint32, evm after the last sample, state)."""
    x = np.ascontiguousarray(iq, dtype=np.complex64)
    st = state if state is not None else H.DigitalState()
    out = np.empty(max(1, x.size), np.uint32)
    n, evm = C.c_int(), C.c_float()
    H.check(H.lib().csdr_table_run(ctx.h, C.byref(table), x.ctypes.data_as(C.c_void_p), int(x.size), C.byref(st),
                                   out.ctypes.data_as(C.c_void_p), int(out.size), C.byref(n), C.byref(evm)))
    return out[:n.value].copy(), evm.value, st


class DemodBank:
    """N demodulator slots (csdr_bank); one slot = one DemodulatorInstance's Pre + Demod thread arithmetic."""

    def __init__(self, ctx, max_demods, max_blocks=1):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        self.max_blocks = max_blocks
        H.check(self._l.csdr_bank_create(ctx.h, int(max_demods), int(max_blocks), C.byref(self.h)))

    def configure(self, slot, post, modem, bandwidth, frequency, audio_sample_rate=48000, modem_arg=0):
        """modem_arg: FM stereo de-emphasis in microseconds (0: the reference's default 75, negative: none)"""
        m = H.MODEM_BY_NAME[modem] if isinstance(modem, str) else int(modem)
        p = H.DemodParams(m, int(bandwidth), int(audio_sample_rate), int(modem_arg), int(frequency))
        H.check(self._l.csdr_bank_configure_slot(self.h, int(slot), C.byref(p), post.h))

    def configure_digital(self, slot, post, kind, bandwidth, frequency, cons=0, bps=0, sps=0, bw=0.0, audio_sample_rate=48000, fdelay=0, ebf=None):
        """a digital-lab modem (kind: "PSK", "DPSK", "ASK", "QAM", "BPSK", "QPSK", "OOK", "FSK", "GMSK" or CSDR_DIGITAL_*); 0 = the reference
        default.  GMSK: sps = samples per symbol, fdelay, ebf (= bw)"""
        k = H.DIGITAL_BY_NAME[kind] if isinstance(kind, str) else int(kind)
        p = H.DemodParams(H.CSDR_MODEM_DIGITAL, int(bandwidth), int(audio_sample_rate), 0, int(frequency))
        d = digital_params(k, cons, bps, sps, bw if ebf is None else ebf, fdelay)
        H.check(self._l.csdr_bank_configure_digital_slot(self.h, int(slot), C.byref(p), C.byref(d), post.h))

    def configure_table(self, slot, post, tables, bandwidth, frequency, audio_sample_rate=48000):
        """a table-driven digital modem (APSK, SQAM, V.29, liquid's arb family): `tables` is one H.Constellation or a sequence of up to eight with
        distinct sizes (design_rings / nearest_table), the first active; set_digital_cons(slot, n_points) switches among them"""
        tabs = [tables] if isinstance(tables, H.Constellation) else list(tables)
        arr = (H.Constellation * max(1, len(tabs)))(*tabs)
        p = H.DemodParams(H.CSDR_MODEM_DIGITAL, int(bandwidth), int(audio_sample_rate), 0, int(frequency))
        H.check(self._l.csdr_bank_configure_table_slot(self.h, int(slot), C.byref(p), arr, len(tabs), post.h))

    def set_digital_cons(self, slot, cons):
        """writeSetting("cons"): the next execute decides with constellation `cons`; every constellation keeps its own state"""
        H.check(self._l.csdr_bank_set_digital_cons(self.h, int(slot), int(cons)))

    def digital_results(self, slot):
        arr = (H.DigitalResult * self.max_blocks)()
        n = C.c_int()
        H.check(self._l.csdr_bank_fetch_digital_results(self.h, int(slot), arr, self.max_blocks, C.byref(n)))
        return [arr[i] for i in range(n.value)]

    def symbols(self, slot, cap=1 << 22):
        out = np.empty(cap, np.uint32)
        n = C.c_int()
        H.check(self._l.csdr_bank_fetch_symbols(self.h, int(slot), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def set_frequency(self, slot, f):
        H.check(self._l.csdr_bank_set_frequency(self.h, int(slot), int(f)))

    def set_active(self, slot, active):
        H.check(self._l.csdr_bank_set_active(self.h, int(slot), int(bool(active))))

    def execute(self, post):
        H.check(self._l.csdr_bank_execute(self.h, post.h))

    def results(self, slot):
        arr = (H.BlockResult * self.max_blocks)()
        n = C.c_int()
        H.check(self._l.csdr_bank_fetch_results(self.h, int(slot), arr, self.max_blocks, C.byref(n)))
        return [arr[i] for i in range(n.value)]

    def audio(self, slot, cap=1 << 22):
        out = np.empty(cap, np.float32)
        n = C.c_int()
        H.check(self._l.csdr_bank_fetch_audio(self.h, int(slot), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def iq(self, slot, cap=1 << 22):
        out = np.empty(cap, np.complex64)
        n = C.c_int()
        H.check(self._l.csdr_bank_fetch_iq(self.h, int(slot), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def demod_output(self, slot, cap=2048):
        """scaled demodulator output of the last block (ModemAnalog::getDemodOutputData), at most 2048 samples"""
        out = np.empty(cap, np.float32)
        n = C.c_int()
        H.check(self._l.csdr_bank_fetch_demod_output(self.h, int(slot), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def set_fms_pilot(self, slot, b15=None, a15=None):
        """replace (or, with None, restore) the pilot band-pass sections of an FM-stereo slot"""
        if b15 is None:
            H.check(self._l.csdr_bank_set_fms_pilot(self.h, int(slot), None, None))
            return
        b = np.ascontiguousarray(b15, dtype=np.float32); a = np.ascontiguousarray(a15, dtype=np.float32)
        assert b.size == 15 and a.size == 15
        H.check(self._l.csdr_bank_set_fms_pilot(self.h, int(slot), b.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p)))

    def fms_stage(self, slot, which, cap=1 << 22):
        """FM stereo intermediates of the last batch: which = 0 pilot oscillator phase words (uint32), 1 stereo-difference stream (float32)"""
        out = np.empty(cap, dtype=np.uint32 if which == 0 else np.float32)
        n = C.c_int(0)
        H.check(self._l.csdr_bank_fetch_fms_stage(self.h, int(slot), int(which), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def pcm16(self, slot, cap=1 << 22):
        """the slot's audio of the last execute as 16-bit PCM, every block scaled by its own peak (AudioFileWAV.cpp:133-157), converted on the device"""
        out = np.empty(cap, np.int16)
        n = C.c_int()
        H.check(self._l.csdr_bank_fetch_pcm16(self.h, int(slot), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return out[:n.value].copy()

    def scope_frame(self, slot):
        """the audio-scope tap of the last block as a device-resident frame (H.ScopeFrame; n == 0: nothing to show)"""
        f = H.ScopeFrame()
        H.check(self._l.csdr_bank_scope_frame(self.h, int(slot), C.byref(f)))
        return f

    def total_audio(self):
        n = C.c_int64()
        H.check(self._l.csdr_bank_total_audio(self.h, C.byref(n)))
        return n.value

    def close(self):
        if self.h:
            self._l.csdr_bank_destroy(self.h)
            self.h = C.c_void_p()


class SpectrumProcessor:
    """SpectrumVisualProcessor's arithmetic (csdr_spec), full-span view."""

    def __init__(self, ctx, fft_size, max_frames=1):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        self.fft_size = fft_size
        H.check(self._l.csdr_spec_create(ctx.h, C.byref(self.h)))
        H.check(self._l.csdr_spec_setup(self.h, int(fft_size), int(max_frames)))

    def set_average_rate(self, r):
        H.check(self._l.csdr_spec_set_average_rate(self.h, float(r)))

    def set_scale_factor(self, f):
        H.check(self._l.csdr_spec_set_scale_factor(self.h, float(f)))

    def set_peak_hold(self, enabled):
        H.check(self._l.csdr_spec_set_peak_hold(self.h, int(bool(enabled))))

    def set_hide_dc(self, enabled, center_freq=None, bandwidth=None, input_freq=None):
        H.check(self._l.csdr_spec_set_hide_dc(self.h, int(bool(enabled))))
        if center_freq is not None:
            H.check(self._l.csdr_spec_set_center_frequency(self.h, int(center_freq)))
        if bandwidth is not None:
            H.check(self._l.csdr_spec_set_bandwidth(self.h, int(bandwidth)))
        if input_freq is not None:
            H.check(self._l.csdr_spec_set_input_frequency(self.h, int(input_freq)))

    def set_view(self, on, center_freq=None, bandwidth=None):
        H.check(self._l.csdr_spec_set_view(self.h, int(bool(on))))
        if center_freq is not None:
            H.check(self._l.csdr_spec_set_center_frequency(self.h, int(center_freq)))
        if bandwidth is not None:
            H.check(self._l.csdr_spec_set_bandwidth(self.h, int(bandwidth)))

    def process_view_input(self, iq, frequency, sample_rate):
        """one process() input in zoomed-view mode; returns the number of frames it produced (0 or 1)"""
        H.check(self._l.csdr_spec_set_input_frequency(self.h, int(frequency)))
        H.check(self._l.csdr_spec_set_input_rate(self.h, int(sample_rate)))
        p, is_dev, n, keep = _as_iq_arg(iq)
        H.check(self._l.csdr_spec_process(self.h, p, is_dev, 1, int(n), H.CSDR_SPEC_FIRST_FRAME))
        self._keep = keep
        return self._l.csdr_spec_frames(self.h)

    @property
    def desired_input_size(self):
        return self._l.csdr_spec_desired_input_size(self.h)

    def fetch_hold(self, frame):
        """spectrum_hold_points of a frame, or None when it carries none"""
        pts = np.empty(2 * self.fft_size, np.float32)
        n = C.c_int()
        H.check(self._l.csdr_spec_fetch_hold(self.h, int(frame), pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(n)))
        return pts if n.value else None

    def process(self, iq, n_blocks, block_len, contiguous=False, lines=False):
        """frames per `mode`: first 2*fftSize samples of every block (default), every non-overlapping frame
        (contiguous=True), or one overlapped frame per short block (lines=True: FFTDataDistributor's fftSize-sample lines)"""
        p, is_dev, n, keep = _as_iq_arg(iq)
        if n < n_blocks * block_len:
            raise ValueError("iq holds %d samples, need %d" % (n, n_blocks * block_len))
        mode = H.CSDR_SPEC_LINES if lines else (H.CSDR_SPEC_CONTIGUOUS if contiguous else H.CSDR_SPEC_FIRST_FRAME)
        H.check(self._l.csdr_spec_process(self.h, p, is_dev, int(n_blocks), int(block_len), mode))
        self._keep = keep
        return self._l.csdr_spec_frames(self.h)

    def fetch(self, frame):
        pts = np.empty(2 * self.fft_size, np.float32)
        ce, fl = C.c_double(), C.c_double()
        H.check(self._l.csdr_spec_fetch(self.h, int(frame), pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(ce), C.byref(fl)))
        return pts, ce.value, fl.value

    def fft_only(self, x):
        a = np.ascontiguousarray(x, dtype=np.complex64)
        assert a.size == 2 * self.fft_size
        out = np.empty(a.size, np.complex64)
        H.check(self._l.csdr_spec_fft_only(self.h, a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
        return out

    def close(self):
        if self.h:
            self._l.csdr_spec_destroy(self.h)
            self.h = C.c_void_p()


class SpectrumBank:
    """N independent SpectrumVisualProcessors of one fft_size (csdr_specbank): one per demodulator, all slots and all inputs of a call in one launch;
    state and points stay in HBM."""

    def __init__(self, ctx, fft_size, max_slots, max_frames=1):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_specbank_create(ctx.h, C.byref(self.h)))
        self.setup(fft_size, max_slots, max_frames)

    def setup(self, fft_size, max_slots, max_frames=1):
        H.check(self._l.csdr_specbank_setup(self.h, int(fft_size), int(max_slots), int(max_frames)))
        self.fft_size, self.max_slots, self.max_frames = int(fft_size), int(max_slots), int(max_frames)

    def set_average_rate(self, r):
        H.check(self._l.csdr_specbank_set_average_rate(self.h, float(r)))

    def set_scale_factor(self, f):
        H.check(self._l.csdr_specbank_set_scale_factor(self.h, float(f)))

    def set_peak_hold(self, enabled):
        H.check(self._l.csdr_specbank_set_peak_hold(self.h, int(bool(enabled))))

    def get_peak_hold(self):
        return bool(self._l.csdr_specbank_get_peak_hold(self.h))

    def reset_slot(self, slot):
        H.check(self._l.csdr_specbank_reset_slot(self.h, int(slot)))

    def try_process(self, items):
        """items: [(slot, iq)] with iq a numpy array, a CUDA torch tensor, a DevicePointer, or None / empty for no input -> the return code"""
        arr = (H.SpecBankItem * max(len(items), 1))()
        keep = []
        for k, (slot, iq) in enumerate(items):
            arr[k].slot = int(slot)
            if iq is None or (isinstance(iq, np.ndarray) and iq.size == 0):
                arr[k].n, arr[k].iq, arr[k].is_dev = 0, None, 0
                continue
            p, is_dev, n, ka = _as_iq_arg(iq)
            arr[k].n, arr[k].iq, arr[k].is_dev = int(n), p.value, int(is_dev)
            keep.append(ka)
        rc = self._l.csdr_specbank_process(self.h, arr, len(items))
        self._keep = keep
        return rc

    def process(self, items):
        H.check(self.try_process(items))

    def process_bank(self, bank):
        """every block of the bank's last execute, for every active slot the object has room for: one call, no host synchronisation"""
        H.check(self._l.csdr_specbank_process_bank(self.h, bank.h))

    def frames(self, slot):
        return self._l.csdr_specbank_frames(self.h, int(slot))

    def fetch(self, slot, frame):
        pts = np.empty(2 * self.fft_size, np.float32)
        ce, fl = C.c_double(), C.c_double()
        H.check(self._l.csdr_specbank_fetch(self.h, int(slot), int(frame), pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(ce), C.byref(fl)))
        return pts, ce.value, fl.value

    def fetch_hold(self, slot, frame):
        """spectrum_hold_points of a frame, or None when it carries none"""
        pts = np.empty(2 * self.fft_size, np.float32)
        n = C.c_int()
        H.check(self._l.csdr_specbank_fetch_hold(self.h, int(slot), int(frame), pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(n)))
        return pts if n.value else None

    def device_points(self, slot):
        """(device pointer, frames): the [frames, fft_size] y values of the slot's last call; the context's boundary stream waits for them"""
        p, n = C.c_void_p(), C.c_int()
        H.check(self._l.csdr_specbank_device_points(self.h, int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def close(self):
        if self.h:
            self._l.csdr_specbank_destroy(self.h)
            self.h = C.c_void_p()


class ViewBank:
    """N independent SpectrumVisualProcessors in zoomed view, of one fft_size (csdr_viewbank): the reference's demodulator spectrum -- the channel
    row shifted, resampled to rate / 2^k and shown over `bandwidth` -- for every demodulator at once; all slots and all inputs of a call in one
    launch, state and points stay in HBM."""

    def __init__(self, ctx, fft_size, max_slots, max_frames=1, max_samples=65536):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_viewbank_create(ctx.h, C.byref(self.h)))
        self.setup(fft_size, max_slots, max_frames, max_samples)

    def setup(self, fft_size, max_slots, max_frames=1, max_samples=65536):
        H.check(self._l.csdr_viewbank_setup(self.h, int(fft_size), int(max_slots), int(max_frames), int(max_samples)))
        self.fft_size, self.max_slots, self.max_frames, self.max_samples = int(fft_size), int(max_slots), int(max_frames), int(max_samples)

    def set_average_rate(self, r):
        H.check(self._l.csdr_viewbank_set_average_rate(self.h, float(r)))

    def set_scale_factor(self, f):
        H.check(self._l.csdr_viewbank_set_scale_factor(self.h, float(f)))

    def set_peak_hold(self, enabled):
        H.check(self._l.csdr_viewbank_set_peak_hold(self.h, int(bool(enabled))))

    def get_peak_hold(self):
        return bool(self._l.csdr_viewbank_get_peak_hold(self.h))

    def set_hide_dc(self, enabled):
        H.check(self._l.csdr_viewbank_set_hide_dc(self.h, int(bool(enabled))))

    def try_set_view(self, slot, center_freq, bandwidth):
        return self._l.csdr_viewbank_set_view(self.h, int(slot), int(center_freq), int(bandwidth))

    def set_view(self, slot, center_freq, bandwidth):
        H.check(self.try_set_view(slot, center_freq, bandwidth))

    def reset_slot(self, slot):
        H.check(self._l.csdr_viewbank_reset_slot(self.h, int(slot)))

    def try_process(self, items):
        """items: [(slot, iq, frequency, sample_rate)] with iq a numpy array, a CUDA torch tensor, a DevicePointer, or None / empty for no
        input -> the return code"""
        arr = (H.ViewBankItem * max(len(items), 1))()
        keep = []
        for k, (slot, iq, frequency, sample_rate) in enumerate(items):
            arr[k].slot, arr[k].frequency, arr[k].sample_rate = int(slot), int(frequency), int(sample_rate)
            if iq is None or (isinstance(iq, np.ndarray) and iq.size == 0):
                arr[k].n, arr[k].iq, arr[k].is_dev = 0, None, 0
                continue
            p, is_dev, n, ka = _as_iq_arg(iq)
            arr[k].n, arr[k].iq, arr[k].is_dev = int(n), p.value, int(is_dev)
            keep.append(ka)
        rc = self._l.csdr_viewbank_process(self.h, arr, len(items))
        self._keep = keep
        return rc

    def process(self, items):
        H.check(self.try_process(items))

    def try_process_post(self, post, slots, channels):
        s = np.ascontiguousarray(slots, dtype=np.int32)
        c = np.ascontiguousarray(channels, dtype=np.int32)
        if s.size != c.size:
            raise ValueError("%d slots, %d channels" % (s.size, c.size))
        return self._l.csdr_viewbank_process_post(self.h, post.h, s.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), s.size)

    def process_post(self, post, slots, channels):
        """slot slots[i] gets every block of row channels[i] of the post's last execute, where it lies in HBM: one call, no host synchronisation"""
        H.check(self.try_process_post(post, slots, channels))

    def frames(self, slot):
        return self._l.csdr_viewbank_frames(self.h, int(slot))

    def fetch(self, slot, frame):
        pts = np.empty(2 * self.fft_size, np.float32)
        ce, fl = C.c_double(), C.c_double()
        H.check(self._l.csdr_viewbank_fetch(self.h, int(slot), int(frame), pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(ce), C.byref(fl)))
        return pts, ce.value, fl.value

    def fetch_hold(self, slot, frame):
        """spectrum_hold_points of a frame, or None when it carries none"""
        pts = np.empty(2 * self.fft_size, np.float32)
        n = C.c_int()
        H.check(self._l.csdr_viewbank_fetch_hold(self.h, int(slot), int(frame), pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(n)))
        return pts if n.value else None

    def device_points(self, slot):
        """(device pointer, frames): the [frames, fft_size] y values of the slot's last call; the context's boundary stream waits for them"""
        p, n = C.c_void_p(), C.c_int()
        H.check(self._l.csdr_viewbank_device_points(self.h, int(slot), C.byref(p), C.byref(n)))
        return p.value, n.value

    def slot_info(self, slot):
        """-> dict of the slot's integers behind its last item (csdr_viewbank_slot_state)"""
        st = H.ViewBankSlotState()
        H.check(self._l.csdr_viewbank_slot_info(self.h, int(slot), C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in H.ViewBankSlotState._fields_}

    def fetch_last(self, slot):
        """the slot's fftLastData: 2 * fft_size complex samples"""
        out = np.empty(2 * self.fft_size, np.complex64)
        H.check(self._l.csdr_viewbank_fetch_last(self.h, int(slot), out.ctypes.data_as(C.c_void_p), 2 * out.size))
        return out

    def close(self):
        if self.h:
            self._l.csdr_viewbank_destroy(self.h)
            self.h = C.c_void_p()


def design_gradient(stops, length=256):
    """Gradient::generate(length) for colour stops [[r, g, b], ...] (host only) -> (r, g, b) float32 arrays"""
    a = np.ascontiguousarray(stops, dtype=np.float32).reshape(-1, 3)
    r, g, b = (np.empty(max(int(length), 0), np.float32) for _ in range(3))
    H.check(H.lib().csdr_design_gradient(a.ctypes.data_as(C.c_void_p), int(a.shape[0]), int(length), r.ctypes.data_as(C.c_void_p),
                                         g.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
    return r, g, b


VIEW_MODES = {"linear": H.WF_VIEW_LINEAR, "peak": H.WF_VIEW_PEAK}
VIEW_TAP = np.dtype([("first", np.int32), ("count", np.int32), ("frac", np.float32), ("half", np.int32)])


def _view_mode(mode):
    return VIEW_MODES[mode] if isinstance(mode, str) else int(mode)


def design_view_columns(fft_size, width, mode="linear"):
    """the column taps of a `width` pixel wide view of a waterfall of fft_size points (host only) -> structured array [width] of VIEW_TAP"""
    t = np.zeros(max(int(width), 0), VIEW_TAP)
    H.check(H.lib().csdr_design_view_columns(int(fft_size), int(width), _view_mode(mode), t.ctypes.data_as(C.c_void_p)))
    return t


def design_view_rows(lines, height, mode="linear"):
    """the row taps of a `height` pixel high view of a ring of `lines` lines (host only) -> structured array [height] of VIEW_TAP"""
    t = np.zeros(max(int(height), 0), VIEW_TAP)
    H.check(H.lib().csdr_design_view_rows(int(lines), int(height), _view_mode(mode), t.ctypes.data_as(C.c_void_p)))
    return t


class Waterfall:
    """WaterfallPanel's arithmetic (csdr_waterfall): spectrum lines quantised to bytes, two ring textures, the themed RGBA picture."""

    def __init__(self, ctx, fft_size, lines, max_pending=256):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_waterfall_create(ctx.h, C.byref(self.h)))
        self.setup(fft_size, lines, max_pending)

    def setup(self, fft_size, lines, max_pending=256):
        H.check(self._l.csdr_waterfall_setup(self.h, int(fft_size), int(lines), int(max_pending)))
        self.fft_size, self.half, self.lines = int(fft_size), int(fft_size) // 2, int(lines)

    def set_gradient(self, stops):
        a = np.ascontiguousarray(stops, dtype=np.float32).reshape(-1, 3)
        H.check(self._l.csdr_waterfall_set_gradient(self.h, a.ctypes.data_as(C.c_void_p), int(a.shape[0])))

    def step(self, points=None, n_lines=None):
        """points: None (repeat the previous points n_lines times), a numpy float32 array [n_lines, n] / [n], or a CUDA torch tensor of that
        shape; returns the number of lines taken"""
        taken = C.c_int()
        if points is None:
            H.check(self._l.csdr_waterfall_step(self.h, None, 0, 0, int(1 if n_lines is None else n_lines), C.byref(taken)))
            return taken.value
        if isinstance(points, np.ndarray):
            a = np.ascontiguousarray(points, dtype=np.float32)
            ptr, is_dev, shape = a.ctypes.data_as(C.c_void_p), 0, a.shape
        else:
            a = points.contiguous()
            ptr, is_dev, shape = C.c_void_p(a.data_ptr()), 1, tuple(a.shape)
        rows = 1 if len(shape) == 1 else int(shape[0])
        H.check(self._l.csdr_waterfall_step(self.h, ptr, is_dev, int(shape[-1]), rows, C.byref(taken)))
        self._keep = a
        return taken.value

    def step_spec(self, spec, frame0=0, n_frames=1):
        taken = C.c_int()
        H.check(self._l.csdr_waterfall_step_spec(self.h, spec.h, int(frame0), int(n_frames), C.byref(taken)))
        return taken.value

    def update(self):
        H.check(self._l.csdr_waterfall_update(self.h))

    @property
    def lines_buffered(self):
        return self._l.csdr_waterfall_lines_buffered(self.h)

    def offset(self, half=0):
        return self._l.csdr_waterfall_offset(self.h, int(half))

    def fetch_index(self, half):
        out = np.empty((self.lines, self.half), np.uint8)
        H.check(self._l.csdr_waterfall_fetch_index(self.h, int(half), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def fetch_rgba(self, first_row=0, n_rows=None, fetch=True):
        """the picture [n_rows, 2 * half, 4] uint8; fetch=False renders it and leaves it on the device (device_rgba)"""
        n_rows = self.lines - first_row if n_rows is None else n_rows
        if not fetch:
            H.check(self._l.csdr_waterfall_fetch_rgba(self.h, int(first_row), int(n_rows), None, 0))
            return None
        out = np.empty((n_rows, 2 * self.half, 4), np.uint8)
        H.check(self._l.csdr_waterfall_fetch_rgba(self.h, int(first_row), int(n_rows), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def device_rgba(self):
        p = C.c_void_p()
        H.check(self._l.csdr_waterfall_device_rgba(self.h, C.byref(p)))
        return p.value

    def view(self, width, height, mode="linear", fetch=True):
        """the ring scaled to a viewport, [height, width, 4] uint8: mode "linear" is the reference's GL_LINEAR picture, "peak" the maximum over
        every pixel's footprint; fetch=False renders it and leaves it on the device (device_view)"""
        if not fetch:
            H.check(self._l.csdr_waterfall_render_view(self.h, int(width), int(height), _view_mode(mode), None, 0))
            return None
        out = np.empty((max(int(height), 0), max(int(width), 0), 4), np.uint8)
        H.check(self._l.csdr_waterfall_render_view(self.h, int(width), int(height), _view_mode(mode), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def device_view(self):
        """(device pointer, width, height) of the last rendered view; the context's boundary stream waits for it"""
        p, w, h = C.c_void_p(), C.c_int(), C.c_int()
        H.check(self._l.csdr_waterfall_device_view(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def close(self):
        if self.h:
            self._l.csdr_waterfall_destroy(self.h)
            self.h = C.c_void_p()


class WaterfallBank:
    """N independent WaterfallPanels of one fft_size and one `lines` (csdr_wfbank): one per demodulator; every slot of a step, an update or a
    render in one launch; lines, textures and pictures stay in HBM."""

    def __init__(self, ctx, fft_size, lines, max_slots, max_pending=256):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_wfbank_create(ctx.h, C.byref(self.h)))
        self.setup(fft_size, lines, max_slots, max_pending)

    def setup(self, fft_size, lines, max_slots, max_pending=256):
        H.check(self._l.csdr_wfbank_setup(self.h, int(fft_size), int(lines), int(max_slots), int(max_pending)))
        self.fft_size, self.half, self.lines, self.max_slots = int(fft_size), int(fft_size) // 2, int(lines), int(max_slots)

    def set_gradient(self, stops):
        a = np.ascontiguousarray(stops, dtype=np.float32).reshape(-1, 3)
        H.check(self._l.csdr_wfbank_set_gradient(self.h, a.ctypes.data_as(C.c_void_p), int(a.shape[0])))

    def reset_slot(self, slot):
        H.check(self._l.csdr_wfbank_reset_slot(self.h, int(slot)))

    def try_step(self, items):
        """items: [(slot, points)] or [(slot, None, n_lines)] -- points None (repeat the slot's previous points n_lines times), a numpy float32
        array [n_lines, n] / [n], or a CUDA torch tensor of that shape -> (return code, [lines taken per item])"""
        arr = (H.WfBankItem * max(len(items), 1))()
        taken = (C.c_int * max(len(items), 1))()
        keep = []
        for k, it in enumerate(items):
            slot, points = it[0], it[1]
            arr[k].slot = int(slot)
            if points is None:
                arr[k].n_floats_per_line, arr[k].points, arr[k].is_dev, arr[k].n_lines = 0, None, 0, int(it[2]) if len(it) > 2 else 1
                continue
            if isinstance(points, np.ndarray):
                a = np.ascontiguousarray(points, dtype=np.float32)
                ptr, is_dev, shape = a.ctypes.data, 0, a.shape
            else:
                a = points.contiguous()
                ptr, is_dev, shape = a.data_ptr(), 1, tuple(a.shape)
            arr[k].n_floats_per_line, arr[k].points, arr[k].is_dev = int(shape[-1]), ptr, is_dev
            arr[k].n_lines = 1 if len(shape) == 1 else int(shape[0])
            keep.append(a)
        rc = self._l.csdr_wfbank_step(self.h, arr, len(items), taken)
        self._keep = keep
        return rc, [taken[k] for k in range(len(items))]

    def step(self, items):
        rc, taken = self.try_step(items)
        H.check(rc)
        return taken

    def step_from(self, specbank):
        """the frames of every slot of the SpectrumBank's last process, straight from its points in HBM: one call, no host synchronisation ->
        the lines taken over all slots"""
        total = C.c_int()
        H.check(self._l.csdr_wfbank_step_specbank(self.h, specbank.h, C.byref(total)))
        return total.value

    def update(self):
        H.check(self._l.csdr_wfbank_update(self.h))

    def lines_buffered(self, slot):
        return self._l.csdr_wfbank_lines_buffered(self.h, int(slot))

    def offset(self, slot, half=0):
        return self._l.csdr_wfbank_offset(self.h, int(slot), int(half))

    def fetch_index(self, slot, half):
        out = np.empty((self.lines, self.half), np.uint8)
        H.check(self._l.csdr_wfbank_fetch_index(self.h, int(slot), int(half), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def view(self, slots, width, height, mode="linear", atlas_cols=1, fetch=True):
        """the listed slots' rings scaled to width x height tiles of one picture, [tile rows * height, atlas_cols * width, 4] uint8; slots: a list, or
        an int n for slots 0 .. n - 1; fetch=False renders it and leaves it on the device (device_view)"""
        if isinstance(slots, (int, np.integer)):
            n, lst = int(slots), None
        else:
            n = len(slots)
            lst = (C.c_int * max(n, 1))(*[int(s) for s in slots])
        if not fetch:
            H.check(self._l.csdr_wfbank_render(self.h, lst, n, int(width), int(height), _view_mode(mode), int(atlas_cols), None, 0))
            return None
        tile_rows = -(-n // max(int(atlas_cols), 1))
        out = np.empty((max(tile_rows * int(height), 0), max(int(atlas_cols) * int(width), 0), 4), np.uint8)
        H.check(self._l.csdr_wfbank_render(self.h, lst, n, int(width), int(height), _view_mode(mode), int(atlas_cols), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def device_view(self):
        """(device pointer, width, height) of the last rendered picture in pixels; the context's boundary stream waits for it"""
        p, w, h = C.c_void_p(), C.c_int(), C.c_int()
        H.check(self._l.csdr_wfbank_device_view(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def close(self):
        if self.h:
            self._l.csdr_wfbank_destroy(self.h)
            self.h = C.c_void_p()


TRACE_KINDS = {"spectrum": H.TRACE_SPECTRUM, "y": H.TRACE_SCOPE_Y, "2y": H.TRACE_SCOPE_2Y, "xy": H.TRACE_SCOPE_XY}


def _trace_kind(kind):
    return TRACE_KINDS[kind] if isinstance(kind, str) else int(kind)


def design_trace_envelope(points, width, height, kind="spectrum", hold=None, layout=0, n=None):
    """the lit intervals of a polyline's columns in a width x height tile (host only; csdr_hip.h, "Trace bank", item 8) -> (lo, hi), int32 [2, width]:
    row 0 the line (2Y: the upper sub-panel), row 1 the hold (2Y: the lower sub-panel), -1 where a column is unlit"""
    a = np.ascontiguousarray(points, dtype=np.float32).ravel()
    h = None if hold is None else np.ascontiguousarray(hold, dtype=np.float32).ravel()
    n = a.size // (1 + int(layout)) if n is None else int(n)
    lo, hi = (np.empty((2, max(int(width), 0)), np.int32) for _ in range(2))
    H.check(H.lib().csdr_design_trace_envelope(a.ctypes.data_as(C.c_void_p) if a.size else None, None if h is None else h.ctypes.data_as(C.c_void_p), n,
                                               int(layout), _trace_kind(kind), int(width), int(height), lo.ctypes.data_as(C.c_void_p), hi.ctypes.data_as(C.c_void_p)))
    return lo, hi


class TraceBank:
    """The spectrum, hold and scope lines of any number of items as tiles of one RGBA8 atlas with WaterfallBank.view's geometry (csdr_tracebank):
    one launch for all line kinds, one for all XY items; points are read where they lie in HBM."""

    def __init__(self, ctx, max_items=256, max_points=1 << 16):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_tracebank_create(ctx.h, C.byref(self.h)))
        self.setup(max_items, max_points)

    def setup(self, max_items, max_points):
        H.check(self._l.csdr_tracebank_setup(self.h, int(max_items), int(max_points)))
        self.max_items, self.max_points = int(max_items), int(max_points)

    def set_colors(self, bg=None, line=None, hold=None, axis_major=None, axis_minor=None):
        """bg: 4 bytes RGBA; the others 3 bytes RGB; None leaves a colour as it is"""
        arg = [None if c is None else (C.c_uint8 * k)(*[int(v) for v in c]) for c, k in ((bg, 4), (line, 3), (hold, 3), (axis_major, 3), (axis_minor, 3))]
        H.check(self._l.csdr_tracebank_set_colors(self.h, *arg))

    def try_render(self, items, width, height, atlas_cols=1, out=None, fetch=True):
        """items: dicts with kind ("spectrum" | "y" | "2y" | "xy" or a CSDR_TRACE_* value), points and optionally hold (each a numpy float32 array,
        a DevicePointer or None), layout (0 | 1), n (default: what the points hold); or None for an empty tile -> (return code, picture or None)"""
        arr = (H.TraceItem * max(len(items), 1))()
        keep = []

        def place(p):
            if p is None:
                return None, 0, 0
            if isinstance(p, DevicePointer):
                keep.append(p)
                return p.ptr, 1, p.n
            a = np.ascontiguousarray(p, dtype=np.float32).ravel()
            keep.append(a)
            return (a.ctypes.data if a.size else None), 0, a.size
        for k, it in enumerate(items):
            if it is None:
                continue
            kind, layout = _trace_kind(it.get("kind", "spectrum")), int(it.get("layout", 0))
            ptr, dev, floats = place(it.get("points"))
            hptr, hdev, _ = place(it.get("hold"))
            n = it.get("n")
            if n is None:
                n = floats if kind == H.TRACE_SCOPE_XY else floats // (1 + (layout & 1))
            arr[k].points, arr[k].hold, arr[k].n, arr[k].layout, arr[k].kind = ptr, hptr, int(n), layout, kind
            arr[k].is_dev = (H.TRACE_DEV_POINTS if dev else 0) | (H.TRACE_DEV_HOLD if hdev else 0)
        n_items, cols = len(items), int(atlas_cols)
        if not fetch:
            return self._l.csdr_tracebank_render(self.h, arr, n_items, int(width), int(height), cols, None, 0), None
        if out is None:
            out = np.empty((max(-(-n_items // max(cols, 1)) * int(height), 0), max(cols * int(width), 0), 4), np.uint8)
        rc = self._l.csdr_tracebank_render(self.h, arr, n_items, int(width), int(height), cols, out.ctypes.data_as(C.c_void_p), out.nbytes)
        return rc, out

    def render(self, items, width, height, atlas_cols=1, out=None, fetch=True):
        """-> [tile rows * height, atlas_cols * width, 4] uint8; fetch=False renders it and leaves it on the device (device_view)"""
        rc, pic = self.try_render(items, width, height, atlas_cols, out, fetch)
        H.check(rc)
        return pic

    def render_spectra(self, bank, slots, width, height, frame=-1, hold=True, atlas_cols=1, fetch=True):
        """frame `frame` (-1: the last one) of the listed slots of a SpectrumBank's or a ViewBank's last process, one tile per slot.  The points are
        read where they lie in HBM (bank.device_points) and never cross the link.  The HOLD points come as a host item through bank.fetch_hold: no
        existing call hands them out in HBM.  A slot without frames gives an empty tile."""
        items = []
        for s in slots:
            p, frames = bank.device_points(s)
            f = frames - 1 if frame < 0 else int(frame)
            if frames <= 0 or f >= frames:
                items.append(None)
                continue
            hp = bank.fetch_hold(s, f) if hold else None
            items.append(dict(kind="spectrum", points=DevicePointer(p + 4 * f * bank.fft_size, bank.fft_size), n=bank.fft_size,
                              hold=None if hp is None else hp[1::2].copy()))
        return self.render(items, width, height, atlas_cols, fetch=fetch)

    def render_scopes(self, scope_bank, slots, width, height, frame=-1, atlas_cols=1, fetch=True):
        """the waveform item of frame `frame` (-1: the last one) of the listed slots of a ScopeBank's last process, one tile per slot, read where it
        lies in HBM (scope_bank.device_points).  The kind comes from each frame's mode (Y, 2Y, XY); mode and length are only returned by
        ScopeBank.fetch, so that call is made per slot for them.  A slot without a waveform gives an empty tile."""
        items = []
        for s in slots:
            p, frames, stride = scope_bank.device_points(s, False)
            f = frames - 1 if frame < 0 else int(frame)
            it = scope_bank.fetch(s, f, False) if 0 <= f < frames else None
            if it is None:
                items.append(None)
                continue
            nf, kind = it["points"].size, H.TRACE_SCOPE_Y + int(it["mode"])
            xy = kind == H.TRACE_SCOPE_XY
            items.append(dict(kind=kind, points=DevicePointer(p + 4 * f * stride, nf), n=nf if xy else nf // 2, layout=0 if xy else 1))
        return self.render(items, width, height, atlas_cols, fetch=fetch)

    def device_view(self):
        """(device pointer, width, height) of the last rendered picture in pixels; the context's boundary stream waits for it"""
        p, w, h = C.c_void_p(), C.c_int(), C.c_int()
        H.check(self._l.csdr_tracebank_device_view(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def close(self):
        if self.h:
            self._l.csdr_tracebank_destroy(self.h)
            self.h = C.c_void_p()


def design_density_cover(points, width, height, n, frames=1, kind="spectrum", layout=0, stride_floats=None):
    """how many of the frames pass through every pixel of a width x height tile (host only; csdr_hip.h, "Density bank", item 1) -> uint32 [height, width]"""
    a = np.ascontiguousarray(points, dtype=np.float32).ravel()
    stride = int(n) * (1 + int(layout)) if stride_floats is None else int(stride_floats)
    cover = np.empty((max(int(height), 0), max(int(width), 0)), np.uint32)
    H.check(H.lib().csdr_design_density_cover(a.ctypes.data_as(C.c_void_p) if a.size else None, int(n), int(layout), stride, int(frames), _trace_kind(kind),
                                              int(width), int(height), cover.ctypes.data_as(C.c_void_p)))
    return cover


def density_palette(stops, alpha=255):
    """a 256-entry RGBA palette for DensityBank.set_palette from colour stops [[r, g, b], ...] in 0 .. 1 (csdr_design_gradient) -> uint8 [256, 4]"""
    r, g, b = design_gradient(stops, 256)
    pal = np.empty((256, 4), np.uint8)
    for k, ch in enumerate((r, g, b)):
        pal[:, k] = np.clip(np.floor(ch.astype(np.float64) * 255.0 + 0.5), 0, 255).astype(np.uint8)
    pal[:, 3] = int(alpha)
    return pal


class DensityBank:
    """The persistence display (csdr_density): one uint32 hit grid per slot in HBM -- how often the trace passed through every pixel of a
    width x height tile -- stepped with ALL frames of its items in two launches and drawn through a palette as tiles of one RGBA8 atlas with
    WaterfallBank.view's geometry.  Points are read where they lie in HBM."""

    def __init__(self, ctx, width, height, max_slots=1, max_frames=1024, max_points=1 << 16):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_density_create(ctx.h, C.byref(self.h)))
        self.setup(width, height, max_slots, max_frames, max_points)

    def setup(self, width, height, max_slots, max_frames, max_points):
        H.check(self._l.csdr_density_setup(self.h, int(width), int(height), int(max_slots), int(max_frames), int(max_points)))
        self.width, self.height, self.max_slots, self.max_frames, self.max_points = int(width), int(height), int(max_slots), int(max_frames), int(max_points)

    def set_palette(self, rgba):
        """rgba: uint8 [256, 4]"""
        a = np.ascontiguousarray(rgba, dtype=np.uint8).reshape(256, 4)
        H.check(self._l.csdr_density_set_palette(self.h, a.ctypes.data_as(C.c_void_p)))

    def reset_slot(self, slot):
        H.check(self._l.csdr_density_reset_slot(self.h, int(slot)))

    def try_step(self, items):
        """items: dicts with slot, points (a numpy float32 array, a DevicePointer or None: decay only), n (default: what one frame of the points
        holds), frames (default 1), layout (0 | 1), kind ("spectrum" | "y"), stride_floats (default n * (1 + layout)), keep_q16 (default 65536),
        weight (default 1) -> return code"""
        arr = (H.DensityItem * max(len(items), 1))()
        keep = []
        for k, it in enumerate(items):
            layout, frames = int(it.get("layout", 0)), int(it.get("frames", 1))
            p = it.get("points")
            ptr, dev, floats = None, 0, 0
            if isinstance(p, DevicePointer):
                keep.append(p)
                ptr, dev, floats = p.ptr, 1, p.n
            elif p is not None:
                a = np.ascontiguousarray(p, dtype=np.float32).ravel()
                keep.append(a)
                ptr, floats = (a.ctypes.data if a.size else None), a.size
            n = it.get("n")
            if n is None:
                n = floats // max(frames, 1) // (1 + (layout & 1))
            stride = it.get("stride_floats")
            arr[k].points, arr[k].slot, arr[k].n, arr[k].frames, arr[k].layout = ptr, int(it["slot"]), int(n), frames, layout
            arr[k].stride_floats = int(n) * (1 + layout) if stride is None else int(stride)
            arr[k].kind, arr[k].is_dev = _trace_kind(it.get("kind", "spectrum")), dev
            arr[k].keep_q16, arr[k].weight = int(it.get("keep_q16", 65536)), int(it.get("weight", 1))
        return self._l.csdr_density_step(self.h, arr, len(items))

    def step(self, items):
        H.check(self.try_step(items))

    def step_spec(self, slot, spec, frame0=0, n_frames=None, keep_q16=65536, weight=1):
        """frames [frame0, frame0 + n_frames) (default: all from frame0) of a SpectrumProcessor's last process, hideDC as its fetch applies it"""
        if n_frames is None:
            n_frames = self._l.csdr_spec_frames(spec.h) - int(frame0)
        H.check(self._l.csdr_density_step_spec(self.h, int(slot), spec.h, int(frame0), int(n_frames), int(keep_q16), int(weight)))

    def step_specbank(self, bank, keep_q16=65536, weight=1):
        """slot s takes all frames of slot s of a SpectrumBank's last process"""
        H.check(self._l.csdr_density_step_specbank(self.h, bank.h, int(keep_q16), int(weight)))

    def step_views(self, viewbank, slots=None, keep_q16=65536, weight=1):
        """slot s takes all frames of slot s of a ViewBank's last process, read where they lie in HBM (viewbank.device_points).  A slot without frames
        only decays.  The caller synchronises this object (fetch, peak or a fetched render) before the view bank's next process."""
        items = []
        for s in (range(min(self.max_slots, viewbank.max_slots)) if slots is None else slots):
            p, frames = viewbank.device_points(s)
            pts = DevicePointer(p, frames * viewbank.fft_size) if frames > 0 else None
            items.append(dict(slot=s, points=pts, n=viewbank.fft_size, frames=max(frames, 0), keep_q16=keep_q16, weight=weight))
        self.step(items)

    def peak(self, slot):
        v = C.c_uint32()
        H.check(self._l.csdr_density_peak(self.h, int(slot), C.byref(v)))
        return v.value

    def fetch(self, slot):
        """-> the slot's counts, uint32 [height, width]"""
        out = np.empty((self.height, self.width), np.uint32)
        H.check(self._l.csdr_density_fetch(self.h, int(slot), out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def try_render(self, views, atlas_cols=1, out=None, fetch=True):
        """views: (slot, full) pairs or plain slots (full = 0: the slot's peak); slot -1: an all-zero tile -> (return code, picture or None)"""
        arr = (H.DensityView * max(len(views), 1))()
        for k, v in enumerate(views):
            arr[k].slot, arr[k].full = (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), 0)
        n, cols = len(views), int(atlas_cols)
        if not fetch:
            return self._l.csdr_density_render(self.h, arr, n, cols, None, 0), None
        if out is None:
            out = np.empty((max(-(-n // max(cols, 1)) * self.height, 0), max(cols * self.width, 0), 4), np.uint8)
        return self._l.csdr_density_render(self.h, arr, n, cols, out.ctypes.data_as(C.c_void_p), out.nbytes), out

    def render(self, views, atlas_cols=1, out=None, fetch=True):
        """-> [tile rows * height, atlas_cols * width, 4] uint8; fetch=False renders it and leaves it on the device (device_view)"""
        rc, pic = self.try_render(views, atlas_cols, out, fetch)
        H.check(rc)
        return pic

    def device_view(self):
        """(device pointer, width, height) of the last rendered picture in pixels; the context's boundary stream waits for it"""
        p, w, h = C.c_void_p(), C.c_int(), C.c_int()
        H.check(self._l.csdr_density_device_view(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def close(self):
        if self.h:
            self._l.csdr_density_destroy(self.h)
            self.h = C.c_void_p()


PRIM_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("rgba", "u1", (4,)), ("mode", "<i4"), ("mask_x", "<i4"), ("mask_y", "<i4")])
GLYPH_DTYPE = np.dtype([(k, "<i4") for k in ("id", "x", "y", "w", "h", "xoffset", "yoffset", "xadvance")])
OVL_MODES = {"over": H.OVL_OVER, "add": H.OVL_ADD, "copy": H.OVL_COPY}
_ALIGN_H = {"left": H.ALIGN_LEFT, "center": H.ALIGN_CENTER, "right": H.ALIGN_RIGHT}
_ALIGN_V = {"top": H.ALIGN_TOP, "center": H.ALIGN_CENTER, "bottom": H.ALIGN_BOTTOM}
_SIDEBANDS = {"both": H.SIDEBAND_BOTH, "usb": H.SIDEBAND_USB, "lsb": H.SIDEBAND_LSB}


def _named(table, v):
    return table[v] if isinstance(v, str) else int(v)


def overlay_prims(records=()):
    """csdr_overlay_prim records as one numpy array (PRIM_DTYPE): from (x, y, w, h, rgba, mode[, mask_x, mask_y]) tuples, or arrays to concatenate"""
    parts = []
    for r in records:
        if isinstance(r, np.ndarray):
            parts.append(r.astype(PRIM_DTYPE, copy=False).ravel())
            continue
        a = np.zeros(1, PRIM_DTYPE)
        a[0] = (r[0], r[1], r[2], r[3], tuple(r[4]), _named(OVL_MODES, r[5]), r[6] if len(r) > 6 else -1, r[7] if len(r) > 7 else 0)
        parts.append(a)
    return np.concatenate(parts) if parts else np.zeros(0, PRIM_DTYPE)


def _glyph_table(glyphs):
    g = np.ascontiguousarray(glyphs, dtype=GLYPH_DTYPE).ravel()
    return g, g.ctypes.data_as(C.POINTER(H.Glyph))


def design_freq_scale(freq, bandwidth, view_w, view_h, font_scale=1.0):
    """SpectrumPanel's frequency scale (host only; csdr_hip.h, "Overlay bank", a) -> dict(step_mhz, precision, tick_top, label_y, font_size,
    tick_rows, label_row, ticks=[dict(m, value, label, major, column)])"""
    sc, cap = H.FreqScale(), 64
    while True:
        ticks = (H.FreqTick * cap)()
        rc = H.lib().csdr_design_freq_scale(int(freq), int(bandwidth), int(view_w), int(view_h), float(font_scale), C.byref(sc), ticks, cap)
        if rc != -5:
            break
        cap = sc.n_ticks
    H.check(rc)
    out = {k: getattr(sc, k) for k in ("step_mhz", "precision", "tick_top", "label_y", "font_size", "tick_rows", "label_row")}
    out["ticks"] = [dict(m=t.m, value=t.value, label=t.label.decode(), major=bool(t.major), column=t.column) for t in ticks[:sc.n_ticks]]
    return out


def design_db_grid(floor, ceil):
    """SpectrumPanel's dB grid (host only; "Overlay bank", b) -> [dict(alpha, step, p=float64 array)] for each range that applies, in order"""
    ranges, n, p = (H.DbGridRange * 3)(), C.c_int(), (C.c_double * 256)()
    H.check(H.lib().csdr_design_db_grid(float(floor), float(ceil), ranges, C.byref(n), p, 256))
    return [dict(alpha=r.alpha, step=r.step, p=np.array(p[r.first:r.first + r.count], np.float64)) for r in ranges[:n.value]]


def design_db_labels(floor, ceil, fft_size, db_offset=0.0):
    """SpectrumPanel's two dB labels (host only; "Overlay bank", c) -> (ceil label, floor label)"""
    a, b = C.create_string_buffer(64), C.create_string_buffer(64)
    H.check(H.lib().csdr_design_db_labels(float(floor), float(ceil), int(fft_size), float(db_offset), a, b, 64))
    return a.value.decode(), b.value.decode()


def design_demod_marker(demod_freq, bandwidth, sideband, center_freq, srate, flags, view_w, view_h, rgb=(255, 255, 255)):
    """DrawDemodInfo's marker (host only; "Overlay bank", d) -> dict(ux, ofs_left, ofs_right, label_v, narrow, halign, label_x, label_y, prefix, prims)"""
    m, prims, n = H.DemodMarker(), np.zeros(4, PRIM_DTYPE), C.c_int()
    H.check(H.lib().csdr_design_demod_marker(int(demod_freq), int(bandwidth), _named(_SIDEBANDS, sideband), int(center_freq), int(srate), int(flags), int(view_w),
                                             int(view_h), (C.c_uint8 * 3)(*[int(v) for v in rgb]), C.byref(m), prims.ctypes.data_as(C.POINTER(H.OverlayPrim)), C.byref(n)))
    out = {k: getattr(m, k) for k in ("ux", "ofs_left", "ofs_right", "label_v", "narrow", "halign", "label_x", "label_y")}
    out["narrow"], out["prefix"], out["prims"] = bool(m.narrow), m.prefix.decode(), prims[:n.value].copy()
    return out


def design_text(glyphs, line_height, text, x, y, halign="left", valign="top", rgba=(255, 255, 255, 255), mode="over"):
    """one string as masked primitives (host only; "Overlay bank", e) -> PRIM_DTYPE array.  glyphs: GLYPH_DTYPE records (parse_bmfont)"""
    g, gp = _glyph_table(glyphs)
    raw = text.encode("latin-1", "replace") if isinstance(text, str) else bytes(text)
    out, n = np.zeros(max(len(raw), 1), PRIM_DTYPE), C.c_int()
    H.check(H.lib().csdr_design_text(gp, g.size, int(line_height), raw, int(x), int(y), _named(_ALIGN_H, halign), _named(_ALIGN_V, valign),
                                     (C.c_uint8 * 4)(*[int(v) for v in rgba]), _named(OVL_MODES, mode), out.ctypes.data_as(C.POINTER(H.OverlayPrim)), out.size, C.byref(n)))
    return out[:n.value].copy()


def parse_bmfont(text):
    """the text form of an AngelCode .fnt -> dict(glyphs=GLYPH_DTYPE array, line_height, base, scale_w, scale_h, pages={id: file}).  The page images
    are not decoded: the coverage plane OverlayBank.set_font takes is the caller's to produce from them."""
    import shlex
    glyphs, info = [], dict(line_height=0, base=0, scale_w=0, scale_h=0, pages={})
    for ln in text.splitlines():
        words = shlex.split(ln)
        if not words:
            continue
        kv = dict(w.split("=", 1) for w in words[1:] if "=" in w)
        if words[0] == "common":
            info.update(line_height=int(kv.get("lineHeight", 0)), base=int(kv.get("base", 0)), scale_w=int(kv.get("scaleW", 0)), scale_h=int(kv.get("scaleH", 0)))
        elif words[0] == "page":
            info["pages"][int(kv.get("id", 0))] = kv.get("file", "")
        elif words[0] == "char":
            glyphs.append(tuple(int(kv.get(k, 0)) for k in ("id", "x", "y", "width", "height", "xoffset", "yoffset", "xadvance")))
    info["glyphs"] = np.array(glyphs, GLYPH_DTYPE) if glyphs else np.zeros(0, GLYPH_DTYPE)
    return info


def spectrum_annotations(width, height, freq, bandwidth, floor, ceil, fft_size, glyphs, line_height, markers=(), db_offset=0.0, font_scale=1.0,
                         freq_line=(255, 255, 255), text=(255, 255, 255)):
    """One tile's primitive list (PRIM_DTYPE) in the order grid, ticks, MHz labels, dB labels, markers, for a tile that shows `bandwidth` Hz around
    `freq` between the levels floor and ceil: csdr_hip.h, "Overlay bank", a - e, put together.  The grid rows are CSDR_OVL_ADD in 0.12 grey; a tick
    fills rows [0, tick_rows) in freq_line (4 columns, major) or 0.65 of it (1 column); a MHz label is centred on (column, label_row) in `text`; the
    ceil label is right-aligned at column min(88 font_scale, width) against the top edge, the floor label against the bottom edge (the reference's
    two 88 x 14 panels, SpectrumPanel.cpp:282-302, without their grounds).  markers: dicts with freq, bandwidth, and optionally sideband, flags,
    rgb, label; each gives design_demod_marker's primitives and its label in white at alpha 0.8."""
    W, Hh = int(width), int(height)
    out = []
    for rng in design_db_grid(floor, ceil):
        a = int(rng["alpha"] * 255 + 0.5)
        for p in rng["p"]:
            if 0.0 <= p <= 1.0:
                row = int(min(max(np.floor((1.0 - (2.0 * p - 1.0)) * 0.5 * Hh), 0), Hh))
                if row < Hh:
                    out.append((0, row, W, 1, (31, 31, 31, a), H.OVL_ADD))
    sc = design_freq_scale(freq, bandwidth, W, Hh, font_scale)
    minor = tuple(int(c * 0.65 + 0.5) for c in freq_line)
    for t in sc["ticks"]:
        k = 4 if t["major"] else 1
        out.append((t["column"] - k // 2, 0, k, sc["tick_rows"], tuple(freq_line if t["major"] else minor) + (255,), H.OVL_OVER))
    for t in sc["ticks"]:
        out.append(design_text(glyphs, line_height, t["label"], t["column"], sc["label_row"], "center", "center", tuple(text) + (255,)))
    hi, lo = design_db_labels(floor, ceil, fft_size, db_offset)
    xr = min(int(88 * font_scale), W)
    out.append(design_text(glyphs, line_height, hi, xr, 0, "right", "top", tuple(text) + (255,)))
    out.append(design_text(glyphs, line_height, lo, xr, Hh, "right", "bottom", tuple(text) + (255,)))
    for mk in markers:
        m = design_demod_marker(mk["freq"], mk["bandwidth"], mk.get("sideband", "both"), freq, bandwidth, mk.get("flags", 0), W, Hh, mk.get("rgb", (255, 255, 255)))
        out.append(m["prims"])
        out.append(design_text(glyphs, line_height, m["prefix"] + mk.get("label", ""), m["label_x"], m["label_y"], m["halign"], "center", (255, 255, 255, 204)))
    return overlay_prims(out)


class OverlayBank:
    """Ordered primitive lists -- grid rows, ticks, marker bands, glyphs -- composited onto the tiles of an atlas with WaterfallBank.view's geometry
    in one launch (csdr_overlay).  The base picture is a host array, a DevicePointer to what a device_view returned, or nothing."""

    def __init__(self, ctx, max_tiles=256, max_prims=1 << 16):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_overlay_create(ctx.h, C.byref(self.h)))
        self.setup(max_tiles, max_prims)

    def setup(self, max_tiles, max_prims):
        H.check(self._l.csdr_overlay_setup(self.h, int(max_tiles), int(max_prims)))
        self.max_tiles, self.max_prims = int(max_tiles), int(max_prims)

    def set_font(self, plane):
        """plane: [font_h, font_w] uint8 coverage bytes, or None to remove the font"""
        if plane is None:
            H.check(self._l.csdr_overlay_set_font(self.h, None, 0, 0))
            return
        a = np.ascontiguousarray(plane, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError("a font plane is [height, width] bytes")
        H.check(self._l.csdr_overlay_set_font(self.h, a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]))

    @staticmethod
    def pack(lists):
        """one list per tile -> (prims, runs): the lists one behind the other"""
        arrs = [overlay_prims([l]) if isinstance(l, np.ndarray) else overlay_prims(l) for l in lists]
        at = np.concatenate([[0], np.cumsum([a.size for a in arrs])]).astype(int)
        return overlay_prims(arrs), [(int(at[k]), int(arrs[k].size)) for k in range(len(arrs))]

    def try_compose(self, prims, runs, width, height, atlas_cols=1, base=None, out=None, fetch=True):
        """prims: PRIM_DTYPE array (overlay_prims); runs: one (first, count) per tile; base: None, a uint8 array of the picture's size or a
        DevicePointer -> (return code, picture or None)"""
        pr = np.ascontiguousarray(prims, dtype=PRIM_DTYPE).ravel()
        tl = (H.OverlayTile * max(len(runs), 1))()
        for k, (first, count) in enumerate(runs):
            tl[k].first, tl[k].count = int(first), int(count)
        n_tiles, cols = len(runs), int(atlas_cols)
        if base is None:
            bp, bdev, keep = None, 0, None
        elif isinstance(base, DevicePointer):
            bp, bdev, keep = C.c_void_p(base.ptr), 1, base
        else:
            keep = np.ascontiguousarray(base, dtype=np.uint8)
            bp, bdev = keep.ctypes.data_as(C.c_void_p), 0
        pp = pr.ctypes.data_as(C.POINTER(H.OverlayPrim)) if pr.size else None
        if not fetch:
            return self._l.csdr_overlay_compose(self.h, bp, bdev, tl, n_tiles, pp, pr.size, int(width), int(height), cols, None, 0), None
        if out is None:
            out = np.empty((max(-(-n_tiles // max(cols, 1)) * int(height), 0), max(cols * int(width), 0), 4), np.uint8)
        rc = self._l.csdr_overlay_compose(self.h, bp, bdev, tl, n_tiles, pp, pr.size, int(width), int(height), cols, out.ctypes.data_as(C.c_void_p), out.nbytes)
        return rc, out

    def compose(self, prims, runs, width, height, atlas_cols=1, base=None, out=None, fetch=True):
        """-> [tile rows * height, atlas_cols * width, 4] uint8; fetch=False composes it and leaves it on the device (device_view)"""
        rc, pic = self.try_compose(prims, runs, width, height, atlas_cols, base, out, fetch)
        H.check(rc)
        return pic

    def device_view(self):
        """(device pointer, width, height) of the last composed picture in pixels; the context's boundary stream waits for it"""
        p, w, h = C.c_void_p(), C.c_int(), C.c_int()
        H.check(self._l.csdr_overlay_device_view(self.h, C.byref(p), C.byref(w), C.byref(h)))
        return p.value, w.value, h.value

    def close(self):
        if self.h:
            self._l.csdr_overlay_destroy(self.h)
            self.h = C.c_void_p()


class Distributor:
    """FFTDataDistributor's line cutting (csdr_distrib): the waterfall feed, cut where the block lies in HBM."""

    def __init__(self, ctx, max_lines=256, fft_size=None, lines_per_second=None):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_distrib_create(ctx.h, int(max_lines), C.byref(self.h)))
        if fft_size is not None:
            self.set_fft_size(fft_size)
        if lines_per_second is not None:
            self.set_lines_per_second(lines_per_second)

    def set_fft_size(self, n):
        H.check(self._l.csdr_distrib_set_fft_size(self.h, int(n)))

    def set_lines_per_second(self, lps):
        H.check(self._l.csdr_distrib_set_lines_per_second(self.h, int(lps)))

    def try_push(self, iq, frequency, sample_rate, n_samples=None):
        """one popped input; iq: numpy complex64 (host), a CUDA torch tensor or a DevicePointer -> (return code, lines emitted)"""
        p, is_dev, n, keep = _as_iq_arg(iq)
        n_lines = C.c_int()
        rc = self._l.csdr_distrib_push(self.h, p, is_dev, int(n if n_samples is None else n_samples), int(frequency), int(sample_rate), C.byref(n_lines))
        if rc == 0:
            self._keep = (keep, getattr(self, "_keep", (None,))[0])      # the block may still be read until the distributor's stream has passed it
        return rc, n_lines.value

    def push(self, iq, frequency, sample_rate):
        rc, n_lines = self.try_push(iq, frequency, sample_rate)
        H.check(rc)
        return n_lines

    @property
    def state(self):
        st = H.DistribState()
        H.check(self._l.csdr_distrib_get_state(self.h, C.byref(st)))
        return st

    def lines(self):
        """the last push's batch where it lies: (DevicePointer over n_lines * line_len samples, n_lines, line_len)"""
        p, n, ln = C.c_void_p(), C.c_int(), C.c_int()
        H.check(self._l.csdr_distrib_lines(self.h, C.byref(p), C.byref(n), C.byref(ln)))
        return DevicePointer(p.value or 0, n.value * ln.value), n.value, ln.value

    def fetch_lines(self):
        """the last push's lines -> complex64 [n_lines, line_len]"""
        st = self.state
        out = np.empty((st.n_lines, st.line_len), np.complex64)
        n = C.c_int()
        H.check(self._l.csdr_distrib_fetch_lines(self.h, out.ctypes.data_as(C.c_void_p), 2 * out.size, C.byref(n)))
        return out[:n.value]

    def fetch_buffered(self):
        """the carried samples -> complex64 [bufferedItems]"""
        out = np.empty(max(1, int(self.state.buffered_items)), np.complex64)
        n = C.c_int()
        H.check(self._l.csdr_distrib_fetch_buffered(self.h, out.ctypes.data_as(C.c_void_p), 2 * out.size, C.byref(n)))
        return out[:n.value]

    def process_into(self, spec):
        """csdr_spec_process_distrib: the last push's lines through `spec` (a SpectrumProcessor), HBM to HBM; returns the lines it was given"""
        H.check(self._l.csdr_spec_process_distrib(spec.h, self.h))
        return int(self.state.n_lines)

    def close(self):
        if self.h:
            self._l.csdr_distrib_destroy(self.h)
            self.h = C.c_void_p()


class ScopeProcessor:
    """ScopeVisualProcessor's arithmetic (csdr_scope): waveform normalisation + audio spectrum of AudioThreadInput frames."""

    def __init__(self, ctx, fft_size=1024, max_frames=8, max_samples=8192):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_scope_create(ctx.h, C.byref(self.h)))
        H.check(self._l.csdr_scope_setup(self.h, int(fft_size), int(max_frames), int(max_samples)))

    def set_enabled(self, scope=True, spectrum=True):
        H.check(self._l.csdr_scope_set_enabled(self.h, int(scope), int(spectrum)))

    def process(self, frames):
        """frames: list of dicts {data (numpy float32), channels, type, sample_rate, input_rate} (host frames), or of H.ScopeFrame
        structures whose data lies in HBM (DemodBank.scope_frame)"""
        n = len(frames)
        arr = (H.ScopeFrame * n)()
        keep = []
        dev = isinstance(frames[0], H.ScopeFrame)
        for i, f in enumerate(frames):
            if dev:
                arr[i] = f
            else:
                a = np.ascontiguousarray(f["data"], dtype=np.float32)
                keep.append(a)
                arr[i] = H.ScopeFrame(a.ctypes.data, None, a.size, int(f["channels"]), int(f.get("type", 0)), int(f["sample_rate"]), int(f["input_rate"]),
                                      int(f.get("layout", 0)), float(f.get("scale", 1.0)))
        H.check(self._l.csdr_scope_process(self.h, arr, n, 1 if dev else 0))

    def fetch(self, frame, spectrum):
        """-> dict like oracle.ref_modems.RefScopeCpp.push items, or None when that item was not produced"""
        pts = np.empty(1 << 15, np.float32)
        info = H.ScopeInfo()
        H.check(self._l.csdr_scope_fetch(self.h, int(frame), 1 if spectrum else 0, pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(info)))
        if info.n_floats == 0:
            return None
        return dict(points=pts[:info.n_floats].copy(), mode=info.mode, spectrum=bool(info.spectrum), channels=info.channels, input_rate=info.input_rate,
                    sample_rate=info.sample_rate, fft_size=info.fft_size, fft_floor=info.fft_floor, fft_ceil=info.fft_ceil)

    def close(self):
        if self.h:
            self._l.csdr_scope_destroy(self.h)
            self.h = C.c_void_p()


class ScopeBank:
    """N independent ScopeVisualProcessors of one fft_size (csdr_scopebank): one per demodulator, all slots and all frames of a call in two launches;
    state and items stay in HBM."""

    def __init__(self, ctx, fft_size, max_slots, max_frames=1, max_samples=4096):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_scopebank_create(ctx.h, C.byref(self.h)))
        self.setup(fft_size, max_slots, max_frames, max_samples)

    def setup(self, fft_size, max_slots, max_frames=1, max_samples=4096):
        H.check(self._l.csdr_scopebank_setup(self.h, int(fft_size), int(max_slots), int(max_frames), int(max_samples)))
        self.fft_size, self.max_slots, self.max_frames, self.max_samples = int(fft_size), int(max_slots), int(max_frames), int(max_samples)

    def set_enabled(self, scope=True, spectrum=True):
        H.check(self._l.csdr_scopebank_set_enabled(self.h, int(scope), int(spectrum)))

    def set_max_scope_samples(self, n):
        H.check(self._l.csdr_scopebank_set_max_scope_samples(self.h, int(n)))

    def set_average_rate(self, r):
        H.check(self._l.csdr_scopebank_set_average_rate(self.h, float(r)))

    def reset_slot(self, slot):
        H.check(self._l.csdr_scopebank_reset_slot(self.h, int(slot)))

    def try_process(self, items):
        """items: [(slot, frame)] with frame a dict as ScopeProcessor.process takes (host data), an H.ScopeFrame whose data lies in HBM
        (DemodBank.scope_frame), or None for no input; host and device frames do not mix in one call -> the return code"""
        arr = (H.ScopeBankItem * max(len(items), 1))()
        keep = []
        dev = any(isinstance(f, H.ScopeFrame) for _, f in items)
        for k, (slot, f) in enumerate(items):
            arr[k].slot = int(slot)
            if f is None:
                continue
            if isinstance(f, H.ScopeFrame):
                arr[k].frame = f
                continue
            if dev:
                raise ValueError("host and device frames in one call")
            a = np.ascontiguousarray(f["data"], dtype=np.float32)
            keep.append(a)
            arr[k].frame = H.ScopeFrame(a.ctypes.data if a.size else None, None, a.size, int(f["channels"]), int(f.get("type", 0)), int(f["sample_rate"]),
                                        int(f["input_rate"]), int(f.get("layout", 0)), float(f.get("scale", 1.0)))
        return self._l.csdr_scopebank_process(self.h, arr, len(items), 1 if dev else 0)

    def process(self, items):
        H.check(self.try_process(items))

    def process_bank(self, bank):
        """the scope tap of the bank's last execute, for every active slot the object has room for: one call, no host synchronisation"""
        H.check(self._l.csdr_scopebank_process_bank(self.h, bank.h))

    def frames(self, slot):
        return self._l.csdr_scopebank_frames(self.h, int(slot))

    def fetch(self, slot, frame, spectrum):
        """-> the dict ScopeProcessor.fetch returns, or None when that half was switched off"""
        pts = np.empty(max(2 * self.max_samples, self.fft_size), np.float32)
        info = H.ScopeInfo()
        H.check(self._l.csdr_scopebank_fetch(self.h, int(slot), int(frame), 1 if spectrum else 0, pts.ctypes.data_as(C.c_void_p), pts.size, C.byref(info)))
        if info.n_floats == 0:
            return None
        return dict(points=pts[:info.n_floats].copy(), mode=info.mode, spectrum=bool(info.spectrum), channels=info.channels, input_rate=info.input_rate,
                    sample_rate=info.sample_rate, fft_size=info.fft_size, fft_floor=info.fft_floor, fft_ceil=info.fft_ceil)

    def device_points(self, slot, spectrum):
        """(device pointer, frames, stride in floats) of the slot's items of the last call; the context's boundary stream waits for them"""
        p, n, st = C.c_void_p(), C.c_int(), C.c_int()
        H.check(self._l.csdr_scopebank_device_points(self.h, int(slot), 1 if spectrum else 0, C.byref(p), C.byref(n), C.byref(st)))
        return p.value, n.value, st.value

    def close(self):
        if self.h:
            self._l.csdr_scopebank_destroy(self.h)
            self.h = C.c_void_p()


SQUELCH_BLOCK = np.dtype([("level_accum", "<f8"), ("level_count", "<i4"), ("n_in", "<i4"), ("n_audio", "<i4"), ("audio_peak", "<f4")])     # csdr_squelch_block
SQUELCH_ITEM = np.dtype([("level", "<f4"), ("floor", "<f4"), ("ceil", "<f4"), ("flags", "<u4")])                                      # csdr_squelch_item


class SquelchBank:
    """DemodulatorThread's signal level, floor, ceiling and squelch for N demodulators (csdr_squelch): every slot stepped through every block of a
    batch in one launch; the flags gate the mixer feed (AudioMixer.push_bank_squelched) and a bank-wide PCM16 recorder (record)."""

    def __init__(self, ctx, max_slots, max_blocks):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        self.max_slots, self.max_blocks = int(max_slots), int(max_blocks)
        H.check(self._l.csdr_squelch_create(ctx.h, self.max_slots, self.max_blocks, C.byref(self.h)))

    def set_slot(self, slot, enabled=False, level_db=0.0, muted=False, record=H.CSDR_RECORD_SILENCE):
        """squelchEnabled, squelchLevel, muted and the recorder's option; read by the next process call"""
        H.check(self._l.csdr_squelch_set_slot(self.h, int(slot), int(bool(enabled)), float(level_db), int(bool(muted)), int(record)))

    def reset_slot(self, slot):
        H.check(self._l.csdr_squelch_reset_slot(self.h, int(slot)))

    def state(self, slot):
        """-> (signalLevel, signalFloor, signalCeil, squelchBreak) after the last process"""
        lv, fl, ce, br = C.c_float(), C.c_float(), C.c_float(), C.c_int()
        H.check(self._l.csdr_squelch_get_state(self.h, int(slot), C.byref(lv), C.byref(fl), C.byref(ce), C.byref(br)))
        return np.float32(lv.value), np.float32(fl.value), np.float32(ce.value), bool(br.value)

    def try_process(self, inputs):
        """inputs: [dict(slot, sample_rate, blocks, audio=None)]; blocks: a SQUELCH_BLOCK array or rows (level_accum, level_count, n_in, n_audio,
        audio_peak); audio: the blocks' floats back to back as a numpy array, or a DevicePointer -> the return code"""
        arr = (H.SquelchInput * max(len(inputs), 1))()
        keep = []
        for k, x in enumerate(inputs):
            blocks = np.ascontiguousarray(np.asarray(x["blocks"], dtype=SQUELCH_BLOCK) if not isinstance(x["blocks"], np.ndarray) else x["blocks"].astype(SQUELCH_BLOCK, copy=False))
            keep.append(blocks)
            arr[k].slot, arr[k].n_blocks, arr[k].sample_rate = int(x["slot"]), int(x.get("n_blocks", blocks.size)), int(x["sample_rate"])
            arr[k].blocks = C.cast(blocks.ctypes.data, C.POINTER(H.SquelchBlock)) if blocks.size else None
            audio = x.get("audio")
            if isinstance(audio, DevicePointer):
                arr[k].audio, arr[k].audio_is_dev = audio.ptr, 1
                keep.append(audio)
            elif audio is not None:
                a = np.ascontiguousarray(audio, dtype=np.float32)
                keep.append(a)
                arr[k].audio = a.ctypes.data if a.size else None
        return self._l.csdr_squelch_process(self.h, arr, len(inputs))

    def process(self, inputs):
        H.check(self.try_process(inputs))

    def process_bank(self, bank):
        """every block of the bank's last execute, read where it lies in HBM: one call, no host synchronisation"""
        H.check(self._l.csdr_squelch_process_bank(self.h, bank.h))

    def blocks(self, slot):
        return self._l.csdr_squelch_blocks(self.h, int(slot))

    def fetch(self, slot):
        """-> the slot's items of the last process, a SQUELCH_ITEM array"""
        out = np.empty(self.max_blocks, SQUELCH_ITEM)
        n = C.c_int()
        H.check(self._l.csdr_squelch_fetch(self.h, int(slot), C.cast(out.ctypes.data, C.POINTER(H.SquelchItem)), out.size, C.byref(n)))
        return out[:n.value].copy()

    def flags(self):
        """-> uint8 [max_slots, max_blocks] of the last process (0 where nothing was stepped): one copy for the whole bank"""
        out = np.empty((self.max_slots, self.max_blocks), np.uint8)
        H.check(self._l.csdr_squelch_fetch_flags(self.h, out.ctypes.data_as(C.c_void_p), out.size))
        return out

    def device_items(self):
        """(device pointer, stride in items) of the items of the last process; the context's boundary stream waits for them"""
        p, st = C.c_void_p(), C.c_int()
        H.check(self._l.csdr_squelch_device_items(self.h, C.byref(p), C.byref(st)))
        return p.value, st.value

    def record(self, cap=1 << 24):
        """-> (pcm int16 of every stepped slot packed in slot order, offsets int64 [max_slots + 1])"""
        out = np.empty(int(cap), np.int16)
        offs = np.empty(self.max_slots + 1, np.int64)
        H.check(self._l.csdr_squelch_record(self.h, out.ctypes.data_as(C.c_void_p), out.size, offs.ctypes.data_as(C.c_void_p)))
        return out[:offs[-1]], offs

    def close(self):
        if self.h:
            self._l.csdr_squelch_destroy(self.h)
            self.h = C.c_void_p()


class AudioMixer:
    """AudioThread's mixing callback (csdr_mix): per-source block queues, rings in HBM, bit-exact mix-down."""

    def __init__(self, ctx, n_sources, sample_rate=48000, ring_floats=1 << 20, queue_blocks=0):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        H.check(self._l.csdr_mix_create(ctx.h, int(n_sources), int(ring_floats), int(sample_rate), C.byref(self.h)))
        for i in range(n_sources):
            self.set_source(i, queue_blocks=queue_blocks)

    def set_source(self, i, bound=True, active=True, gain=1.0, queue_blocks=0):
        H.check(self._l.csdr_mix_set_source(self.h, int(i), int(bound), int(active), float(gain), int(queue_blocks)))

    def push(self, i, data, channels, sample_rate, peak):
        """-> True when the queue took the block (False: full, dropped -- try_push semantics)"""
        a = np.ascontiguousarray(data, dtype=np.float32)
        rc = self._l.csdr_mix_push(self.h, int(i), a.ctypes.data_as(C.c_void_p), 0, a.size, int(channels), int(sample_rate), float(peak))
        if rc == 1:
            return False
        H.check(rc)
        return True

    def push_bank(self, bank, slots, sources=None):
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        so = np.ascontiguousarray(sources if sources is not None else slots, dtype=np.int32)
        H.check(self._l.csdr_mix_push_bank(self.h, bank.h, sl.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p), sl.size))

    def push_bank_squelched(self, bank, squelch, slots, sources=None):
        """push_bank for the blocks `squelch` (a SquelchBank whose last process was process_bank of the bank's last execute) left open"""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        so = np.ascontiguousarray(sources if sources is not None else slots, dtype=np.int32)
        H.check(self._l.csdr_mix_push_squelched(self.h, bank.h, squelch.h, sl.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p), sl.size))

    def queued(self, i):
        return self._l.csdr_mix_queued(self.h, int(i))

    def render(self, frames, n_buffers=1, fetch=True):
        out = np.empty(n_buffers * frames * 2, np.float32) if fetch else None
        H.check(self._l.csdr_mix_render(self.h, int(frames), int(n_buffers), out.ctypes.data_as(C.c_void_p) if fetch else None))
        return out

    def pcm16(self, peak=1.0, per_buffer_peak=False, cap=1 << 22):
        out = np.empty(cap, np.int16)
        n = C.c_int()
        H.check(self._l.csdr_mix_fetch_pcm16(self.h, out.ctypes.data_as(C.c_void_p), cap, float(peak), int(per_buffer_peak), C.byref(n)))
        return out[:n.value].copy()

    def close(self):
        if self.h:
            self._l.csdr_mix_destroy(self.h)
            self.h = C.c_void_p()


class Comm:
    """csdr_comm: the collectives of ONE stream over the GPUs of a node, RCCL over xGMI behind the C ABI (csdr_comm.hip).  Every rank
    creates one on its own Context with the same 128-byte id (rank 0 makes it: Comm.unique_id(); how it reaches the other ranks is the
    host's business -- parallel.exchange_id uses a TCP store).  Buffers are device memory (torch CUDA tensors / DevicePointer; numpy
    arrays with the host-executing test build); counts are complex samples."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(Comm.ID_BYTES)
        H.check(H.lib().csdr_comm_unique_id(buf))
        return buf.raw

    def __init__(self, ctx, unique_id, rank, world):
        self._l = H.lib()
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        self.h = C.c_void_p()
        assert len(unique_id) == Comm.ID_BYTES
        H.check(self._l.csdr_comm_create(ctx.h, C.c_char_p(bytes(unique_id)), self.rank, self.world, C.byref(self.h)))

    @property
    def world_size(self):
        """ranks of the communicator as the library reports them (csdr_comm_world)"""
        return int(self._l.csdr_comm_world(self.h))

    @staticmethod
    def _ptr(buf):
        if buf is None:
            return None
        if isinstance(buf, np.ndarray):
            return buf.ctypes.data_as(C.c_void_p)
        if isinstance(buf, DevicePointer):
            return C.c_void_p(buf.ptr)
        return C.c_void_p(buf.data_ptr())

    def broadcast(self, iq, n_samples, root=0):
        H.check(self._l.csdr_comm_broadcast(self.h, self._ptr(iq), int(n_samples), int(root)))

    def scatter(self, send, recv, n_samples, root=0):
        H.check(self._l.csdr_comm_scatter(self.h, self._ptr(send), self._ptr(recv), int(n_samples), int(root)))

    def all_to_all(self, send, send_samples, recv, recv_samples):
        a = np.ascontiguousarray(send_samples, dtype=np.int64)
        b = np.ascontiguousarray(recv_samples, dtype=np.int64)
        assert a.size == self.world and b.size == self.world
        H.check(self._l.csdr_comm_all_to_all(self.h, self._ptr(send), a.ctypes.data_as(C.c_void_p), self._ptr(recv), b.ctypes.data_as(C.c_void_p)))

    def p2p(self, ops):
        """ops: [(peer, recv, buffer, byte_offset_in_samples, n_samples)] -- one grouped set of sends (recv False) and receives"""
        arr = (H.P2pOp * max(1, len(ops)))()
        for i, (peer, recv, buf, off, n) in enumerate(ops):
            base = self._ptr(buf).value or 0
            arr[i] = H.P2pOp(int(peer), 1 if recv else 0, base + 8 * int(off), int(n))
        H.check(self._l.csdr_comm_p2p(self.h, arr, len(ops)))

    def max(self, value):
        v = C.c_double(float(value))
        H.check(self._l.csdr_comm_max(self.h, C.byref(v)))
        return v.value

    def barrier(self):
        H.check(self._l.csdr_comm_barrier(self.h))

    def exchange_rows(self, producer, owner, owned, frame0, frames, n_blocks, block_len, frequency):
        """owned: per-rank channel lists; frame0 / frames: per-rank slab position inside the batch (frames = samples per channel)"""
        ch = np.ascontiguousarray([c for o in owned for c in o] or [0], dtype=np.int32)
        nch = np.ascontiguousarray([len(o) for o in owned], dtype=np.int32)
        f0 = np.ascontiguousarray(frame0, dtype=np.int64)
        fr = np.ascontiguousarray(frames, dtype=np.int64)
        assert nch.size == self.world and f0.size == self.world and fr.size == self.world
        H.check(self._l.csdr_post_exchange_rows(self.h, producer.h, owner.h, ch.ctypes.data_as(C.c_void_p), nch.ctypes.data_as(C.c_void_p),
                                                f0.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p), int(n_blocks), int(block_len), int(frequency)))

    def exchange_rows_begin(self, producer, owned, frame0, frames):
        """first half of exchange_rows: the transfers of the producer's current batch, on the communicator's own stream"""
        ch = np.ascontiguousarray([c for o in owned for c in o] or [0], dtype=np.int32)
        nch = np.ascontiguousarray([len(o) for o in owned], dtype=np.int32)
        f0 = np.ascontiguousarray(frame0, dtype=np.int64)
        fr = np.ascontiguousarray(frames, dtype=np.int64)
        assert nch.size == self.world and f0.size == self.world and fr.size == self.world
        H.check(self._l.csdr_post_exchange_rows_begin(self.h, producer.h, ch.ctypes.data_as(C.c_void_p), nch.ctypes.data_as(C.c_void_p),
                                                      f0.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p)))

    def exchange_rows_finish(self, owner, n_blocks, block_len, frequency):
        """second half, for the oldest batch begun: import into the owner behind that batch's transfers, commit"""
        H.check(self._l.csdr_post_exchange_rows_finish(self.h, owner.h, int(n_blocks), int(block_len), int(frequency)))
        owner._last = (int(n_blocks), int(block_len))

    @property
    def exchanges_pending(self):
        return int(self._l.csdr_comm_exchanges_pending(self.h))

    def abort(self):
        H.check(self._l.csdr_comm_abort(self.h))

    def async_error(self):
        """raises if a transfer of this communicator has failed (the communicator is then aborted on this rank too)"""
        H.check(self._l.csdr_comm_async_error(self.h))

    def close(self):
        if self.h:
            self._l.csdr_comm_destroy(self.h)
            self.h = C.c_void_p()


IQ_SAMPLE_BYTES = {H.CSDR_IQ_CF32: 8, H.CSDR_IQ_CS16: 4, H.CSDR_IQ_CS8: 2, H.CSDR_IQ_CU8: 2, H.CSDR_IQ_CS12: 3}
_IQ_DTYPE = {H.CSDR_IQ_CF32: np.float32, H.CSDR_IQ_CS16: np.int16, H.CSDR_IQ_CS8: np.int8, H.CSDR_IQ_CU8: np.uint8, H.CSDR_IQ_CS12: np.uint8}


def iq_format(format, full_scale=None, offset=0.0):
    """-> H.IqFormat.  `format`: a name ("CS16", "CS8", "CU8", "CS12", "CF32") or a CSDR_IQ_* constant; full_scale as the radio reports it."""
    f = H.IQ_FORMAT_BY_NAME[format] if isinstance(format, str) else int(format)
    if full_scale is None:
        if f != H.CSDR_IQ_CF32:
            raise ValueError("full_scale is required for an integer sample format (what the radio reports: 32768, 2048, 128 ...)")
        full_scale = 1.0                                      # unused: CF32 runs no conversion
    return H.IqFormat(f, float(offset), float(full_scale))


def pack_cs12(i, q):
    """integer I / Q arrays (the low 12 bits of each are kept) -> the packed 12-bit stream, 3 bytes per sample:
    b0 = I[7:0], b1 = Q[3:0] << 4 | I[11:8], b2 = Q[11:4]"""
    i = np.asarray(i).astype(np.int64) & 0xFFF
    q = np.asarray(q).astype(np.int64) & 0xFFF
    out = np.empty((i.size, 3), np.uint8)
    out[:, 0] = i & 0xFF
    out[:, 1] = ((q & 0xF) << 4) | (i >> 8)
    out[:, 2] = q >> 4
    return out.reshape(-1)


def iq_convert(ctx, raw, format, full_scale=None, offset=0.0, iq_swap=False, n_samples=None):
    """csdr_iq_convert: the conversion kernel alone on `raw` (a contiguous numpy array holding whole samples of the format) -> complex64"""
    f = iq_format(format, full_scale, offset)
    a = np.ascontiguousarray(raw)
    n = a.nbytes // IQ_SAMPLE_BYTES.get(f.format, 1) if n_samples is None else int(n_samples)
    out = np.empty(max(1, n), np.complex64)
    H.check(H.lib().csdr_iq_convert(ctx.h, C.byref(f), a.ctypes.data_as(C.c_void_p), n, int(iq_swap), out.ctypes.data_as(C.c_void_p)))
    return out[:n]


class Ingest:
    """page-locked block ring -> HBM, ONE transfer per block (csdr_ingest); commit returns the device pointer as an integer.
    With `format` (see iq_format) the slots hold the radio's own sample format and the block is widened to complex64 on the GPU."""

    def __init__(self, ctx, max_samples, depth=3, format=None, full_scale=None, offset=0.0):
        self._l = H.lib()
        self.ctx = ctx
        self.h = C.c_void_p()
        self.max_samples = int(max_samples)
        self.format = None
        if format is None:
            H.check(self._l.csdr_ingest_create(ctx.h, self.max_samples, int(depth), C.byref(self.h)))
        else:
            f = iq_format(format, full_scale, offset)
            H.check(self._l.csdr_ingest_create_raw(ctx.h, self.max_samples, int(depth), C.byref(f), C.byref(self.h)))
            self.format = f

    def acquire(self):
        """-> numpy view of the page-locked slot (max_samples long): complex64, or with a format its integers -- int16 / int8 / uint8 [n, 2] pairs,
        uint8 bytes (3 per sample) for CS12"""
        p = C.c_void_p()
        if self.format is None:
            H.check(self._l.csdr_ingest_acquire(self.h, C.byref(p)))
            buf = (C.c_float * (2 * self.max_samples)).from_address(p.value)
            return np.frombuffer(buf, dtype=np.complex64)
        H.check(self._l.csdr_ingest_acquire_raw(self.h, C.byref(p)))
        fmt = self.format.format
        buf = (C.c_ubyte * (IQ_SAMPLE_BYTES[fmt] * self.max_samples)).from_address(p.value)
        a = np.frombuffer(buf, dtype=_IQ_DTYPE[fmt])
        return a if fmt == H.CSDR_IQ_CS12 else a.reshape(-1, 2)

    def commit(self, n_samples, iq_swap=False):
        p = C.c_void_p()
        fn = self._l.csdr_ingest_commit if self.format is None else self._l.csdr_ingest_commit_raw
        H.check(fn(self.h, int(n_samples), int(iq_swap), C.byref(p)))
        return DevicePointer(p.value, int(n_samples))

    def upload_raw(self, raw, n_samples, iq_swap=False):
        """a block of the current format in the caller's own memory (any alignment, pageable or registered) -> DevicePointer"""
        p = C.c_void_p()
        H.check(self._l.csdr_ingest_upload_raw(self.h, C.c_void_p(raw.ctypes.data), int(n_samples), int(iq_swap), C.byref(p)))
        self._last_upload = raw                               # (the DMA may still read it: see wait())
        return DevicePointer(p.value, int(n_samples))

    def set_format(self, format, full_scale=None, offset=0.0):
        """from the next commit / upload on (a format whose samples are no larger than those the ring was created for)"""
        f = iq_format(format, full_scale, offset)
        H.check(self._l.csdr_ingest_set_format(self.h, C.byref(f)))
        self.format = f

    def next_slot(self):
        return self._l.csdr_ingest_next_slot(self.h)

    def wait(self):
        H.check(self._l.csdr_ingest_wait(self.h))

    def close(self):
        if self.h:
            self._l.csdr_ingest_destroy(self.h)
            self.h = C.c_void_p()


class DevicePointer:
    """a raw device IQ buffer (complex64 samples) that SDRPost.execute / SpectrumProcessor.process accept like a CUDA tensor"""

    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n
