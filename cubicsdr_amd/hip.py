"""ctypes binding of include/csdr_hip.h (the C ABI of libcsdr_hip.so).

There is no CPU fallback: importing works anywhere (so symbol checks can run without a GPU), but creating a
context without a HIP device raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcsdr_hip.so")

CSDR_POST_SINGLE, CSDR_POST_PFBCH, CSDR_POST_PFBCH2 = 0, 1, 2
CSDR_MODEM_NBFM, CSDR_MODEM_FM, CSDR_MODEM_AM, CSDR_MODEM_USB, CSDR_MODEM_LSB, CSDR_MODEM_IQ, CSDR_MODEM_CW, CSDR_MODEM_DSB, CSDR_MODEM_FMS, CSDR_MODEM_HOST = range(10)
CSDR_SPEC_FIRST_FRAME, CSDR_SPEC_CONTIGUOUS, CSDR_SPEC_LINES = 0, 1, 2
MODEM_BY_NAME = {"NBFM": 0, "FM": 1, "AM": 2, "USB": 3, "LSB": 4, "I/Q": 5, "IQ": 5, "CW": 6, "DSB": 7, "FMS": 8, "HOST": 9}
CSDR_MODEM_DIGITAL = 10
CSDR_DIGITAL_PSK, CSDR_DIGITAL_DPSK, CSDR_DIGITAL_ASK, CSDR_DIGITAL_QAM, CSDR_DIGITAL_BPSK, CSDR_DIGITAL_QPSK, CSDR_DIGITAL_OOK, CSDR_DIGITAL_FSK = range(8)
CSDR_DIGITAL_GMSK = 8
DIGITAL_BY_NAME = {"PSK": 0, "DPSK": 1, "ASK": 2, "QAM": 3, "BPSK": 4, "QPSK": 5, "OOK": 6, "FSK": 7, "GMSK": 8}
CSDR_DIGITAL_TABLE = 9
CSDR_TABLE_NEAREST, CSDR_TABLE_RINGS, CSDR_TABLE_QUADRANT = 0, 1, 2
CSDR_TABLE_MAX_POINTS, CSDR_TABLE_MAX_RINGS, CSDR_TABLE_MAX_TABLES = 256, 8, 8
CSDR_DIGITAL_MAX_CARRY = 2048
CSDR_IQ_CF32, CSDR_IQ_CS16, CSDR_IQ_CS8, CSDR_IQ_CU8, CSDR_IQ_CS12 = range(5)
IQ_FORMAT_BY_NAME = {"CF32": 0, "CS16": 1, "CS8": 2, "CU8": 3, "CS12": 4}


class DemodParams(C.Structure):
    _fields_ = [("modem", C.c_int32), ("bandwidth", C.c_int32), ("audio_sample_rate", C.c_int32),
                ("modem_arg", C.c_int32), ("frequency", C.c_int64)]


class BlockResult(C.Structure):
    _fields_ = [("n_iq", C.c_int32), ("n_audio", C.c_int32), ("audio_offset", C.c_int32), ("skipped", C.c_int32),
                ("level_accum", C.c_double), ("level_count", C.c_int32), ("audio_peak", C.c_float),
                ("nco_theta", C.c_uint32), ("resamp_phase", C.c_uint32), ("buffer_index", C.c_uint32),
                ("reserved", C.c_uint32)]


class DigitalParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("cons", C.c_int32), ("bps", C.c_int32), ("sps", C.c_int32), ("bw", C.c_float),
                ("fdelay", C.c_int32), ("reserved", C.c_int32 * 2)]


class DigitalResult(C.Structure):
    _fields_ = [("n_symbols", C.c_int32), ("symbol_offset", C.c_int32), ("lock", C.c_int32), ("evm", C.c_float),
                ("carry", C.c_int32), ("cons", C.c_int32), ("reserved", C.c_int32 * 2)]


class GmskState(C.Structure):
    _fields_ = [("x_prime", C.c_float * 2), ("reserved", C.c_int32 * 2)]


class DigitalState(C.Structure):
    _fields_ = [("r", C.c_float * 2), ("x_hat", C.c_float * 2), ("phi", C.c_float), ("n_carry", C.c_int32),
                ("reserved", C.c_int32 * 2), ("carry", C.c_float * (2 * CSDR_DIGITAL_MAX_CARRY))]


class Constellation(C.Structure):
    _fields_ = [("rule", C.c_int32), ("n_points", C.c_int32), ("sensitivity", C.c_float), ("n_rings", C.c_int32),
                ("points", C.c_float * (2 * CSDR_TABLE_MAX_POINTS)), ("ring_size", C.c_int32 * CSDR_TABLE_MAX_RINGS),
                ("ring_radius", C.c_float * CSDR_TABLE_MAX_RINGS), ("ring_phase", C.c_float * CSDR_TABLE_MAX_RINGS),
                ("ring_slicer", C.c_float * CSDR_TABLE_MAX_RINGS), ("ring_map", C.c_uint8 * CSDR_TABLE_MAX_POINTS)]


class IqFormat(C.Structure):
    _fields_ = [("format", C.c_int32), ("offset", C.c_float), ("full_scale", C.c_double)]


class DistribState(C.Structure):
    _fields_ = [("line_rate_accum", C.c_double), ("buffered_items", C.c_int64), ("buffer_offset", C.c_int64), ("buffer_max", C.c_int64),
                ("dropped", C.c_int64), ("n_lines", C.c_int32), ("line_len", C.c_int32)]


class ViewTap(C.Structure):
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("frac", C.c_float), ("half", C.c_int32)]


WF_VIEW_LINEAR, WF_VIEW_PEAK = 0, 1


class SpecBankItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n", C.c_int32), ("iq", C.c_void_p), ("is_dev", C.c_int32), ("reserved", C.c_int32)]


class ViewBankItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n", C.c_int32), ("iq", C.c_void_p), ("is_dev", C.c_int32), ("reserved", C.c_int32),
                ("frequency", C.c_int64), ("sample_rate", C.c_int64)]


class ViewBankSlotState(C.Structure):
    _fields_ = [("resample_bw", C.c_int64), ("shift_frequency", C.c_int64), ("desired_input_size", C.c_int32), ("last_data_size", C.c_int32),
                ("peak_reset", C.c_int32), ("num_written", C.c_int32)]


class WfBankItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_floats_per_line", C.c_int32), ("points", C.c_void_p), ("is_dev", C.c_int32), ("n_lines", C.c_int32)]


TRACE_SPECTRUM, TRACE_SCOPE_Y, TRACE_SCOPE_2Y, TRACE_SCOPE_XY = range(4)
TRACE_DEV_POINTS, TRACE_DEV_HOLD = 1, 2


class TraceItem(C.Structure):
    _fields_ = [("points", C.c_void_p), ("hold", C.c_void_p), ("n", C.c_int32), ("layout", C.c_int32), ("kind", C.c_int32), ("is_dev", C.c_int32)]


class DensityItem(C.Structure):
    _fields_ = [("points", C.c_void_p), ("stride_floats", C.c_int64), ("slot", C.c_int32), ("n", C.c_int32), ("frames", C.c_int32), ("layout", C.c_int32),
                ("kind", C.c_int32), ("is_dev", C.c_int32), ("keep_q16", C.c_uint32), ("weight", C.c_uint32)]


class DensityView(C.Structure):
    _fields_ = [("slot", C.c_int32), ("full", C.c_uint32)]


OVL_OVER, OVL_ADD, OVL_COPY = range(3)
ALIGN_LEFT, ALIGN_CENTER, ALIGN_RIGHT = range(3)
ALIGN_TOP, ALIGN_BOTTOM = 0, 2
SIDEBAND_BOTH, SIDEBAND_USB, SIDEBAND_LSB = range(3)
MARKER_DELTA_LOCK, MARKER_RECORDING, MARKER_MUTED, MARKER_SOLO, MARKER_CENTERLINE = 1, 2, 4, 8, 16


class OverlayPrim(C.Structure):
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("rgba", C.c_uint8 * 4), ("mode", C.c_int32), ("mask_x", C.c_int32),
                ("mask_y", C.c_int32)]


class OverlayTile(C.Structure):
    _fields_ = [("first", C.c_int32), ("count", C.c_int32)]


class FreqTick(C.Structure):
    _fields_ = [("m", C.c_double), ("value", C.c_double), ("major", C.c_int32), ("column", C.c_int32), ("label", C.c_char * 32)]


class FreqScale(C.Structure):
    _fields_ = [("step_mhz", C.c_double), ("tick_top", C.c_double), ("label_y", C.c_double), ("precision", C.c_int32), ("n_ticks", C.c_int32),
                ("font_size", C.c_int32), ("tick_rows", C.c_int32), ("label_row", C.c_int32), ("pad", C.c_int32)]


class DbGridRange(C.Structure):
    _fields_ = [("alpha", C.c_double), ("step", C.c_double), ("first", C.c_int32), ("count", C.c_int32)]


class DemodMarker(C.Structure):
    _fields_ = [("ux", C.c_float), ("ofs_left", C.c_float), ("ofs_right", C.c_float), ("label_v", C.c_float), ("narrow", C.c_int32), ("halign", C.c_int32),
                ("label_x", C.c_int32), ("label_y", C.c_int32), ("prefix", C.c_char * 8)]


class Glyph(C.Structure):
    _fields_ = [("id", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("xoffset", C.c_int32), ("yoffset", C.c_int32),
                ("xadvance", C.c_int32)]


class P2pOp(C.Structure):
    _fields_ = [("peer", C.c_int32), ("recv", C.c_int32), ("buf", C.c_void_p), ("n_samples", C.c_int64)]


class ScopeFrame(C.Structure):
    _fields_ = [("data", C.c_void_p), ("n_dev", C.c_void_p), ("n", C.c_int32), ("channels", C.c_int32), ("type", C.c_int32),
                ("sample_rate", C.c_int32), ("input_rate", C.c_int32), ("layout", C.c_int32), ("scale", C.c_float)]


class ScopeInfo(C.Structure):
    _fields_ = [("mode", C.c_int32), ("spectrum", C.c_int32), ("channels", C.c_int32), ("input_rate", C.c_int32), ("sample_rate", C.c_int32),
                ("fft_size", C.c_int32), ("n_floats", C.c_int32), ("reserved", C.c_int32), ("fft_floor", C.c_double), ("fft_ceil", C.c_double)]


class ScopeBankItem(C.Structure):
    _fields_ = [("slot", C.c_int32), ("reserved", C.c_int32), ("frame", ScopeFrame)]


CSDR_RECORD_SILENCE, CSDR_RECORD_SKIP_SILENCE, CSDR_RECORD_ALWAYS = 0, 1, 2
CSDR_SQUELCH_SQUELCHED, CSDR_SQUELCH_BREAK, CSDR_SQUELCH_OPEN = 1, 2, 4


class SquelchBlock(C.Structure):
    _fields_ = [("level_accum", C.c_double), ("level_count", C.c_int32), ("n_in", C.c_int32), ("n_audio", C.c_int32), ("audio_peak", C.c_float)]


class SquelchInput(C.Structure):
    _fields_ = [("slot", C.c_int32), ("n_blocks", C.c_int32), ("sample_rate", C.c_int32), ("audio_is_dev", C.c_int32),
                ("blocks", C.POINTER(SquelchBlock)), ("audio", C.c_void_p)]


class SquelchItem(C.Structure):
    _fields_ = [("level", C.c_float), ("floor", C.c_float), ("ceil", C.c_float), ("flags", C.c_uint32)]


_p, _i, _i64, _f, _d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
_pp = C.POINTER(C.c_void_p)

# every symbol include/csdr_hip.h declares: name -> (restype, argtypes)
ABI = {
    "csdr_abi_version": (_i, []),
    "csdr_strerror": (C.c_char_p, [_i]),
    "csdr_last_error": (C.c_char_p, []),
    "csdr_ctx_create": (_i, [_i, _p, _pp]),
    "csdr_ctx_destroy": (None, [_p]),
    "csdr_ctx_synchronize": (_i, [_p]),
    "csdr_ctx_join": (_i, [_p]),
    "csdr_ctx_stream": (_p, [_p]),
    "csdr_ctx_owns_stream": (_i, [_p]),
    "csdr_ctx_timer_start": (_i, [_p]),
    "csdr_ctx_timer_stop": (_i, [_p, C.POINTER(_f)]),
    "csdr_ctx_profile_enable": (_i, [_p, _i]),
    "csdr_ctx_profile_num_kernels": (_i, []),
    "csdr_ctx_profile_kernel_name": (C.c_char_p, [_i]),
    "csdr_ctx_profile_fetch": (_i, [_p, _i, C.POINTER(_d), C.POINTER(_i64)]),
    "csdr_ctx_profile_launches": (_i, [_p, _i, C.POINTER(_i64)]),
    "csdr_ctx_profile_range": (_i, [_p, _i, C.POINTER(_d), C.POINTER(_d)]),
    "csdr_dev_alloc": (_i, [_p, C.c_uint64, _pp]),
    "csdr_dev_free": (_i, [_p, _p]),
    "csdr_dev_upload": (_i, [_p, _p, _p, C.c_uint64]),
    "csdr_dev_download": (_i, [_p, _p, _p, C.c_uint64]),
    "csdr_host_register": (_i, [_p, _p, C.c_uint64]),
    "csdr_host_unregister": (_i, [_p, _p]),
    "csdr_post_create": (_i, [_p, _pp]),
    "csdr_post_destroy": (None, [_p]),
    "csdr_post_configure": (_i, [_p, _i64, _i, _i, _i, _i]),
    "csdr_post_execute": (_i, [_p, _p, _i, _i, _i, _i64]),
    "csdr_post_set_active_channels": (_i, [_p, _p, _i]),
    "csdr_post_channel_bandwidth": (_i64, [_p]),
    "csdr_post_channel_rate": (_i64, [_p]),
    "csdr_post_num_channels": (_i, [_p]),
    "csdr_post_kernel_name": (C.c_char_p, [_p]),
    "csdr_post_set_row_order": (_i, [_p, _p, _i]),
    "csdr_post_channel_center": (_i64, [_p, _i]),
    "csdr_post_channel_at": (_i, [_p, _i64]),
    "csdr_post_read_channel": (_i, [_p, _i, _p, _i, C.POINTER(_i)]),
    "csdr_bank_create": (_i, [_p, _i, _i, _pp]),
    "csdr_bank_destroy": (None, [_p]),
    "csdr_bank_configure_slot": (_i, [_p, _i, C.POINTER(DemodParams), _p]),
    "csdr_bank_set_frequency": (_i, [_p, _i, _i64]),
    "csdr_bank_set_active": (_i, [_p, _i, _i]),
    "csdr_bank_execute": (_i, [_p, _p]),
    "csdr_bank_fetch_results": (_i, [_p, _i, C.POINTER(BlockResult), _i, C.POINTER(_i)]),
    "csdr_bank_fetch_audio": (_i, [_p, _i, _p, _i, C.POINTER(_i)]),
    "csdr_bank_fetch_iq": (_i, [_p, _i, _p, _i, C.POINTER(_i)]),
    "csdr_bank_fetch_demod_output": (_i, [_p, _i, _p, _i, C.POINTER(_i)]),
    "csdr_post_history_length": (_i, [_p]),
    "csdr_post_set_history": (_i, [_p, _p, _i64]),
    "csdr_post_set_dc_blocker": (_i, [_p, _i]),
    "csdr_post_export_rows": (_i, [_p, _p, _i, _p, _i64]),
    "csdr_post_import_begin": (_i, [_p, _i, _i, _i64]),
    "csdr_post_import_rows": (_i, [_p, _p, _i, _p, _i64, _i64, _i64]),
    "csdr_post_import_commit": (_i, [_p]),
    "csdr_design_fms_pilot": (_i, [_i64, _p, _p]),
    "csdr_bank_set_fms_pilot": (_i, [_p, _i, _p, _p]),
    "csdr_bank_fetch_fms_stage": (_i, [_p, _i, _i, _p, _i, C.POINTER(_i)]),
    "csdr_bank_total_audio": (_i, [_p, C.POINTER(_i64)]),
    "csdr_spec_create": (_i, [_p, _pp]),
    "csdr_spec_destroy": (None, [_p]),
    "csdr_spec_setup": (_i, [_p, _i, _i]),
    "csdr_spec_set_average_rate": (_i, [_p, _f]),
    "csdr_spec_set_scale_factor": (_i, [_p, _f]),
    "csdr_spec_set_peak_hold": (_i, [_p, _i]),
    "csdr_spec_get_peak_hold": (_i, [_p]),
    "csdr_spec_set_hide_dc": (_i, [_p, _i]),
    "csdr_spec_set_center_frequency": (_i, [_p, _i64]),
    "csdr_spec_set_bandwidth": (_i, [_p, _i64]),
    "csdr_spec_set_input_frequency": (_i, [_p, _i64]),
    "csdr_spec_set_view": (_i, [_p, _i]),
    "csdr_spec_get_view": (_i, [_p]),
    "csdr_spec_set_input_rate": (_i, [_p, _i64]),
    "csdr_spec_desired_input_size": (_i, [_p]),
    "csdr_spec_process": (_i, [_p, _p, _i, _i, _i, _i]),
    "csdr_spec_frames": (_i, [_p]),
    "csdr_spec_fetch": (_i, [_p, _i, _p, _i, C.POINTER(_d), C.POINTER(_d)]),
    "csdr_spec_fetch_hold": (_i, [_p, _i, _p, _i, C.POINTER(_i)]),
    "csdr_spec_fft_only": (_i, [_p, _p, _p]),
    "csdr_scope_create": (_i, [_p, _pp]),
    "csdr_scope_destroy": (None, [_p]),
    "csdr_scope_setup": (_i, [_p, _i, _i, _i]),
    "csdr_scope_set_enabled": (_i, [_p, _i, _i]),
    "csdr_scope_set_max_scope_samples": (_i, [_p, _i]),
    "csdr_scope_set_average_rate": (_i, [_p, _f]),
    "csdr_scope_process": (_i, [_p, C.POINTER(ScopeFrame), _i, _i]),
    "csdr_scope_frames": (_i, [_p]),
    "csdr_scope_fetch": (_i, [_p, _i, _i, _p, _i, C.POINTER(ScopeInfo)]),
    "csdr_bank_scope_frame": (_i, [_p, _i, C.POINTER(ScopeFrame)]),
    "csdr_mix_create": (_i, [_p, _i, _i, _i, _pp]),
    "csdr_mix_destroy": (None, [_p]),
    "csdr_mix_set_source": (_i, [_p, _i, _i, _i, _f, _i]),
    "csdr_mix_push": (_i, [_p, _i, _p, _i, _i, _i, _i, _f]),
    "csdr_mix_push_bank": (_i, [_p, _p, _p, _p, _i]),
    "csdr_mix_queued": (_i, [_p, _i]),
    "csdr_mix_render": (_i, [_p, _i, _i, _p]),
    "csdr_mix_fetch_pcm16": (_i, [_p, _p, _i, _f, _i, C.POINTER(_i)]),
    "csdr_bank_fetch_pcm16": (_i, [_p, _i, _p, _i, C.POINTER(_i)]),
    "csdr_ingest_create": (_i, [_p, _i64, _i, _pp]),
    "csdr_ingest_destroy": (None, [_p]),
    "csdr_ingest_acquire": (_i, [_p, _pp]),
    "csdr_ingest_commit": (_i, [_p, _i64, _i, _pp]),
    "csdr_ingest_upload": (_i, [_p, _p, _i64, _i, _pp]),
    "csdr_ingest_wait": (_i, [_p]),
    "csdr_comm_unique_id": (_i, [_p]),
    "csdr_comm_create": (_i, [_p, _p, _i, _i, _pp]),
    "csdr_comm_destroy": (None, [_p]),
    "csdr_comm_rank": (_i, [_p]),
    "csdr_comm_world": (_i, [_p]),
    "csdr_comm_broadcast": (_i, [_p, _p, _i64, _i]),
    "csdr_comm_scatter": (_i, [_p, _p, _p, _i64, _i]),
    "csdr_comm_all_to_all": (_i, [_p, _p, _p, _p, _p]),
    "csdr_comm_p2p": (_i, [_p, _p, _i]),
    "csdr_comm_max": (_i, [_p, C.POINTER(_d)]),
    "csdr_comm_barrier": (_i, [_p]),
    "csdr_post_exchange_rows": (_i, [_p, _p, _p, _p, _p, _p, _p, _i, _i, _i64]),
    "csdr_post_exchange_rows_begin": (_i, [_p, _p, _p, _p, _p, _p]),
    "csdr_post_exchange_rows_finish": (_i, [_p, _p, _i, _i, _i64]),
    "csdr_comm_exchanges_pending": (_i, [_p]),
    "csdr_comm_abort": (_i, [_p]),
    "csdr_comm_async_error": (_i, [_p]),
    "csdr_ingest_next_slot": (_i, [_p]),
    "csdr_bank_configure_digital_slot": (_i, [_p, _i, C.POINTER(DemodParams), C.POINTER(DigitalParams), _p]),
    "csdr_bank_set_digital_cons": (_i, [_p, _i, _i]),
    "csdr_bank_fetch_digital_results": (_i, [_p, _i, C.POINTER(DigitalResult), _i, C.POINTER(_i)]),
    "csdr_bank_fetch_symbols": (_i, [_p, _i, _p, _i, C.POINTER(_i)]),
    "csdr_digital_run": (_i, [_p, C.POINTER(DigitalParams), _i64, _p, _i, C.POINTER(DigitalState), _p, _i, C.POINTER(_i), C.POINTER(_f)]),
    "csdr_iq_format_bytes": (_i, [_i, _i64, C.POINTER(C.c_uint64)]),
    "csdr_ingest_create_raw": (_i, [_p, _i64, _i, C.POINTER(IqFormat), _pp]),
    "csdr_ingest_acquire_raw": (_i, [_p, _pp]),
    "csdr_ingest_commit_raw": (_i, [_p, _i64, _i, _pp]),
    "csdr_ingest_upload_raw": (_i, [_p, _p, _i64, _i, _pp]),
    "csdr_ingest_set_format": (_i, [_p, C.POINTER(IqFormat)]),
    "csdr_iq_convert": (_i, [_p, C.POINTER(IqFormat), _p, _i64, _i, _p]),
    "csdr_gmsk_run": (_i, [_p, C.POINTER(DigitalParams), _p, _i, C.POINTER(GmskState), _p, _p, _p, _i, C.POINTER(_i)]),
    "csdr_design_rings": (_i, [_p, _i, C.POINTER(Constellation)]),
    "csdr_bank_configure_table_slot": (_i, [_p, _i, C.POINTER(DemodParams), C.POINTER(Constellation), _i, _p]),
    "csdr_waterfall_create": (_i, [_p, _pp]),
    "csdr_waterfall_destroy": (None, [_p]),
    "csdr_waterfall_setup": (_i, [_p, _i, _i, _i]),
    "csdr_design_gradient": (_i, [_p, _i, _i, _p, _p, _p]),
    "csdr_waterfall_set_gradient": (_i, [_p, _p, _i]),
    "csdr_waterfall_step": (_i, [_p, _p, _i, _i, _i, C.POINTER(_i)]),
    "csdr_waterfall_step_spec": (_i, [_p, _p, _i, _i, C.POINTER(_i)]),
    "csdr_waterfall_update": (_i, [_p]),
    "csdr_waterfall_lines_buffered": (_i, [_p]),
    "csdr_waterfall_offset": (_i, [_p, _i]),
    "csdr_waterfall_fetch_index": (_i, [_p, _i, _p, _i64]),
    "csdr_waterfall_fetch_rgba": (_i, [_p, _i, _i, _p, _i64]),
    "csdr_waterfall_device_rgba": (_i, [_p, _pp]),
    "csdr_design_view_columns": (_i, [_i, _i, _i, _p]),
    "csdr_design_view_rows": (_i, [_i, _i, _i, _p]),
    "csdr_waterfall_render_view": (_i, [_p, _i, _i, _i, _p, _i64]),
    "csdr_waterfall_device_view": (_i, [_p, _pp, C.POINTER(_i), C.POINTER(_i)]),
    "csdr_distrib_create": (_i, [_p, _i, _pp]),
    "csdr_distrib_destroy": (None, [_p]),
    "csdr_distrib_set_fft_size": (_i, [_p, _i]),
    "csdr_distrib_set_lines_per_second": (_i, [_p, _i]),
    "csdr_distrib_push": (_i, [_p, _p, _i, _i, _i64, _i64, C.POINTER(_i)]),
    "csdr_distrib_get_state": (_i, [_p, C.POINTER(DistribState)]),
    "csdr_distrib_lines": (_i, [_p, _pp, C.POINTER(_i), C.POINTER(_i)]),
    "csdr_distrib_fetch_lines": (_i, [_p, _p, _i64, C.POINTER(_i)]),
    "csdr_distrib_fetch_buffered": (_i, [_p, _p, _i64, C.POINTER(_i)]),
    "csdr_spec_process_distrib": (_i, [_p, _p]),
    "csdr_specbank_create": (_i, [_p, _pp]),
    "csdr_specbank_destroy": (None, [_p]),
    "csdr_specbank_setup": (_i, [_p, _i, _i, _i]),
    "csdr_specbank_set_average_rate": (_i, [_p, _f]),
    "csdr_specbank_set_scale_factor": (_i, [_p, _f]),
    "csdr_specbank_set_peak_hold": (_i, [_p, _i]),
    "csdr_specbank_get_peak_hold": (_i, [_p]),
    "csdr_specbank_reset_slot": (_i, [_p, _i]),
    "csdr_specbank_process": (_i, [_p, C.POINTER(SpecBankItem), _i]),
    "csdr_specbank_process_bank": (_i, [_p, _p]),
    "csdr_specbank_frames": (_i, [_p, _i]),
    "csdr_specbank_fetch": (_i, [_p, _i, _i, _p, _i, C.POINTER(_d), C.POINTER(_d)]),
    "csdr_specbank_fetch_hold": (_i, [_p, _i, _i, _p, _i, C.POINTER(_i)]),
    "csdr_specbank_device_points": (_i, [_p, _i, _pp, C.POINTER(_i)]),
    "csdr_viewbank_create": (_i, [_p, _pp]),
    "csdr_viewbank_destroy": (None, [_p]),
    "csdr_viewbank_setup": (_i, [_p, _i, _i, _i, _i]),
    "csdr_viewbank_set_average_rate": (_i, [_p, _f]),
    "csdr_viewbank_set_scale_factor": (_i, [_p, _f]),
    "csdr_viewbank_set_peak_hold": (_i, [_p, _i]),
    "csdr_viewbank_get_peak_hold": (_i, [_p]),
    "csdr_viewbank_set_hide_dc": (_i, [_p, _i]),
    "csdr_viewbank_set_view": (_i, [_p, _i, C.c_int64, C.c_int64]),
    "csdr_viewbank_reset_slot": (_i, [_p, _i]),
    "csdr_viewbank_process": (_i, [_p, C.POINTER(ViewBankItem), _i]),
    "csdr_viewbank_process_post": (_i, [_p, _p, _p, _p, _i]),
    "csdr_viewbank_frames": (_i, [_p, _i]),
    "csdr_viewbank_fetch": (_i, [_p, _i, _i, _p, _i, C.POINTER(_d), C.POINTER(_d)]),
    "csdr_viewbank_fetch_hold": (_i, [_p, _i, _i, _p, _i, C.POINTER(_i)]),
    "csdr_viewbank_device_points": (_i, [_p, _i, _pp, C.POINTER(_i)]),
    "csdr_viewbank_slot_info": (_i, [_p, _i, C.POINTER(ViewBankSlotState)]),
    "csdr_viewbank_fetch_last": (_i, [_p, _i, _p, _i]),
    "csdr_scopebank_create": (_i, [_p, _pp]),
    "csdr_scopebank_destroy": (None, [_p]),
    "csdr_scopebank_setup": (_i, [_p, _i, _i, _i, _i]),
    "csdr_scopebank_set_enabled": (_i, [_p, _i, _i]),
    "csdr_scopebank_set_max_scope_samples": (_i, [_p, _i]),
    "csdr_scopebank_set_average_rate": (_i, [_p, _f]),
    "csdr_scopebank_reset_slot": (_i, [_p, _i]),
    "csdr_scopebank_process": (_i, [_p, C.POINTER(ScopeBankItem), _i, _i]),
    "csdr_scopebank_process_bank": (_i, [_p, _p]),
    "csdr_scopebank_frames": (_i, [_p, _i]),
    "csdr_scopebank_fetch": (_i, [_p, _i, _i, _i, _p, _i, C.POINTER(ScopeInfo)]),
    "csdr_scopebank_device_points": (_i, [_p, _i, _i, _pp, C.POINTER(_i), C.POINTER(_i)]),
    "csdr_squelch_create": (_i, [_p, _i, _i, _pp]),
    "csdr_squelch_destroy": (None, [_p]),
    "csdr_squelch_set_slot": (_i, [_p, _i, _i, _f, _i, _i]),
    "csdr_squelch_reset_slot": (_i, [_p, _i]),
    "csdr_squelch_get_state": (_i, [_p, _i, C.POINTER(_f), C.POINTER(_f), C.POINTER(_f), C.POINTER(_i)]),
    "csdr_squelch_process": (_i, [_p, C.POINTER(SquelchInput), _i]),
    "csdr_squelch_process_bank": (_i, [_p, _p]),
    "csdr_squelch_blocks": (_i, [_p, _i]),
    "csdr_squelch_fetch": (_i, [_p, _i, C.POINTER(SquelchItem), _i, C.POINTER(_i)]),
    "csdr_squelch_fetch_flags": (_i, [_p, _p, _i64]),
    "csdr_squelch_device_items": (_i, [_p, _pp, C.POINTER(_i)]),
    "csdr_squelch_record": (_i, [_p, _p, _i64, _p]),
    "csdr_mix_push_squelched": (_i, [_p, _p, _p, _p, _p, _i]),
    "csdr_wfbank_create": (_i, [_p, _pp]),
    "csdr_wfbank_destroy": (None, [_p]),
    "csdr_wfbank_setup": (_i, [_p, _i, _i, _i, _i]),
    "csdr_wfbank_set_gradient": (_i, [_p, _p, _i]),
    "csdr_wfbank_reset_slot": (_i, [_p, _i]),
    "csdr_wfbank_step": (_i, [_p, C.POINTER(WfBankItem), _i, C.POINTER(_i)]),
    "csdr_wfbank_step_specbank": (_i, [_p, _p, C.POINTER(_i)]),
    "csdr_wfbank_update": (_i, [_p]),
    "csdr_wfbank_lines_buffered": (_i, [_p, _i]),
    "csdr_wfbank_offset": (_i, [_p, _i, _i]),
    "csdr_wfbank_fetch_index": (_i, [_p, _i, _i, _p, _i64]),
    "csdr_wfbank_render": (_i, [_p, C.POINTER(_i), _i, _i, _i, _i, _i, _p, _i64]),
    "csdr_wfbank_device_view": (_i, [_p, _pp, C.POINTER(_i), C.POINTER(_i)]),
    "csdr_tracebank_create": (_i, [_p, _pp]),
    "csdr_tracebank_destroy": (None, [_p]),
    "csdr_tracebank_setup": (_i, [_p, _i, _i]),
    "csdr_tracebank_set_colors": (_i, [_p, _p, _p, _p, _p, _p]),
    "csdr_tracebank_render": (_i, [_p, C.POINTER(TraceItem), _i, _i, _i, _i, _p, _i64]),
    "csdr_tracebank_device_view": (_i, [_p, _pp, C.POINTER(_i), C.POINTER(_i)]),
    "csdr_design_trace_envelope": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p]),
    "csdr_overlay_create": (_i, [_p, _pp]),
    "csdr_overlay_destroy": (None, [_p]),
    "csdr_overlay_setup": (_i, [_p, _i, _i]),
    "csdr_overlay_set_font": (_i, [_p, _p, _i, _i]),
    "csdr_overlay_compose": (_i, [_p, _p, _i, C.POINTER(OverlayTile), _i, C.POINTER(OverlayPrim), _i, _i, _i, _i, _p, _i64]),
    "csdr_overlay_device_view": (_i, [_p, _pp, C.POINTER(_i), C.POINTER(_i)]),
    "csdr_design_freq_scale": (_i, [_i64, _i64, _i, _i, C.c_double, C.POINTER(FreqScale), C.POINTER(FreqTick), _i]),
    "csdr_design_db_grid": (_i, [C.c_float, C.c_float, C.POINTER(DbGridRange), C.POINTER(_i), C.POINTER(C.c_double), _i]),
    "csdr_design_db_labels": (_i, [C.c_float, C.c_float, _i, C.c_double, C.c_char_p, C.c_char_p, _i]),
    "csdr_design_demod_marker": (_i, [_i64, _i, _i, _i64, _i64, _i, _i, _i, _p, C.POINTER(DemodMarker), C.POINTER(OverlayPrim), C.POINTER(_i)]),
    "csdr_design_text": (_i, [C.POINTER(Glyph), _i, _i, C.c_char_p, _i, _i, _i, _i, _p, _i, C.POINTER(OverlayPrim), _i, C.POINTER(_i)]),
    "csdr_density_create": (_i, [_p, _pp]),
    "csdr_density_destroy": (None, [_p]),
    "csdr_density_setup": (_i, [_p, _i, _i, _i, _i, _i]),
    "csdr_density_set_palette": (_i, [_p, _p]),
    "csdr_density_reset_slot": (_i, [_p, _i]),
    "csdr_density_step": (_i, [_p, C.POINTER(DensityItem), _i]),
    "csdr_density_step_spec": (_i, [_p, _i, _p, _i, _i, C.c_uint32, C.c_uint32]),
    "csdr_density_step_specbank": (_i, [_p, _p, C.c_uint32, C.c_uint32]),
    "csdr_density_peak": (_i, [_p, _i, C.POINTER(C.c_uint32)]),
    "csdr_density_fetch": (_i, [_p, _i, _p, _i64]),
    "csdr_density_render": (_i, [_p, C.POINTER(DensityView), _i, _i, _p, _i64]),
    "csdr_density_device_view": (_i, [_p, _pp, C.POINTER(_i), C.POINTER(_i)]),
    "csdr_design_density_cover": (_i, [_p, _i, _i, _i64, _i, _i, _i, _i, _p]),
    "csdr_table_run": (_i, [_p, C.POINTER(Constellation), _p, _i, C.POINTER(DigitalState), _p, _i, C.POINTER(_i), C.POINTER(_f)]),
}

_lib = None


class CsdrError(RuntimeError):
    pass


def lib():
    """Load libcsdr_hip.so (built in-tree by cubicsdr_amd/build.py).  Fails loudly when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CsdrError("HIP extension %s is missing: run `python -m cubicsdr_amd.build` (no CPU fallback exists)" % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc):
    if rc != 0:
        l = lib()
        raise CsdrError("%s: %s" % (l.csdr_strerror(rc).decode(), l.csdr_last_error().decode()))


def _host_ptr(a):
    return a.ctypes.data_as(C.c_void_p)
