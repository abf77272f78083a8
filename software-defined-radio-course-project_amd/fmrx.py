"""fmrx.py — Python host binding of libfmrx.so (the C ABI in include/fmrx.h).

Mirrors the reference's per-block interface (src/project.cpp rf_thread / audio_thread bodies
and the filter.h primitives) for tests, the bench and Python callers.  There is no CPU
compute path here: everything numeric runs in the HIP kernels of libfmrx.so, and loading
fails loudly if the library has not been built.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from concurrent.futures import ThreadPoolExecutor
from contextlib import contextmanager
from typing import NamedTuple

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG_DIR)
# FMRX_LIB_PATH: an A/B build of the same sources (Makefile `ab` target; measurements only)
LIB_PATH = os.environ.get("FMRX_LIB_PATH") or os.path.join(PKG_DIR, "libfmrx.so")
HEADER = os.path.join(REPO, "include", "fmrx.h")

FMRX_OK, FMRX_EINVAL, FMRX_EHIP, FMRX_ENOMEM, FMRX_ESTATE = 0, -1, -2, -3, -4
MONO, STEREO = 1, 2
# raw I/Q formats (include/fmrx.h FMRX_IQ_*)
IQ_U8, IQ_S8, IQ_S16, IQ_F32 = 0, 1, 2, 3
IQ_DTYPES = {IQ_U8: np.dtype(np.uint8), IQ_S8: np.dtype(np.int8), IQ_S16: np.dtype("<i2"), IQ_F32: np.dtype("<f4")}


class FmrxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"fmrx error {code}: {msg}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("mode", C.c_int), ("channels", C.c_int), ("rf_taps", C.c_int),
                ("bp_taps", C.c_int), ("audio_taps", C.c_int), ("n_streams", C.c_int),
                ("device", C.c_int)]


class Geometry(C.Structure):
    _fields_ = [("rf_fs", C.c_int), ("rf_decim", C.c_int), ("if_fs", C.c_int), ("bp_fs", C.c_int),
                ("audio_up", C.c_int), ("audio_down", C.c_int), ("rf_taps", C.c_int),
                ("bp_taps", C.c_int), ("audio_taps_total", C.c_int), ("block_bytes", C.c_size_t),
                ("iq_pairs", C.c_size_t), ("if_samples", C.c_size_t), ("audio_frames", C.c_size_t),
                ("pcm_samples", C.c_size_t)]


class ScanConfig(C.Structure):
    """fmrx_scan_config (include/fmrx.h): the band scan's transform size and detector settings."""
    _fields_ = [("fft_bins", C.c_int), ("raster_hz", C.c_int), ("raster_origin_hz", C.c_int),
                ("channel_hz", C.c_int), ("min_separation_hz", C.c_int), ("dc_notch_bins", C.c_int),
                ("floor_percentile", C.c_int), ("min_snr_db", C.c_float)]


class Station(C.Structure):
    """fmrx_station: a station the band scan found, offset_hz from the capture's centre."""
    _fields_ = [("offset_hz", C.c_int32), ("power_db", C.c_float), ("snr_db", C.c_float)]

    def __repr__(self):
        return f"Station(offset_hz={self.offset_hz}, power_db={self.power_db:.2f}, snr_db={self.snr_db:.2f})"


RDS_TAIL = 103  # include/fmrx.h FMRX_RDS_TAIL
RDS_WINDOW, RDS_BITS_PER_WINDOW = 2432, 76  # 38 kS/s samples and bits a window of the RDS back half


class RdsInfo(C.Structure):
    """Mirror of fmrx_rds_info: what the RDS group parser has read so far."""
    _fields_ = [("bits", C.c_uint64), ("blocks", C.c_uint64), ("groups", C.c_uint64), ("pi", C.c_uint16),
                ("pty", C.c_uint8), ("tp", C.c_uint8), ("rt_ab", C.c_uint8), ("tail_n", C.c_uint8),
                ("ps_raw", C.c_char * 9), ("rt_raw", C.c_char * 65), ("tail_bits", C.c_uint8 * RDS_TAIL),
                ("tail_codes", C.c_uint8 * RDS_TAIL)]

    def __init__(self):
        super().__init__()
        _check(lib().fmrx_rds_info_init(C.byref(self)))

    @property
    def ps(self) -> str:
        return self.ps_raw.decode("ascii")

    @property
    def rt(self) -> str:
        return self.rt_raw.decode("ascii")

    def as_dict(self) -> dict:
        return {"pi": self.pi, "pty": self.pty, "tp": self.tp, "ps": self.ps, "rt": self.rt, "bits": self.bits,
                "blocks": self.blocks, "groups": self.groups}


RDS_EXT_TAIL, RDS_MAX_AF = 16, 25  # include/fmrx.h FMRX_RDS_EXT_TAIL, FMRX_RDS_MAX_AF
RDS_NO_BURST = 0xFFFFFFFF  # FMRX_RDS_NO_BURST: a burst table entry without a pattern
# fmrx_rds_block_rec as a numpy record: an accepted block of the RDS block sync
RDS_BLOCK = np.dtype([("bit", "<u8"), ("info", "<u2"), ("slot", "u1"), ("c_prime", "u1"), ("corrected", "u1"),
                      ("votes", "u1"), ("pad", "u1", (2,))])


class RdsSyncConfig(C.Structure):
    """fmrx_rds_sync_config: the block sync's constants (defaults 8, 3, 2)."""
    _fields_ = [("J", C.c_int), ("V", C.c_int), ("B", C.c_int)]


class _RdsBlockRec(C.Structure):
    _fields_ = [("bit", C.c_uint64), ("info", C.c_uint16), ("slot", C.c_uint8), ("c_prime", C.c_uint8),
                ("corrected", C.c_uint8), ("votes", C.c_uint8), ("pad", C.c_uint8 * 2)]


class RdsExt(C.Structure):
    """Mirror of fmrx_rds_ext: what the block-wise RDS parser has read so far."""
    _fields_ = [("bits", C.c_uint64), ("exact_blocks", C.c_uint64), ("corrected_blocks", C.c_uint64),
                ("groups", C.c_uint64), ("partial_groups", C.c_uint64), ("pi", C.c_uint16), ("pi_set", C.c_uint8),
                ("pty", C.c_uint8), ("tp", C.c_uint8), ("ta", C.c_uint8), ("ms", C.c_uint8), ("di", C.c_uint8),
                ("rt_ab", C.c_uint8), ("ptyn_ab", C.c_uint8), ("ps_sure", C.c_uint8), ("ptyn_sure", C.c_uint8),
                ("rt_sure", C.c_uint64), ("af_n", C.c_uint8), ("af_count", C.c_uint8),
                ("af_raw", C.c_uint8 * RDS_MAX_AF), ("ct_set", C.c_uint8), ("ct_hour", C.c_uint8),
                ("ct_minute", C.c_uint8), ("ct_month", C.c_uint8), ("ct_day", C.c_uint8), ("ct_offset", C.c_int8),
                ("ct_year", C.c_uint16), ("ct_mjd", C.c_uint32), ("ps_raw", C.c_char * 9), ("rt_raw", C.c_char * 65),
                ("ptyn_raw", C.c_char * 9), ("tail_n", C.c_uint8), ("tail_done", C.c_uint8 * RDS_EXT_TAIL),
                ("tail", _RdsBlockRec * RDS_EXT_TAIL)]

    def __init__(self):
        super().__init__()
        _check(lib().fmrx_rds_ext_init(C.byref(self)))

    @property
    def ps(self) -> str:
        return self.ps_raw.decode("ascii")

    @property
    def rt(self) -> str:
        return self.rt_raw.decode("ascii")

    @property
    def ptyn(self) -> str:
        return self.ptyn_raw.decode("ascii")

    @property
    def af(self) -> list:
        """The alternative frequencies in MHz, in order of first appearance."""
        return [round(87.5 + 0.1 * self.af_raw[k], 1) for k in range(self.af_n)]

    @property
    def ct(self) -> dict | None:
        """The last clock time as fields (offset: the local time offset in half hours), None before one."""
        if not self.ct_set:
            return None
        return {"mjd": self.ct_mjd, "year": self.ct_year, "month": self.ct_month, "day": self.ct_day,
                "hour": self.ct_hour, "minute": self.ct_minute, "offset": self.ct_offset}

    def as_dict(self) -> dict:
        return {"pi": self.pi if self.pi_set else None, "pty": self.pty, "tp": self.tp, "ta": self.ta, "ms": self.ms,
                "di": self.di, "ps": self.ps, "rt": self.rt, "ptyn": self.ptyn, "af": self.af, "af_count": self.af_count,
                "ct": self.ct, "bits": self.bits, "exact_blocks": self.exact_blocks,
                "corrected_blocks": self.corrected_blocks, "groups": self.groups, "partial_groups": self.partial_groups}


METER_TONES = 7  # include/fmrx.h FMRX_METER_TONES
METER_TONES_KHZ = (17, 19, 21, 56, 58, 61, 63)
METER_WINDOWS = 64  # 1 ms windows a frame


class MeterReport(C.Structure):
    """fmrx_meter_report: a stream's summed tone powers and the frames they cover."""
    _fields_ = [("sum", C.c_double * METER_TONES), ("frames", C.c_uint64)]


class MeterConfig(C.Structure):
    """fmrx_meter_config: the decision's two thresholds in dB."""
    _fields_ = [("pilot_min_snr_db", C.c_float), ("rds_min_snr_db", C.c_float)]


class Subcarriers(C.Structure):
    """fmrx_subcarriers: what fmrx_meter_detect says of a report."""
    _fields_ = [("pilot_db", C.c_float), ("pilot_snr_db", C.c_float), ("rds_db", C.c_float), ("rds_snr_db", C.c_float),
                ("stereo", C.c_int), ("rds", C.c_int)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


BLEND_STEPS = 16  # thresholds of soft stereo; a level is 0 .. 16
BLEND_CARRY = 8   # floats of carry a stream (include/fmrx.h: a and g of the last three frames, the level, 0)
BLEND_PER = 4     # csrc/fmrx_internal.h kBlendPer: consecutive (right, left) frames a lane of the apply kernel


class BlendConfig(C.Structure):
    """fmrx_blend_config: the pilot signal-to-noise ratios (dB) of level 1 and of level 16."""
    _fields_ = [("lo_db", C.c_float), ("hi_db", C.c_float)]


class BlendReport(C.Structure):
    """fmrx_blend_report: a stream's meter frames, and how many of them sat at each level 0 .. 16."""
    _fields_ = [("frames", C.c_uint64), ("level_frames", C.c_uint64 * (BLEND_STEPS + 1))]


QUIET_STEPS = 16  # thresholds of the high-cut and of the soft mute; a level is 0 .. 16
QUIET_CARRY = 8   # floats of carry a stream (include/fmrx.h: n of the last three frames, the last c and m, three zeros)
QUIET_HIST = 63   # inputs of history a stream and channel


class QuietConfig(C.Structure):
    """fmrx_quiet_config: the readings (dB) between which the high-cut and the soft mute close, the mute's depth
    (dB) and the high-cut's corner (Hz)."""
    _fields_ = [("cut_lo_db", C.c_float), ("cut_hi_db", C.c_float), ("mute_lo_db", C.c_float), ("mute_hi_db", C.c_float),
                ("mute_depth_db", C.c_float), ("corner_hz", C.c_int)]


class QuietReport(C.Structure):
    """fmrx_quiet_report: a stream's meter frames, and how many of them sat at each cut and mute level 0 .. 16."""
    _fields_ = [("frames", C.c_uint64), ("cut_frames", C.c_uint64 * (QUIET_STEPS + 1)), ("mute_frames", C.c_uint64 * (QUIET_STEPS + 1))]


class CarrierReport(C.Structure):
    """fmrx_carrier_report: a stream's summed demod samples and squares and the frames they cover."""
    _fields_ = [("sum", C.c_double), ("sumsq", C.c_double), ("frames", C.c_uint64)]


class AfcConfig(C.Structure):
    """fmrx_afc_config: the decision's grid, deadband, reach, window, the tracking switch and the carrier gate."""
    _fields_ = [("step_hz", C.c_int), ("deadband_hz", C.c_int), ("max_pull_hz", C.c_int), ("frames", C.c_int),
                ("track", C.c_int), ("max_mean_square", C.c_float)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class AfcDecision(C.Structure):
    """fmrx_afc_decision: what fmrx_afc_decide says of a report."""
    _fields_ = [("err_hz", C.c_double), ("mean", C.c_double), ("mean_square", C.c_double), ("carrier", C.c_int),
                ("correction_hz", C.c_int32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class AfcStatus(C.Structure):
    """fmrx_afc_status: a stream's total report, where it was tuned and where it is, its counts and last decision."""
    _fields_ = [("total", CarrierReport), ("origin_hz", C.c_int32), ("offset_hz", C.c_int32), ("retunes", C.c_uint32),
                ("refused", C.c_uint32), ("decisions", C.c_uint32), ("last", AfcDecision)]


_vp, _sz, _fp, _i16p, _u8p =C.c_void_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_uint8)

# name -> (restype, argtypes); every function declared in include/fmrx.h
PROTOTYPES = {
    "fmrx_config_default": (C.c_int, [C.POINTER(Config), C.c_int, C.c_int]),
    "fmrx_geometry": (C.c_int, [C.POINTER(Config), C.POINTER(Geometry)]),
    "fmrx_create": (C.c_int, [C.POINTER(Config), C.POINTER(_vp)]),
    "fmrx_destroy": (None, [_vp]),
    "fmrx_reset": (C.c_int, [_vp]),
    "fmrx_last_error": (C.c_char_p, []),
    "fmrx_version": (C.c_char_p, []),
    "fmrx_state_size": (C.c_int, [_vp, C.POINTER(_sz)]),
    "fmrx_get_state": (C.c_int, [_vp, _vp, _sz]),
    "fmrx_set_state": (C.c_int, [_vp, _vp, _sz]),
    "fmrx_history_bytes": (C.c_int, [_vp, C.POINTER(_sz)]),
    "fmrx_seek": (C.c_int, [_vp, _vp, _sz, C.c_int]),
    "fmrx_process": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_rf_block": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_audio_block": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_rds_block": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "fmrx_rds_device": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "fmrx_rds_granule": (C.c_int, [_vp, C.POINTER(_sz)]),
    "fmrx_rds_bits": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "fmrx_rds_bits_device": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "fmrx_rds_info_init": (C.c_int, [C.POINTER(RdsInfo)]),
    "fmrx_rds_parse": (C.c_int, [C.POINTER(RdsInfo), _vp, _vp, _sz]),
    "fmrx_rds_decode": (C.c_int, [_vp, _vp, _sz]),
    "fmrx_rds_decode_device": (C.c_int, [_vp, _vp, _sz]),
    "fmrx_rds_info_get": (C.c_int, [_vp, C.c_int, C.POINTER(RdsInfo)]),
    "fmrx_set_rds": (C.c_int, [_vp, C.c_int]),
    "fmrx_rds_sync_config_default": (C.c_int, [C.POINTER(RdsSyncConfig)]),
    "fmrx_rds_sync_design": (C.c_int, [C.c_int, _vp, C.POINTER(C.c_int)]),
    "fmrx_rds_blocks": (C.c_int, [_vp, C.POINTER(RdsSyncConfig), _vp, _sz, _vp, _sz, _vp]),
    "fmrx_rds_blocks_device": (C.c_int, [_vp, C.POINTER(RdsSyncConfig), _vp, _sz, _vp, _sz, _vp]),
    "fmrx_rds_blocks_flush": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_rds_ext_init": (C.c_int, [C.POINTER(RdsExt)]),
    "fmrx_rds_parse_blocks": (C.c_int, [C.POINTER(RdsExt), _vp, _sz, C.c_uint64, C.c_int]),
    "fmrx_set_rds_sync": (C.c_int, [_vp, C.c_int]),
    "fmrx_rds_ext_get": (C.c_int, [_vp, C.c_int, C.POINTER(RdsExt)]),
    "fmrx_fm_demod_arctan": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int]),
    "fmrx_estimate_psd": (C.c_int, [_vp, _vp, _sz, C.c_int, C.c_float, _vp, _vp]),
    "fmrx_psd_device": (C.c_int, [_vp, _vp, _sz, C.c_int, C.c_float, _vp]),
    "fmrx_process_device": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_process_device_ex": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "fmrx_tuner_design": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _vp]),
    "fmrx_tune": (C.c_int, [_vp, _vp, C.c_uint64]),
    "fmrx_tuner_info": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "fmrx_process_shared": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_process_shared_device": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_iq_pair_bytes": (C.c_int, [C.c_int]),
    "fmrx_set_input_format": (C.c_int, [_vp, C.c_int]),
    "fmrx_input_format": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "fmrx_scan_config_default": (C.c_int, [C.POINTER(ScanConfig)]),
    "fmrx_scan_spectrum": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, C.POINTER(_sz)]),
    "fmrx_scan_spectrum_device": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp]),
    "fmrx_scan_detect": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(ScanConfig), C.POINTER(Station), C.c_int,
                                   C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "fmrx_scan": (C.c_int, [_vp, _vp, _sz, C.POINTER(ScanConfig), C.POINTER(Station), C.c_int, C.POINTER(C.c_int)]),
    "fmrx_wide_design": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int), _vp, C.POINTER(C.c_int), _vp]),
    "fmrx_set_capture_decim": (C.c_int, [_vp, C.c_int]),
    "fmrx_capture_decim": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "fmrx_tune_wide": (C.c_int, [_vp, _vp, C.c_uint64]),
    "fmrx_wide_info": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "fmrx_process_wide": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_process_wide_device": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_scan_detect_wide": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(ScanConfig), C.POINTER(Station), C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "fmrx_scan_wide": (C.c_int, [_vp, _vp, _sz, C.POINTER(ScanConfig), C.POINTER(Station), C.c_int, C.POINTER(C.c_int)]),
    "fmrx_rate_design": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 6 + [_vp, C.POINTER(C.c_int), _vp]),
    "fmrx_set_capture_rate": (C.c_int, [_vp, C.c_int]),
    "fmrx_capture_rate": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "fmrx_wide_granule": (C.c_int, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "fmrx_scan_detect_rate": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(ScanConfig), C.POINTER(Station), C.c_int,
                                        C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "fmrx_deemph_design": (C.c_int, [C.c_int, C.c_int, _vp]),
    "fmrx_set_deemphasis": (C.c_int, [_vp, C.c_int]),
    "fmrx_deemphasis": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "fmrx_deemph": (C.c_int, [_vp, _vp, _sz, C.c_int, _vp, _vp, _vp]),
    "fmrx_meter_design": (C.c_int, [C.c_int, C.POINTER(C.c_int), _vp]),
    "fmrx_meter": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_meter_device": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_meter_config_default": (C.c_int, [C.POINTER(MeterConfig)]),
    "fmrx_meter_accumulate": (C.c_int, [C.POINTER(MeterReport), _vp, _sz]),
    "fmrx_meter_detect": (C.c_int, [C.POINTER(MeterReport), C.POINTER(MeterConfig), C.POINTER(Subcarriers)]),
    "fmrx_set_meter": (C.c_int, [_vp, C.c_int]),
    "fmrx_meter_get": (C.c_int, [_vp, C.c_int, C.POINTER(MeterReport)]),
    "fmrx_blend_config_default": (C.c_int, [C.POINTER(BlendConfig)]),
    "fmrx_blend_design": (C.c_int, [C.POINTER(BlendConfig), _vp]),
    "fmrx_blend_levels": (C.c_int, [_vp, C.POINTER(BlendConfig), _vp, _sz, _vp, _vp]),
    "fmrx_blend_levels_device": (C.c_int, [_vp, C.POINTER(BlendConfig), _vp, _sz, _vp, _vp]),
    "fmrx_blend_apply_device": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp]),
    "fmrx_set_stereo_blend": (C.c_int, [_vp, C.c_int, C.POINTER(BlendConfig)]),
    "fmrx_stereo_blend": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(BlendConfig)]),
    "fmrx_blend_hold": (C.c_int, [_vp, C.c_int]),
    "fmrx_blend_get": (C.c_int, [_vp, C.c_int, C.POINTER(BlendReport)]),
    "fmrx_quiet_config_default": (C.c_int, [C.POINTER(QuietConfig)]),
    "fmrx_quiet_design": (C.c_int, [C.c_int, C.c_int, C.POINTER(QuietConfig), _vp, _vp, _vp, _vp]),
    "fmrx_quiet_levels": (C.c_int, [_vp, C.POINTER(QuietConfig), _vp, _sz, _vp, _vp]),
    "fmrx_quiet_levels_device": (C.c_int, [_vp, C.POINTER(QuietConfig), _vp, _sz, _vp, _vp]),
    "fmrx_quiet_apply_device": (C.c_int, [_vp, _vp, _sz, _vp, _vp, _vp, _vp]),
    "fmrx_set_quieting": (C.c_int, [_vp, C.c_int, C.POINTER(QuietConfig)]),
    "fmrx_quieting": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(QuietConfig)]),
    "fmrx_quiet_hold": (C.c_int, [_vp, C.c_int]),
    "fmrx_quiet_get": (C.c_int, [_vp, C.c_int, C.POINTER(QuietReport)]),
    "fmrx_carrier": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_carrier_device": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_carrier_accumulate": (C.c_int, [C.POINTER(CarrierReport), _vp, _sz]),
    "fmrx_afc_config_default": (C.c_int, [C.POINTER(AfcConfig)]),
    "fmrx_afc_decide": (C.c_int, [C.POINTER(CarrierReport), C.c_int, C.POINTER(AfcConfig), C.POINTER(AfcDecision)]),
    "fmrx_set_afc": (C.c_int, [_vp, C.POINTER(AfcConfig), C.c_int]),
    "fmrx_afc_get": (C.c_int, [_vp, C.c_int, C.POINTER(AfcStatus)]),
    "fmrx_synchronize": (C.c_int, [_vp]),
    "fmrx_stream": (_vp, [_vp]),
    "fmrx_kernel_timing": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
    "fmrx_impulse_response_lpf": (C.c_int, [_fp, C.c_float, C.c_float, C.c_int, C.c_int]),
    "fmrx_impulse_response_bpf": (C.c_int, [_fp, C.c_float, C.c_float, C.c_float, C.c_int]),
    "fmrx_resample": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "fmrx_fm_demod": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int]),
    "fmrx_pll": (C.c_int, [_vp, _vp, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _vp]),
    "fmrx_mixer": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int]),
    "fmrx_lr_extraction": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int]),
    "fmrx_normalize_iq": (C.c_int, [_vp, _vp, _sz, _vp, _vp]),
    "fmrx_quantize": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmrx_synth_host": (C.c_int, [C.c_uint64, C.c_int, C.c_uint64, _sz, _vp]),
    "fmrx_synth_device": (C.c_int, [_vp, C.c_uint64, C.c_int, C.c_uint64, _sz, _vp]),
    "fmrx_synth_device_streams": (C.c_int, [_vp, _vp, _sz, C.c_int, C.c_uint64, _sz, _vp, _sz]),
    "fmrx_test_pll_fallback": (C.c_int, [_vp, C.c_int, _vp, _vp, _sz, _vp]),
    "fmrx_debug_mono_stamps": (C.c_int, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "fmrx_debug_pll_stats": (C.c_int, [_vp, _vp]),
    "fmrx_debug_set_knob": (C.c_int, [_vp, C.c_int, C.c_double]),
    "fmrx_debug_pll_redos": (C.c_int, [_vp, _vp]),
    "fmrx_debug_stage_timing": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_long), C.c_int]),
}

# fmrx_debug_stage_timing's stage kinds (csrc/fmrx_internal.h StageKind)
STAGES = ["front_end", "bandpass_pair", "pll_prep", "runner_lane", "runner_pred", "runner_sat", "runner_pipe20",
          "runner_pipe21", "runner_pipe22", "pll_check", "pll_tail", "pll_nco", "audio", "runner_idx17", "runner_idx18",
          "runner_idx19", "runner_cnt17", "runner_cnt18", "runner_cnt19", "runner_cnt20", "runner_cnt21", "runner_stick"]

# fmrx_debug_set_knob's knobs (include/fmrx.h FMRX_KNOB_*): none changes the output; the
# pll_inject / pll_pipe_miss / pll_hint_skew test hooks make the PLL runners redo work
KNOBS = {"pll_spec": 0, "pll_sat": 1, "pll_pred": 2, "pll_pipe": 3, "pll_idx": 4, "stereo_chunks": 5,
         "mono_split": 6, "bpf_tile": 7, "halo_kernel": 8, "pll_inject": 9, "pll_pipe_miss": 10,
         "pll_hint_skew": 11, "pll_cnt": 12, "pll_stick": 13, "stereo_head": 14,
         "stereo_lead": 15, "audio_defer": 16, "stereo_tail": 17}
# fmrx_debug_pll_redos's trigOffset ranges (slots r and 4 + r of each stream's 8)
REDO_RANGES = ["[2^17,2^20)", "[2^20,2^21)", "[2^21,2^22)", "[2^22,2^24]"]
REDO_SLOTS = 8
# knobs every new Receiver applies after fmrx_create (tests set it per test, e.g. with
# monkeypatch.setattr; the library itself reads only the tuning knobs' environment variables)
DEFAULT_KNOBS: dict = {}

_lib = None


def header_symbols() -> list[str]:
    """Function names declared in include/fmrx.h."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(fmrx_[a-z0-9_]+)\s*\(", txt)))


def lib() -> C.CDLL:
    """Load libfmrx.so (raises if it is missing: there is no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is not built; run `make -C {PKG_DIR}` "
                              "(the HIP extension is required, there is no CPU path)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc != FMRX_OK:
        raise FmrxError(rc, lib().fmrx_last_error().decode())


def _np_ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def default_config(mode: int = 0, channels: int = MONO, **kw) -> Config:
    cfg = Config()
    _check(lib().fmrx_config_default(C.byref(cfg), mode, channels))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def geometry(cfg: Config) -> Geometry:
    g = Geometry()
    _check(lib().fmrx_geometry(C.byref(cfg), C.byref(g)))
    return g


def lpf(fs: float, fc: float, taps: int, gain: int = 1) -> np.ndarray:
    """impulseResponseLPF (src/filter.cpp:14-37)."""
    h = np.zeros(taps, np.float32)
    _check(lib().fmrx_impulse_response_lpf(h.ctypes.data_as(_fp), fs, fc, taps, gain))
    return h


def bpf(fs: float, fb: float, fe: float, taps: int) -> np.ndarray:
    """impulseResponseBPF (src/filter.cpp:39-64)."""
    h = np.zeros(taps, np.float32)
    _check(lib().fmrx_impulse_response_bpf(h.ctypes.data_as(_fp), fs, fb, fe, taps))
    return h


def tuner_design(rf_fs: int, offset_hz: int) -> tuple[int, int, np.ndarray]:
    """Rotator of a stream tuned to offset_hz (fmrx_tuner_design): (N, k, table), table[p] =
    (c[p], s[p]) as float32, shape (N, 2); pair n of the stream takes entry (k n) mod N."""
    n, k = C.c_int(), C.c_int()
    _check(lib().fmrx_tuner_design(rf_fs, offset_hz, C.byref(n), C.byref(k), None))
    tab = np.zeros((n.value, 2), np.float32)
    _check(lib().fmrx_tuner_design(rf_fs, offset_hz, C.byref(n), C.byref(k), _np_ptr(tab)))
    return n.value, k.value, tab


def wide_design(rf_fs: int, decim: int, offset_hz: int) -> dict:
    """fmrx_wide_design: how an offset against a capture at decim * rf_fs splits and what the
    down-converter runs with.  A dict: coarse_hz, fine_hz, N, k, table (N x 2 float32: c[p], s[p]),
    h (the 16 decim + 1 float32 taps)."""
    fc, fr, n, k, t = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _check(lib().fmrx_wide_design(rf_fs, decim, offset_hz, C.byref(fc), C.byref(fr), C.byref(n), C.byref(k), None,
                                  C.byref(t), None))
    tab, h = np.zeros((n.value, 2), np.float32), np.zeros(t.value, np.float32)
    _check(lib().fmrx_wide_design(rf_fs, decim, offset_hz, None, None, None, None, _np_ptr(tab), None, _np_ptr(h)))
    return {"coarse_hz": fc.value, "fine_hz": fr.value, "N": n.value, "k": k.value, "table": tab, "h": h}


def rate_design(rf_fs: int, cap_fs: int, offset_hz: int) -> dict:
    """fmrx_rate_design: how an offset against a capture at cap_fs = rf_fs * down / up splits and what the
    rational down-converter runs with.  A dict: up, down, coarse_hz, fine_hz, N, k, table (N x 2 float32:
    c[p], s[p]), h (the 16 down + 1 float32 taps; an integer ratio reads up = 1 and wide_design's values)."""
    v = [C.c_int() for _ in range(7)]  # up, down, coarse, fine, N, k, taps
    _check(lib().fmrx_rate_design(rf_fs, cap_fs, offset_hz, *[C.byref(x) for x in v[:6]], None, C.byref(v[6]), None))
    up, down, fc, fr, n, k, t = (x.value for x in v)
    tab, h = np.zeros((n, 2), np.float32), np.zeros(t, np.float32)
    _check(lib().fmrx_rate_design(rf_fs, cap_fs, offset_hz, None, None, None, None, None, None, _np_ptr(tab), None, _np_ptr(h)))
    return {"up": up, "down": down, "coarse_hz": fc, "fine_hz": fr, "N": n, "k": k, "table": tab, "h": h}


DEEMPH_TAPS = 64      # csrc/fmrx_internal.h kDeemphTaps: taps of the de-emphasis FIR (63 floats of carry)
DEEMPH_CHUNK = 1024   # kDeemphChunk: outputs a workgroup of the de-emphasis kernel


def deemph_design(audio_fs: int, tau_us: int) -> np.ndarray:
    """fmrx_deemph_design: the 64 float32 taps of the de-emphasis filter for tau_us (50 or 75) at
    audio_fs S/s.  Host only."""
    h = np.zeros(DEEMPH_TAPS, np.float32)
    _check(lib().fmrx_deemph_design(int(audio_fs), int(tau_us), _np_ptr(h)))
    return h


def meter_design(bp_fs: int) -> tuple[int, np.ndarray]:
    """fmrx_meter_design: (P, tables) of the subcarrier meter at bp_fs; tables float32 of shape (7, 2, P):
    tone, (c, s), sample of the 1 ms window.  Host only."""
    p = C.c_int()
    _check(lib().fmrx_meter_design(int(bp_fs), C.byref(p), None))
    tab = np.zeros((METER_TONES, 2, p.value), np.float32)
    _check(lib().fmrx_meter_design(int(bp_fs), None, _np_ptr(tab)))
    return p.value, tab


def meter_accumulate(power, report: MeterReport | None = None) -> MeterReport:
    """fmrx_meter_accumulate (host only): add one stream's frames x 7 powers to report (a new one when None)."""
    report = MeterReport() if report is None else report
    p = np.ascontiguousarray(power, np.float32).reshape(-1, METER_TONES)
    _check(lib().fmrx_meter_accumulate(C.byref(report), _np_ptr(p), p.shape[0]))
    return report


def meter_detect(report: MeterReport, pilot_min_snr_db: float | None = None, rds_min_snr_db: float | None = None) -> dict:
    """fmrx_meter_detect (host only): levels and flags of a report as a dict (pilot_db, pilot_snr_db, rds_db,
    rds_snr_db, stereo, rds).  A threshold left None keeps fmrx_meter_config_default's (10 and 1.94 dB)."""
    cfg, out = MeterConfig(), Subcarriers()
    _check(lib().fmrx_meter_config_default(C.byref(cfg)))
    if pilot_min_snr_db is not None:
        cfg.pilot_min_snr_db = pilot_min_snr_db
    if rds_min_snr_db is not None:
        cfg.rds_min_snr_db = rds_min_snr_db
    given = pilot_min_snr_db is not None or rds_min_snr_db is not None
    _check(lib().fmrx_meter_detect(C.byref(report), C.byref(cfg) if given else None, C.byref(out)))
    return out.as_dict()


def carrier_accumulate(sums, report: CarrierReport | None = None) -> CarrierReport:
    """fmrx_carrier_accumulate (host only): add one stream's frames x 2 sums to report (a new one when None)."""
    report = CarrierReport() if report is None else report
    p = np.ascontiguousarray(sums, np.float32).reshape(-1, 2)
    _check(lib().fmrx_carrier_accumulate(C.byref(report), _np_ptr(p), p.shape[0]))
    return report


def afc_config_default(**kw) -> AfcConfig:
    """fmrx_afc_config_default, with the fields given (step_hz, deadband_hz, max_pull_hz, frames, track,
    max_mean_square) set."""
    cfg = AfcConfig()
    _check(lib().fmrx_afc_config_default(C.byref(cfg)))
    for k, v in kw.items():
        if k not in dict(AfcConfig._fields_):
            raise TypeError(f"no AFC setting {k!r}")
        setattr(cfg, k, v)
    return cfg


def afc_decide(report: CarrierReport, bp_fs: int, **kw) -> dict:
    """fmrx_afc_decide (host only): err_hz, mean, mean_square, carrier and correction_hz of a report as a
    dict; the settings given replace afc_config_default's."""
    out = AfcDecision()
    _check(lib().fmrx_afc_decide(C.byref(report), int(bp_fs), C.byref(afc_config_default(**kw)) if kw else None, C.byref(out)))
    return out.as_dict()


def blend_config(lo_db: float | None = None, hi_db: float | None = None) -> BlendConfig:
    """fmrx_blend_config_default (10 and 22 dB) with the bounds given replaced."""
    cfg = BlendConfig()
    _check(lib().fmrx_blend_config_default(C.byref(cfg)))
    if lo_db is not None:
        cfg.lo_db = lo_db
    if hi_db is not None:
        cfg.hi_db = hi_db
    return cfg


def blend_design(lo_db: float | None = None, hi_db: float | None = None) -> np.ndarray:
    """fmrx_blend_design: the 16 float32 thresholds of soft stereo (a bound left None keeps its default).
    Host only."""
    T = np.zeros(BLEND_STEPS, np.float32)
    _check(lib().fmrx_blend_design(C.byref(blend_config(lo_db, hi_db)), _np_ptr(T)))
    return T


def quiet_config(**kw) -> QuietConfig:
    """fmrx_quiet_config_default (22, 34, 36, 44, 20 dB and 2500 Hz) with the fields given replaced
    (cut_lo_db, cut_hi_db, mute_lo_db, mute_hi_db, mute_depth_db, corner_hz)."""
    cfg = QuietConfig()
    _check(lib().fmrx_quiet_config_default(C.byref(cfg)))
    names = [f[0] for f in QuietConfig._fields_]
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"quiet_config: no field {k!r}")
        if v is not None:
            setattr(cfg, k, v)
    return cfg


def quiet_design(audio_fs: int, bp_fs: int, **kw) -> dict:
    """fmrx_quiet_design (host only): Tc and Tm (16 float32 each), h (64 float32) and the float32 gains g0, cg,
    cw of quiet_config(**kw) at the audio rate (48000 or 44100) and bp_fs, as a dict."""
    Tc, Tm = np.zeros(QUIET_STEPS, np.float32), np.zeros(QUIET_STEPS, np.float32)
    h, g = np.zeros(QUIET_HIST + 1, np.float32), np.zeros(3, np.float32)
    _check(lib().fmrx_quiet_design(int(audio_fs), int(bp_fs), C.byref(quiet_config(**kw)), _np_ptr(Tc), _np_ptr(Tm), _np_ptr(h), _np_ptr(g)))
    return {"Tc": Tc, "Tm": Tm, "h": h, "g0": g[0], "cg": g[1], "cw": g[2]}


def iq_pair_bytes(fmt: int) -> int:
    """fmrx_iq_pair_bytes: bytes an I/Q pair of the format takes (FmrxError(EINVAL) if unknown)."""
    n = lib().fmrx_iq_pair_bytes(fmt)
    if n < 0:
        _check(n)
    return n


def iq_format_of(a) -> int:
    """The raw I/Q format an array's dtype stands for: uint8, int8, int16, float32, and complex64
    (viewed as float32 pairs).  ValueError for anything else."""
    dt = np.asarray(a).dtype
    if dt == np.complex64:
        return IQ_F32
    for fmt, want in IQ_DTYPES.items():
        if dt == want:
            return fmt
    raise ValueError(f"no raw I/Q format for dtype {dt} (uint8, int8, int16, float32, complex64)")


def _iq_flat(a) -> np.ndarray:
    """a as a contiguous array of its raw format's elements (complex64 as float32 pairs)."""
    a = np.ascontiguousarray(a)
    return a.view(np.float32) if a.dtype == np.complex64 else a


MAX_STATIONS = 256  # stations a scan reports unless max_out says otherwise


def scan_config(**kw) -> ScanConfig:
    """fmrx_scan_config_default with the given fields replaced."""
    cfg = ScanConfig()
    _check(lib().fmrx_scan_config_default(C.byref(cfg)))
    for k, v in kw.items():
        if k not in dict(ScanConfig._fields_):
            raise TypeError(f"no scan setting {k!r}")
        setattr(cfg, k, v)
    return cfg


def _stations(arr, n: int) -> list:
    return [Station(arr[i].offset_hz, arr[i].power_db, arr[i].snr_db) for i in range(n)]


def _station_call(fn, args, max_out: int, cfg: dict, want_floor: bool = False):
    """A call that fills a station list: fn(*args, scan config, list, max_out, &found[, &floor_db])."""
    out = (Station * max(max_out, 1))()
    n, fl = C.c_int(), C.c_float()
    _check(fn(*args, C.byref(scan_config(**cfg)), out, max_out, C.byref(n), *([C.byref(fl)] if want_floor else [])))
    found = _stations(out, min(n.value, max_out))
    return (found, fl.value) if want_floor else found


def scan_detect(power: np.ndarray, rf_fs: int, max_out: int = MAX_STATIONS, **cfg):
    """fmrx_scan_detect on an FFT-shifted linear power spectrum (Receiver.scan_spectrum): (stations
    ascending by offset -- the strongest max_out of those found --, floor_db).  Host only."""
    p = np.ascontiguousarray(power, np.float32).reshape(-1)
    return _station_call(lib().fmrx_scan_detect, (_np_ptr(p), p.size, rf_fs), max_out, cfg, True)


def scan_detect_wide(power: np.ndarray, rf_fs: int, decim: int, max_out: int = MAX_STATIONS, **cfg):
    """fmrx_scan_detect_wide: scan_detect on the spectrum of a capture at decim * rf_fs; every reported
    offset is one fmrx_wide_design accepts.  Host only."""
    p = np.ascontiguousarray(power, np.float32).reshape(-1)
    return _station_call(lib().fmrx_scan_detect_wide, (_np_ptr(p), p.size, rf_fs, decim), max_out, cfg, True)


def scan_detect_rate(power: np.ndarray, rf_fs: int, cap_fs: int, max_out: int = MAX_STATIONS, **cfg):
    """fmrx_scan_detect_rate: scan_detect on the spectrum of a capture at cap_fs Hz for a mode at rf_fs;
    every reported offset is one fmrx_rate_design accepts.  Host only."""
    p = np.ascontiguousarray(power, np.float32).reshape(-1)
    return _station_call(lib().fmrx_scan_detect_rate, (_np_ptr(p), p.size, rf_fs, cap_fs), max_out, cfg, True)


def rds_parse(bits, codes, info: RdsInfo | None = None) -> RdsInfo:
    """fmrx_rds_parse (host only): feed bits and their codes, in pieces of any size, into info (a new
    RdsInfo when None) and return it."""
    info = RdsInfo() if info is None else info
    b = np.ascontiguousarray(bits, np.uint8).reshape(-1)
    c = np.ascontiguousarray(codes, np.uint8).reshape(-1)
    if b.size != c.size:
        raise ValueError("bits and codes differ in length")
    _check(lib().fmrx_rds_parse(C.byref(info), _np_ptr(b), _np_ptr(c), b.size))
    return info


def rds_sync_config(**kw) -> RdsSyncConfig:
    """fmrx_rds_sync_config_default, with the fields given (J, V, B) set."""
    cfg = RdsSyncConfig()
    _check(lib().fmrx_rds_sync_config_default(C.byref(cfg)))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def rds_sync_design(B: int = 2) -> tuple[np.ndarray, int]:
    """fmrx_rds_sync_design (host only): the 1024 burst patterns by syndrome (RDS_NO_BURST: none) and how
    many bursts of length <= B the table holds."""
    tab = np.zeros(1024, np.uint32)
    n = C.c_int(0)
    _check(lib().fmrx_rds_sync_design(int(B), _np_ptr(tab), C.byref(n)))
    return tab, n.value


def rds_parse_blocks(blocks, n_bits: int = 0, ext: RdsExt | None = None, flush: bool = False) -> RdsExt:
    """fmrx_rds_parse_blocks (host only): feed one stream's block records (RDS_BLOCK), in pieces of any size,
    into ext (a new RdsExt when None) and return it; flush=True also closes the open groups."""
    ext = RdsExt() if ext is None else ext
    b = np.ascontiguousarray(blocks, RDS_BLOCK).reshape(-1)
    _check(lib().fmrx_rds_parse_blocks(C.byref(ext), _np_ptr(b), b.size, int(n_bits), int(bool(flush))))
    return ext


PROBE_FRAMES = 16  # frames (64 ms each) decode_stations(probe=True) meters before it decides
AFC_PASSES = 3     # passes over those frames decode_stations(afc=True) makes at most before it decodes


class _Route:
    """How decode_stations reaches a capture, chosen once from the mode, the dtype's format, capture_decim and
    capture_rate: at the mode's own rate (scan, tune, process_shared) or through the down-converter (scan_wide,
    tune_wide, process_wide)."""

    def __init__(self, mode: int, rf_taps: int, fmt: int, capture_decim: int, capture_rate: int | None):
        self.mode, self.rf_taps, self.fmt, self.decim, self.rate = mode, rf_taps, fmt, capture_decim, capture_rate
        self.wide = capture_decim != 1 or capture_rate is not None
        self.rf_fs = geometry(default_config(mode)).rf_fs
        self.cap_fs = capture_decim * self.rf_fs if capture_rate is None else capture_rate

    @contextmanager
    def open(self, channels: int, offsets=None):
        """A context set to the capture's format and rate; with offsets, a stream tuned to each."""
        with Receiver(self.mode, channels, rf_taps=self.rf_taps, n_streams=len(offsets) if offsets else 1) as rx:
            if self.fmt != IQ_U8:
                rx.set_input_format(self.fmt)
            if self.rate is not None:
                rx.set_capture_rate(self.rate)
            elif self.wide:
                rx.set_capture_decim(self.decim)
            if offsets:
                (rx.tune_wide if self.wide else rx.tune)(offsets)
            yield rx

    def scan(self, rx: Receiver, iq: np.ndarray, **cfg) -> list:
        return (rx.scan_wide if self.wide else rx.scan)(iq, **cfg)

    def process(self, rx: Receiver, iq: np.ndarray) -> np.ndarray:
        return (rx.process_wide if self.wide else rx.process_shared)(iq).reshape(rx.n_streams, -1)

    def granule(self, rx: Receiver) -> int:
        """Elements of the capture an RDS granule (whole frames) takes."""
        blocks, pairs = rx.wide_granule if self.wide else (1, rx.geo.iq_pairs)
        return rx.rds_granule // blocks * pairs * 2

    def accepts(self, hz: int) -> bool:
        """Whether the tuner's design takes the offset."""
        try:
            rate_design(self.rf_fs, self.cap_fs, hz) if self.wide else tuner_design(self.rf_fs, hz)
            return True
        except FmrxError:
            return False


class _Run(NamedTuple):
    """What one context's run yields: the PCM, a row a stream, and a list with an entry a stream of each
    product that was on (None: off)."""
    pcm: np.ndarray
    infos: list | None = None
    levels: list | None = None
    blends: list | None = None
    decided: list | None = None
    quiets: list | None = None


def _leading_pass(route: _Route, iq: np.ndarray, offsets: list, meter: bool, measure: bool) -> _Run | None:
    """A mono context over the capture's leading whole frames, PROBE_FRAMES at most, with the subcarrier meter
    (levels) and/or the measure-only AFC (decided) on; None when the capture holds no whole frame."""
    with route.open(MONO, offsets) as rx:
        per = route.granule(rx)
        frames = rx.rds_granule * rx.geo.if_samples // (METER_WINDOWS * (rx.geo.bp_fs // 1000))  # a granule's
        n = min(iq.size // per, max(1, PROBE_FRAMES // frames))
        if n == 0:
            return None
        if meter:
            rx.set_meter(True)
        if measure:
            rx.set_afc(True, track=0)
        pcm, streams = route.process(rx, iq[: n * per]), range(len(offsets))
        return _Run(pcm, levels=[meter_detect(rx.meter_report(k)) for k in streams] if meter else None,
                    decided=[afc_decide(rx.afc_status(k).total, rx.geo.bp_fs) for k in streams] if measure else None)


def _afc_passes(route: _Route, iq: np.ndarray, stations: list, probe: bool):
    """Up to AFC_PASSES leading passes that move every station by afc_decide's correction, within max_pull_hz
    of where the scan found it and only to offsets the route accepts, until none moves: (the last pass, which
    with probe carries the levels too, or None; pulls, a dict a station or None)."""
    found, reach = [s.offset_hz for s in stations], afc_config_default().max_pull_hz
    last = None
    for _ in range(AFC_PASSES):
        last = _leading_pass(route, iq, [s.offset_hz for s in stations], meter=probe, measure=True)
        moved = False
        for s, f, d in zip(stations, found, last.decided if last else ()):
            to = min(f + reach, max(f - reach, s.offset_hz + d["correction_hz"]))
            if to != s.offset_hz and route.accepts(to):
                s.offset_hz, moved = to, True
        if not moved:
            break
    if last is None:
        return None, [None] * len(stations)
    return last, [{"err_hz": d["err_hz"], "mean_square": d["mean_square"], "carrier": d["carrier"], "pulled_hz": s.offset_hz - f}
                  for s, f, d in zip(stations, found, last.decided)]


def _grouped_decode(route: _Route, iq: np.ndarray, offsets: list, channels: int, rds: bool, levels: list | None,
                    rds_sync: bool, blend: bool, deemphasis_us: int, quiet: bool = False) -> _Run:
    """The full decode, one context a group of stations: stereo where channels asks for it, RDS where rds
    does, and with levels each only where the station's meter found the subcarrier (mono PCM then duplicated
    into R and L, None in infos and blends).  One group runs in the calling thread; several run side by side, a
    thread each (a context has a stream of its own and the library's calls release the GIL), so that their
    serial PLL chains overlap as they do inside one context."""
    groups: dict = {}
    for k in range(len(offsets)):
        stereo = channels == STEREO and (levels is None or bool(levels[k]["stereo"]))
        groups.setdefault((stereo, rds and (levels is None or bool(levels[k]["rds"]))), []).append(k)

    def decode(group) -> _Run:
        (stereo, with_rds), sel = group
        with route.open(STEREO if stereo else MONO, [offsets[k] for k in sel]) as rx:
            if deemphasis_us:
                rx.set_deemphasis(deemphasis_us)
            per = route.granule(rx) if rds or blend or quiet else 1  # rds, blend, quiet: whole RDS granules of the capture
            if with_rds:
                rx.set_rds(True)
                rx.set_rds_sync(rds_sync)
            if blend and stereo:
                rx.set_stereo_blend(True)
            if quiet:
                rx.set_quieting(True)
            pcm, streams = route.process(rx, iq[: iq.size // per * per]), range(len(sel))
            if with_rds and rds_sync:
                rx.rds_blocks_flush()
            return _Run(pcm if stereo or channels != STEREO else np.repeat(pcm, 2, axis=1),
                        infos=[(rx.rds_ext if rds_sync else rx.rds_info)(k).as_dict() for k in streams] if with_rds else None,
                        blends=[rx.blend_report(k) for k in streams] if blend and stereo else None,
                        quiets=[rx.quiet_report(k) for k in streams] if quiet else None)

    if len(groups) == 1:
        runs = [decode(group) for group in groups.items()]
    else:
        with ThreadPoolExecutor(max_workers=len(groups)) as pool:
            runs = list(pool.map(decode, groups.items()))
    pcm, infos, blends, quiets = ([None] * len(offsets) for _ in range(4))
    for sel, run in zip(groups.values(), runs):
        for i, k in enumerate(sel):
            pcm[k], infos[k], blends[k] = run.pcm[i], run.infos and run.infos[i], run.blends and run.blends[i]
            quiets[k] = run.quiets and run.quiets[i]
    return _Run(np.stack(pcm), infos, levels or [None] * len(offsets), blends, quiets=quiets)


def _stations_result(stations: list, run: _Run, pulls: list, rds: bool, probe: bool, blend: bool, afc: bool, quiet: bool = False) -> tuple:
    """decode_stations' result, and the one place that states its order:
    (stations, pcm[, infos if rds][, levels if probe][, blends if blend][, pulls if afc][, quiets if quiet])."""
    parts = ((True, stations), (True, run.pcm), (rds, run.infos), (probe, run.levels), (blend, run.blends), (afc, pulls),
             (quiet, run.quiets))
    return tuple(part for wanted, part in parts if wanted)


def decode_stations(iq: np.ndarray, mode: int = 0, channels: int = MONO, rf_taps: int = 51, capture_decim: int = 1,
                    capture_rate: int | None = None, rds: bool = False, deemphasis_us: int = 0, probe: bool = False,
                    rds_sync: bool = False, blend: bool = False, afc: bool = False, quiet: bool = False, **cfg):
    """Decode everything in a capture: scan it, tune one stream to every station found and run
    process_shared over its whole blocks.  Returns (stations, pcm), pcm one row a station (S16);
    ([], an empty array) when the scan finds none.  capture_decim > 1: the capture is at
    capture_decim times the mode's rate (scan_wide, tune_wide, process_wide).  capture_rate=HZ: the
    capture's rate in Hz instead (set_capture_rate; whole granules are decoded); giving both is a
    ValueError.  rds=True: the capture is trimmed to whole RDS granules and the result is
    (stations, pcm, infos), infos one dict a station (pi, pty, tp, ps, rt and the parser's counters).
    deemphasis_us=50 or 75: the PCM is de-emphasised (set_deemphasis; 0, the default: as broadcast).
    probe=True: a mono pass with the subcarrier meter on (set_meter) over the capture's leading whole
    frames, PROBE_FRAMES of them at most, first says which stations carry a pilot and an RDS subcarrier;
    the stations are then decoded in one context a group (the groups side by side, a thread each): stereo only with a pilot (a station without one
    under channels=STEREO returns its mono PCM duplicated into R and L), RDS only with the subcarrier
    (None in infos otherwise).  The result gains a trailing list, levels: meter_detect's dict a station
    (None where the capture holds no whole frame: everything is then decoded as without probe).
    rds_sync=True (with rds=True; a ValueError without): the block sync runs behind the bits (set_rds_sync) and
    is flushed at the end, and infos holds RdsExt.as_dict()'s extended dict a station instead.
    blend=True (with channels=STEREO; a ValueError without): soft stereo (set_stereo_blend, the default
    thresholds) blends every station decoded in stereo toward mono by its pilot; the capture is trimmed to whole
    RDS granules and the result gains a last list, blends: Receiver.blend_report's dict a station (None for a
    station that probe=True routed to mono, which stays mono).
    afc=True: after the scan, up to AFC_PASSES mono passes over the same leading frames with the measure-only
    AFC switch (set_afc(track=0)) move every station by afc_decide's correction (the default configuration;
    within max_pull_hz of the scan's offset, and only to offsets the tuner's design accepts) and stop early when
    none moves; with probe=True the last of them is the probe's pass too.  The stations returned carry the
    corrected offset_hz, everything is decoded there, and the result gains a last list after the probe's and
    the blend's: a dict a station (err_hz, mean_square and carrier of its last measurement, pulled_hz against
    the scan's offset), None where the capture holds no whole frame (decoded as without afc).
    quiet=True (either channel count): quieting (set_quieting, the default configuration) rolls off the treble
    and turns down the audio of every station by its noise level; the capture is trimmed to whole RDS granules
    and the result gains a last list after all the others, quiets: Receiver.quiet_report's dict a station."""
    if rds_sync and not rds:
        raise ValueError("rds_sync needs rds")
    if blend and channels != STEREO:
        raise ValueError("blend needs channels=STEREO")
    if capture_rate is not None and capture_decim != 1:
        raise ValueError("capture_rate and capture_decim exclude each other")
    route = _Route(mode, rf_taps, iq_format_of(iq), capture_decim, capture_rate)  # the dtype says which raw format
    iq = _iq_flat(iq).reshape(-1)
    want = dict(rds=rds, probe=probe, blend=blend, afc=afc, quiet=quiet)
    with route.open(channels) as rx:
        stations = route.scan(rx, iq, **cfg)
    if not stations:
        return _stations_result([], _Run(np.zeros((0, 0), np.int16), [], [], [], quiets=[]), [], **want)
    lead, pulls = None, None
    if afc:
        lead, pulls = _afc_passes(route, iq, stations, probe)
    elif probe:
        lead = _leading_pass(route, iq, [s.offset_hz for s in stations], meter=True, measure=False)
    run = _grouped_decode(route, iq, [s.offset_hz for s in stations], channels, rds, lead.levels if lead else None,
                          rds_sync, blend, deemphasis_us, quiet)
    return _stations_result(stations, run, pulls, **want)


def synth_host(seed: int, rf_fs: int, first_pair: int, n_pairs: int) -> np.ndarray:
    out = np.zeros(2 * n_pairs, np.uint8)
    _check(lib().fmrx_synth_host(seed, rf_fs, first_pair, n_pairs, _np_ptr(out)))
    return out


class Receiver:
    """One libfmrx context: ``n_streams`` independent IQ streams on one GPU.

    Host-buffer methods mirror the reference's block loop; ``*_device`` methods take
    device pointers (e.g. ``torch.Tensor.data_ptr()``) and enqueue on the context stream.
    """

    def __init__(self, mode: int = 0, channels: int = MONO, rf_taps: int = 51, n_streams: int = 1,
                 device: int = 0, bp_taps: int = 51, audio_taps: int = 51, knobs: dict | None = None):
        self.cfg = default_config(mode, channels, rf_taps=rf_taps, n_streams=n_streams,
                                  device=device, bp_taps=bp_taps, audio_taps=audio_taps)
        self.geo = geometry(self.cfg)
        h = C.c_void_p()
        _check(lib().fmrx_create(C.byref(self.cfg), C.byref(h)))
        self.h = h
        self.n_streams = n_streams
        self.channels = channels
        for k, v in {**DEFAULT_KNOBS, **(knobs or {})}.items():
            self.set_knob(k, v)

    def set_knob(self, name: str, value: float) -> None:
        """fmrx_debug_set_knob (include/fmrx.h FMRX_KNOB_*; KNOBS names them)."""
        _check(lib().fmrx_debug_set_knob(self.h, KNOBS[name], float(value)))

    def close(self) -> None:
        if getattr(self, "h", None):
            lib().fmrx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- sizes
    @property
    def block_bytes(self) -> int:
        """Bytes of a block of raw I/Q in the context's input format (geo.block_bytes for u8)."""
        return self.geo.iq_pairs * self._pair_bytes

    def n_blocks(self, n_bytes_per_stream: int) -> int:
        return n_bytes_per_stream // self.block_bytes

    # ---- raw I/Q format
    _fmt, _pair_bytes = IQ_U8, 2

    def set_input_format(self, fmt: int) -> None:
        """fmrx_set_input_format: the raw format of every stream (IQ_U8 .. IQ_F32), then a reset."""
        _check(lib().fmrx_set_input_format(self.h, int(fmt)))
        self._fmt, self._pair_bytes = int(fmt), iq_pair_bytes(int(fmt))

    @property
    def input_format(self) -> int:
        f = C.c_int()
        _check(lib().fmrx_input_format(self.h, C.byref(f)))
        return f.value

    def _raw(self, iq) -> np.ndarray:
        """iq as a contiguous array of the context's format's elements, two a pair.  u8 contexts
        convert as they always did; any other format takes arrays of its own dtype only."""
        if self._fmt == IQ_U8:
            dt = getattr(iq, "dtype", None)
            if dt is not None and dt != np.uint8 and (dt == np.complex64 or dt in IQ_DTYPES.values()):
                raise FmrxError(FMRX_EINVAL, f"array of dtype {dt} for a u8 context (set_input_format first)")
            return np.ascontiguousarray(iq, np.uint8)
        a = _iq_flat(iq)
        if a.dtype != IQ_DTYPES[self._fmt]:
            raise FmrxError(FMRX_EINVAL, f"array of dtype {a.dtype} for input format {self._fmt} "
                                         f"({IQ_DTYPES[self._fmt]})")
        return a

    # ---- host entry points
    def _streams(self, iq: np.ndarray) -> tuple[np.ndarray, int]:
        iq = self._raw(iq).reshape(self.n_streams, -1)
        per = 2 * self.geo.iq_pairs  # elements a block
        nb = iq.shape[1] // per
        return np.ascontiguousarray(iq[:, : nb * per]), nb

    def process(self, iq: np.ndarray) -> np.ndarray:
        """Full blocks of raw I/Q of the context's format (per stream; u8 unless set_input_format
        said otherwise) -> S16 PCM (R,L interleaved for stereo)."""
        iq, nb = self._streams(iq)
        out = np.zeros((self.n_streams, nb * self.geo.pcm_samples), np.int16)
        if nb:
            _check(lib().fmrx_process(self.h, _np_ptr(iq), nb, _np_ptr(out)))
        return out if self.n_streams > 1 else out[0]

    def rf_block(self, iq: np.ndarray) -> np.ndarray:
        """rf_thread body (project.cpp:48-70): u8 I/Q -> demod floats."""
        iq, nb = self._streams(iq)
        out = np.zeros((self.n_streams, nb * self.geo.if_samples), np.float32)
        if nb:
            _check(lib().fmrx_rf_block(self.h, _np_ptr(iq), nb, _np_ptr(out)))
        return out if self.n_streams > 1 else out[0]

    def audio_block(self, demod: np.ndarray) -> np.ndarray:
        """audio_thread body (project.cpp:132-195): demod floats -> S16."""
        d = np.ascontiguousarray(demod, np.float32).reshape(self.n_streams, -1)
        nb = d.shape[1] // self.geo.if_samples
        out = np.zeros((self.n_streams, nb * self.geo.pcm_samples), np.int16)
        if nb:
            _check(lib().fmrx_audio_block(self.h, _np_ptr(d), nb, _np_ptr(out)))
        return out if self.n_streams > 1 else out[0]

    def rds_block(self, demod: np.ndarray, want_nco: bool = False, want_channel: bool = False):
        """rds_thread body (project.cpp:200-271): demod floats -> RDS mixer output (and
        optionally the PLL output and the 54-60 kHz channel).  Returns a dict of arrays."""
        d = np.ascontiguousarray(demod, np.float32).reshape(self.n_streams, -1)
        nb = d.shape[1] // self.geo.if_samples
        n = nb * self.geo.if_samples
        d = np.ascontiguousarray(d[:, :n])
        out = {"rds": np.zeros((self.n_streams, n), np.float32)}
        if want_nco:
            out["nco"] = np.zeros((self.n_streams, n), np.float32)
        if want_channel:
            out["channel"] = np.zeros((self.n_streams, n), np.float32)
        if nb:
            _check(lib().fmrx_rds_block(self.h, _np_ptr(d), nb, _np_ptr(out["rds"]),
                                        _np_ptr(out["nco"]) if want_nco else None,
                                        _np_ptr(out["channel"]) if want_channel else None))
        return {k: (v if self.n_streams > 1 else v[0]) for k, v in out.items()}

    def rds_device(self, d_demod: int, n_blocks: int, d_rds: int, d_nco: int | None = None,
                   d_channel: int | None = None) -> None:
        _check(lib().fmrx_rds_device(self.h, d_demod, n_blocks, d_rds, d_nco, d_channel))

    # ---- RDS back half
    @property
    def rds_granule(self) -> int:
        """fmrx_rds_granule: the blocks an RDS call takes whole multiples of."""
        b = _sz()
        _check(lib().fmrx_rds_granule(self.h, C.byref(b)))
        return b.value

    def rds_bits(self, rds: np.ndarray, want_y: bool = False) -> dict:
        """fmrx_rds_bits: the mixer rows (rds_block's "rds"; whole RDS granules) -> a dict of bits and codes
        (76 a window, one byte each), win (windows x (p, q)) and, with want_y, the 38 kS/s samples y."""
        d = np.ascontiguousarray(rds, np.float32).reshape(self.n_streams, -1)
        nb = d.shape[1] // self.geo.if_samples
        if nb * self.geo.if_samples != d.shape[1]:
            raise FmrxError(FMRX_EINVAL, "rds_bits takes whole blocks")
        n_out = d.shape[1] * 19 // (self.geo.bp_fs // 2000)
        nw = n_out // RDS_WINDOW
        out = {"bits": np.zeros((self.n_streams, nw * RDS_BITS_PER_WINDOW), np.uint8),
               "codes": np.zeros((self.n_streams, nw * RDS_BITS_PER_WINDOW), np.uint8),
               "win": np.zeros((self.n_streams, nw, 2), np.uint8)}
        if want_y:
            out["y"] = np.zeros((self.n_streams, n_out), np.float32)
        _check(lib().fmrx_rds_bits(self.h, _np_ptr(d), nb, _np_ptr(out["bits"]), _np_ptr(out["codes"]),
                                   _np_ptr(out["win"]), _np_ptr(out["y"]) if want_y else None))
        return {k: (v if self.n_streams > 1 else v[0]) for k, v in out.items()}

    def rds_bits_device(self, d_rds: int, n_blocks: int, d_bits: int | None, d_codes: int | None,
                        d_win: int | None = None, d_y: int | None = None) -> None:
        _check(lib().fmrx_rds_bits_device(self.h, d_rds, n_blocks, d_bits, d_codes, d_win, d_y))

    def rds_decode(self, demod: np.ndarray) -> None:
        """fmrx_rds_decode: demod blocks (whole RDS granules) through the front half, the bits and the
        parser into the streams' info (rds_info)."""
        d = np.ascontiguousarray(demod, np.float32).reshape(self.n_streams, -1)
        nb = d.shape[1] // self.geo.if_samples
        if nb * self.geo.if_samples != d.shape[1]:
            raise FmrxError(FMRX_EINVAL, "rds_decode takes whole blocks")
        _check(lib().fmrx_rds_decode(self.h, _np_ptr(d), nb))

    def rds_decode_device(self, d_demod: int, n_blocks: int) -> None:
        _check(lib().fmrx_rds_decode_device(self.h, d_demod, n_blocks))

    def set_rds(self, on: bool) -> None:
        """fmrx_set_rds: the tuned, shared and wide process calls also decode RDS (whole RDS granules)."""
        _check(lib().fmrx_set_rds(self.h, int(bool(on))))

    def rds_info(self, stream: int = 0) -> RdsInfo:
        info = RdsInfo()
        _check(lib().fmrx_rds_info_get(self.h, int(stream), C.byref(info)))
        return info

    # ---- FM de-emphasis
    def _rds_block_rows(self, counts: np.ndarray, rows: np.ndarray) -> list:
        return [rows[s, : min(int(counts[s]), rows.shape[1])].copy() for s in range(self.n_streams)]

    def rds_blocks(self, bits: np.ndarray, **cfg) -> list:
        """fmrx_rds_blocks: n_streams rows of bits (rds_bits' "bits"; any length) -> a list of RDS_BLOCK record
        arrays, the blocks a stream's positions judged by this call carry, in bit order.  J, V, B: the
        constants (the defaults when none is given)."""
        d = np.ascontiguousarray(bits, np.uint8).reshape(self.n_streams, -1)
        n = d.shape[1]
        rows = np.zeros((self.n_streams, max(n, 1)), RDS_BLOCK)
        counts = np.zeros(self.n_streams, np.uint32)
        c = C.byref(rds_sync_config(**cfg)) if cfg else None
        _check(lib().fmrx_rds_blocks(self.h, c, _np_ptr(d), n, _np_ptr(rows), rows.shape[1], _np_ptr(counts)))
        return self._rds_block_rows(counts, rows)

    def rds_blocks_device(self, d_bits: int, n_bits: int, d_blocks: int, max_blocks: int, d_counts: int, **cfg) -> None:
        c = C.byref(rds_sync_config(**cfg)) if cfg else None
        _check(lib().fmrx_rds_blocks_device(self.h, c, d_bits, n_bits, d_blocks, max_blocks, d_counts))

    def rds_blocks_flush(self) -> list:
        """fmrx_rds_blocks_flush: the blocks of the positions still pending, as rds_blocks returns them."""
        rows = np.zeros((self.n_streams, 26 * 8), RDS_BLOCK)
        counts = np.zeros(self.n_streams, np.uint32)
        _check(lib().fmrx_rds_blocks_flush(self.h, _np_ptr(rows), rows.shape[1], _np_ptr(counts)))
        return self._rds_block_rows(counts, rows)

    def set_rds_sync(self, on: bool) -> None:
        """fmrx_set_rds_sync: with set_rds on, the RDS decode also runs the block sync into rds_ext."""
        _check(lib().fmrx_set_rds_sync(self.h, int(bool(on))))

    def rds_ext(self, stream: int = 0) -> RdsExt:
        ext = RdsExt()
        _check(lib().fmrx_rds_ext_get(self.h, int(stream), C.byref(ext)))
        return ext

    @property
    def audio_fs(self) -> int:
        """The PCM's rate: if_fs audio_up / audio_down (geo.if_fs already holds audio_up)."""
        return self.geo.if_fs // self.geo.audio_down

    def set_deemphasis(self, tau_us: int) -> None:
        """fmrx_set_deemphasis: 0 off (the default), 50 or 75 us; every call that writes PCM then
        de-emphasises it.  Clears the stage's carry and nothing else."""
        _check(lib().fmrx_set_deemphasis(self.h, int(tau_us)))

    def deemphasis(self) -> int:
        t = C.c_int()
        _check(lib().fmrx_deemphasis(self.h, C.byref(t)))
        return t.value

    def deemph(self, d_in: int, n: int, tau_us: int, d_state: int, d_out: int | None = None,
               d_pcm: int | None = None) -> None:
        """fmrx_deemph: the de-emphasis kernel on one row of n device floats; d_state 63 floats in/out."""
        _check(lib().fmrx_deemph(self.h, d_in, n, int(tau_us), d_state, d_out, d_pcm))

    # ---- subcarrier meter
    def meter(self, demod: np.ndarray) -> np.ndarray:
        """fmrx_meter: demod rows (whole frames: multiples of rds_granule blocks) -> the tone powers,
        float32 of shape (n_streams, frames, 7), or (frames, 7) for one stream."""
        d = np.ascontiguousarray(demod, np.float32).reshape(self.n_streams, -1)
        nb = d.shape[1] // self.geo.if_samples
        if nb * self.geo.if_samples != d.shape[1]:
            raise FmrxError(FMRX_EINVAL, "meter takes whole blocks")
        frames = d.shape[1] // (METER_WINDOWS * (self.geo.bp_fs // 1000))
        out = np.zeros((self.n_streams, frames, METER_TONES), np.float32)
        _check(lib().fmrx_meter(self.h, _np_ptr(d), nb, _np_ptr(out)))
        return out if self.n_streams > 1 else out[0]

    def meter_device(self, d_demod: int, n_blocks: int, d_power: int) -> None:
        _check(lib().fmrx_meter_device(self.h, d_demod, n_blocks, d_power))

    def set_meter(self, on: bool) -> None:
        """fmrx_set_meter: the tuned, shared and wide process calls also meter their demod rows (whole frames)."""
        _check(lib().fmrx_set_meter(self.h, int(bool(on))))

    def meter_report(self, stream: int = 0) -> MeterReport:
        rep = MeterReport()
        _check(lib().fmrx_meter_get(self.h, int(stream), C.byref(rep)))
        return rep

    # ---- AFC
    def carrier(self, demod: np.ndarray) -> np.ndarray:
        """fmrx_carrier: demod rows (whole frames: multiples of rds_granule blocks) -> the carrier sums (S, Q),
        float32 of shape (n_streams, frames, 2), or (frames, 2) for one stream."""
        d = np.ascontiguousarray(demod, np.float32).reshape(self.n_streams, -1)
        nb = d.shape[1] // self.geo.if_samples
        if nb * self.geo.if_samples != d.shape[1]:
            raise FmrxError(FMRX_EINVAL, "carrier takes whole blocks")
        frames = d.shape[1] // (METER_WINDOWS * (self.geo.bp_fs // 1000))
        out = np.zeros((self.n_streams, frames, 2), np.float32)
        _check(lib().fmrx_carrier(self.h, _np_ptr(d), nb, _np_ptr(out)))
        return out if self.n_streams > 1 else out[0]

    def carrier_device(self, d_demod: int, n_blocks: int, d_sums: int) -> None:
        _check(lib().fmrx_carrier_device(self.h, d_demod, n_blocks, d_sums))

    def set_afc(self, on: bool, **kw) -> None:
        """fmrx_set_afc: the tuned, shared and wide process calls also sum their demod rows (whole frames) and,
        with track (the default), retune every stream to its carrier between calls; the settings given
        (afc_config_default's fields) replace the defaults."""
        _check(lib().fmrx_set_afc(self.h, C.byref(afc_config_default(**kw)), int(bool(on))))

    def afc_status(self, stream: int = 0) -> AfcStatus:
        st = AfcStatus()
        _check(lib().fmrx_afc_get(self.h, int(stream), C.byref(st)))
        return st

    # ---- soft stereo
    def set_stereo_blend(self, on: bool, lo_db: float | None = None, hi_db: float | None = None) -> None:
        """fmrx_set_stereo_blend: blend every stream toward mono by its pilot's signal-to-noise ratio in the
        tuned, shared and wide calls (STEREO contexts); a bound left None keeps its default (10 / 22 dB)."""
        _check(lib().fmrx_set_stereo_blend(self.h, int(bool(on)), C.byref(blend_config(lo_db, hi_db))))

    def blend_hold(self, on: bool) -> None:
        """fmrx_blend_hold: blended calls of any block count at every stream's last level (a stream's end)."""
        _check(lib().fmrx_blend_hold(self.h, int(bool(on))))

    def stereo_blend(self) -> tuple[bool, float, float]:
        """(on, lo_db, hi_db) as fmrx_stereo_blend reports them."""
        on, cfg = C.c_int(), BlendConfig()
        _check(lib().fmrx_stereo_blend(self.h, C.byref(on), C.byref(cfg)))
        return bool(on.value), cfg.lo_db, cfg.hi_db

    def blend_levels(self, power: np.ndarray, carry: np.ndarray | None = None, lo_db: float | None = None,
                     hi_db: float | None = None) -> tuple[np.ndarray, np.ndarray]:
        """fmrx_blend_levels: power (n_streams, F, 7) as the meter gives it and the carry (n_streams, 8; None:
        zeros, the power-on state) -> (levels uint8 (n_streams, F + 1), entry 0 the carried-in level; the next carry)."""
        p = np.ascontiguousarray(power, np.float32)
        if p.ndim != 3 or p.shape[0] != self.n_streams or p.shape[1] < 1 or p.shape[2] != METER_TONES:
            raise FmrxError(FMRX_EINVAL, f"power of shape {p.shape}: expected ({self.n_streams}, F >= 1, {METER_TONES})")
        c = np.zeros((self.n_streams, BLEND_CARRY), np.float32) if carry is None else np.array(carry, np.float32, order="C")
        if c.shape != (self.n_streams, BLEND_CARRY):
            raise FmrxError(FMRX_EINVAL, f"carry of shape {c.shape}: expected ({self.n_streams}, {BLEND_CARRY})")
        lv = np.zeros((self.n_streams, p.shape[1] + 1), np.uint8)
        _check(lib().fmrx_blend_levels(self.h, C.byref(blend_config(lo_db, hi_db)), _np_ptr(p), p.shape[1], _np_ptr(c), _np_ptr(lv)))
        return lv, c

    def blend_levels_device(self, d_power: int, frames: int, d_carry: int, d_levels: int, lo_db: float | None = None,
                            hi_db: float | None = None) -> None:
        _check(lib().fmrx_blend_levels_device(self.h, C.byref(blend_config(lo_db, hi_db)), d_power, frames, d_carry, d_levels))

    def blend_apply(self, d_rl: int, n: int, d_levels: int, d_out: int | None = None, d_pcm: int | None = None) -> None:
        """fmrx_blend_apply_device: n (R, L) float pairs a stream (whole granules) blended by the level rows;
        d_out (may be d_rl) takes the floats, d_pcm their S16.  Async on the context stream."""
        _check(lib().fmrx_blend_apply_device(self.h, d_rl, n, d_levels, d_out, d_pcm))

    def blend_report(self, stream: int = 0) -> dict:
        """fmrx_blend_get as a dict: frames, level_frames (17 counts) and mean = sum(l n_l) / (16 frames),
        1.0 for full stereo throughout, 0.0 for mono (and with no frames yet)."""
        out = BlendReport()
        _check(lib().fmrx_blend_get(self.h, int(stream), C.byref(out)))
        counts = [int(v) for v in out.level_frames]
        frames = int(out.frames)
        mean = sum(l * n for l, n in enumerate(counts)) / (16.0 * frames) if frames else 0.0
        return {"frames": frames, "level_frames": counts, "mean": mean}

    # ---- quieting
    def set_quieting(self, on: bool, **kw) -> None:
        """fmrx_set_quieting: high-cut and soft mute of every stream by its noise level in the tuned, shared and
        wide calls (MONO and STEREO contexts); quiet_config's fields by name, one left out keeps its default."""
        _check(lib().fmrx_set_quieting(self.h, int(bool(on)), C.byref(quiet_config(**kw))))

    def quiet_hold(self, on: bool) -> None:
        """fmrx_quiet_hold: quieted calls of any block count at every stream's last levels (a stream's end)."""
        _check(lib().fmrx_quiet_hold(self.h, int(bool(on))))

    def quieting(self) -> tuple[bool, QuietConfig]:
        """(on, config) as fmrx_quieting reports them."""
        on, cfg = C.c_int(), QuietConfig()
        _check(lib().fmrx_quieting(self.h, C.byref(on), C.byref(cfg)))
        return bool(on.value), cfg

    def quiet_levels(self, power: np.ndarray, carry: np.ndarray | None = None, **kw) -> tuple[np.ndarray, np.ndarray]:
        """fmrx_quiet_levels: power (n_streams, F, 7) as the meter gives it and the carry (n_streams, 8; None:
        zeros, the power-on state) -> (levels uint8 (n_streams, F + 1, 2), the pairs (c, m), pair 0 the carried-in
        one; the next carry).  kw: quiet_config's fields."""
        p = np.ascontiguousarray(power, np.float32)
        if p.ndim != 3 or p.shape[0] != self.n_streams or p.shape[1] < 1 or p.shape[2] != METER_TONES:
            raise FmrxError(FMRX_EINVAL, f"power of shape {p.shape}: expected ({self.n_streams}, F >= 1, {METER_TONES})")
        c = np.zeros((self.n_streams, QUIET_CARRY), np.float32) if carry is None else np.array(carry, np.float32, order="C")
        if c.shape != (self.n_streams, QUIET_CARRY):
            raise FmrxError(FMRX_EINVAL, f"carry of shape {c.shape}: expected ({self.n_streams}, {QUIET_CARRY})")
        lv = np.zeros((self.n_streams, p.shape[1] + 1, 2), np.uint8)
        _check(lib().fmrx_quiet_levels(self.h, C.byref(quiet_config(**kw)), _np_ptr(p), p.shape[1], _np_ptr(c), _np_ptr(lv)))
        return lv, c

    def quiet_levels_device(self, d_power: int, frames: int, d_carry: int, d_levels: int, **kw) -> None:
        _check(lib().fmrx_quiet_levels_device(self.h, C.byref(quiet_config(**kw)), d_power, frames, d_carry, d_levels))

    def quiet_apply(self, d_in: int, n: int, d_levels: int, d_state: int, d_out: int | None = None, d_pcm: int | None = None) -> None:
        """fmrx_quiet_apply_device: n frames a stream (whole granules; STEREO: (R, L) pairs) through the high-cut
        and the soft mute by the level rows, with the context's config; d_state (n_streams x channels x 63 floats)
        is the history, in and out; d_out (never d_in) takes the floats, d_pcm their S16.  Async on the context
        stream."""
        _check(lib().fmrx_quiet_apply_device(self.h, d_in, n, d_levels, d_state, d_out, d_pcm))

    def quiet_report(self, stream: int = 0) -> dict:
        """fmrx_quiet_get as a dict: frames, cut_frames and mute_frames (17 counts each) and cut_mean, mute_mean =
        sum(l n_l) / (16 frames), 1.0 for untouched throughout, 0.0 for closed (and with no frames yet)."""
        out = QuietReport()
        _check(lib().fmrx_quiet_get(self.h, int(stream), C.byref(out)))
        cut, mute, frames = [int(v) for v in out.cut_frames], [int(v) for v in out.mute_frames], int(out.frames)
        mean = lambda counts: sum(l * n for l, n in enumerate(counts)) / (16.0 * frames) if frames else 0.0
        return {"frames": frames, "cut_frames": cut, "mute_frames": mute, "cut_mean": mean(cut), "mute_mean": mean(mute)}

    def estimate_psd(self, samples: np.ndarray, freq_bins: int, fs: float):
        """estimatePSD (fourier.cpp:35-117) on the GPU: (freq, psd_db)."""
        x = np.ascontiguousarray(samples, np.float32)
        freq = np.zeros(freq_bins // 2, np.float32)
        psd = np.zeros(freq_bins // 2, np.float32)
        _check(lib().fmrx_estimate_psd(self.h, _np_ptr(x), x.size, freq_bins, fs, _np_ptr(freq), _np_ptr(psd)))
        return freq, psd

    def psd_device(self, d_samples: int, n: int, freq_bins: int, fs: float, d_psd: int) -> None:
        _check(lib().fmrx_psd_device(self.h, d_samples, n, freq_bins, fs, d_psd))

    def fm_demod_arctan(self, d_out: int, d_prev_phase: int, d_i: int, d_q: int, n: int) -> None:
        """fmDemodArctan (fmSupportLib.py:34-63) on device buffers (float in/out, double phase)."""
        _check(lib().fmrx_fm_demod_arctan(self.h, d_out, d_prev_phase, d_i, d_q, n))

    # ---- device entry points (pointers are device addresses)
    def process_device(self, d_iq: int, n_blocks: int, d_pcm: int, d_mono: int | None = None) -> None:
        _check(lib().fmrx_process_device_ex(self.h, d_iq, n_blocks, d_pcm, d_mono))

    # ---- off-centre tuning (several stations from one capture)
    def _tune(self, fn, offsets, first_pair: int) -> None:
        off = np.ascontiguousarray(np.atleast_1d(np.asarray(offsets, dtype=np.int64)))
        if off.size != self.n_streams:
            raise ValueError(f"{off.size} offsets for {self.n_streams} streams")
        if np.any(np.abs(off) >= 2 ** 31):
            raise FmrxError(FMRX_EINVAL, "offset does not fit 32 bits")
        off = off.astype(np.int32)
        _check(fn(self.h, _np_ptr(off), first_pair))

    def _info(self, fn) -> tuple[list[int], int, bool]:
        off = np.zeros(self.n_streams, np.int32)
        pos, on = C.c_uint64(), C.c_int()
        _check(fn(self.h, _np_ptr(off), C.byref(pos), C.byref(on)))
        return [int(v) for v in off], pos.value, bool(on.value)

    def _capture_call(self, fn, iq, per: int, blocks: int = 1) -> np.ndarray:
        """One capture's whole units of `per` elements (`blocks` blocks each) through fn: S16 PCM, n_streams rows."""
        iq = self._raw(iq).reshape(-1)
        nb = iq.size // per * blocks
        iq = np.ascontiguousarray(iq[: nb // blocks * per])
        out = np.zeros((self.n_streams, nb * self.geo.pcm_samples), np.int16)
        _check(fn(self.h, _np_ptr(iq), nb, _np_ptr(out)))
        return out if self.n_streams > 1 else out[0]

    def _scan(self, fn, iq, max_out: int, cfg: dict) -> list:
        iq = self._raw(iq).reshape(-1)
        return _station_call(fn, (self.h, _np_ptr(iq), iq.size // 2), max_out, cfg)

    def tune(self, offsets, first_pair: int = 0) -> None:
        """fmrx_tune: per-stream offsets in Hz (an int for one stream), or None for tuning off;
        first_pair is the absolute pair index of the next call's first I/Q pair."""
        if offsets is None:
            _check(lib().fmrx_tune(self.h, None, first_pair))
            return
        self._tune(lib().fmrx_tune, offsets, first_pair)

    def tuner_info(self) -> tuple[list[int], int, bool]:
        """fmrx_tuner_info: (offsets in Hz, next pair index, tuned)."""
        return self._info(lib().fmrx_tuner_info)

    def process_shared(self, iq: np.ndarray) -> np.ndarray:
        """One capture (one stream's whole blocks of raw I/Q) decoded by every tuned stream:
        S16 PCM, n_streams rows."""
        return self._capture_call(lib().fmrx_process_shared, iq, 2 * self.geo.iq_pairs)

    def process_shared_device(self, d_iq: int, n_blocks: int, d_pcm: int) -> None:
        _check(lib().fmrx_process_shared_device(self.h, d_iq, n_blocks, d_pcm))

    # ---- wide captures: a capture at decim times the mode's rate
    def set_capture_decim(self, decim: int) -> None:
        """fmrx_set_capture_decim: 1 = no wide stage, 2..10 = the capture runs at decim * rf_fs; then a reset."""
        _check(lib().fmrx_set_capture_decim(self.h, int(decim)))

    @property
    def capture_decim(self) -> int:
        d = C.c_int()
        _check(lib().fmrx_capture_decim(self.h, C.byref(d)))
        return d.value

    def set_capture_rate(self, cap_fs: int) -> None:
        """fmrx_set_capture_rate: the capture's rate in Hz, rf_fs * down / up (up = 1: set_capture_decim); then a reset."""
        _check(lib().fmrx_set_capture_rate(self.h, int(cap_fs)))

    @property
    def capture_rate(self) -> tuple[int, int, int]:
        """fmrx_capture_rate: (cap_fs, up, down)."""
        v = [C.c_int() for _ in range(3)]
        _check(lib().fmrx_capture_rate(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    @property
    def wide_granule(self) -> tuple[int, int]:
        """fmrx_wide_granule: (narrow blocks, wide pairs) of the unit a wide call is a multiple of."""
        b, w = _sz(), _sz()
        _check(lib().fmrx_wide_granule(self.h, C.byref(b), C.byref(w)))
        return b.value, w.value

    def tune_wide(self, offsets, first_pair: int = 0) -> None:
        """fmrx_tune_wide: per-stream offsets in Hz against the capture's rate (an int for one stream);
        first_pair is the absolute wide-pair index of the next call's first pair, a multiple of decim."""
        self._tune(lib().fmrx_tune_wide, offsets, first_pair)

    def wide_info(self) -> tuple[list[int], int, bool]:
        """fmrx_wide_info: (wide offsets in Hz, next wide-pair index, wide tuning on)."""
        return self._info(lib().fmrx_wide_info)

    def process_wide(self, iq: np.ndarray) -> np.ndarray:
        """One wide capture (whole granules: blocks of capture_decim * iq_pairs pairs at an integer
        ratio) decoded by every stream tuned with tune_wide: S16 PCM, n_streams rows."""
        blocks, pairs = self.wide_granule
        return self._capture_call(lib().fmrx_process_wide, iq, 2 * pairs, blocks)

    def process_wide_device(self, d_iq: int, n_blocks: int, d_pcm: int) -> None:
        _check(lib().fmrx_process_wide_device(self.h, d_iq, n_blocks, d_pcm))

    def scan_wide(self, iq: np.ndarray, max_out: int = MAX_STATIONS, **cfg) -> list:
        """fmrx_scan_wide: the stations of a wide capture, ascending by offset against its centre."""
        return self._scan(lib().fmrx_scan_wide, iq, max_out, cfg)

    # ---- band scan: which offsets of a capture hold a station
    def scan_spectrum(self, iq: np.ndarray, fft_bins: int = 4096) -> tuple[np.ndarray, int]:
        """Welch power spectrum of a raw I/Q capture (fmrx_scan_spectrum): (power, n_segments), power
        linear and FFT-shifted, bin j at (j - fft_bins / 2) * rf_fs / fft_bins Hz."""
        iq = self._raw(iq).reshape(-1)
        power = np.zeros(max(fft_bins, 0), np.float32)
        nseg = _sz()
        _check(lib().fmrx_scan_spectrum(self.h, _np_ptr(iq), iq.size // 2, fft_bins, _np_ptr(power), C.byref(nseg)))
        return power, nseg.value

    def scan_spectrum_device(self, d_iq: int, n_pairs: int, fft_bins: int, d_power: int) -> None:
        _check(lib().fmrx_scan_spectrum_device(self.h, d_iq, n_pairs, fft_bins, d_power))

    def scan(self, iq: np.ndarray, max_out: int = MAX_STATIONS, **cfg) -> list:
        """fmrx_scan: the stations of a raw I/Q capture, ascending by offset (settings: ScanConfig's
        fields)."""
        return self._scan(lib().fmrx_scan, iq, max_out, cfg)

    def synchronize(self) -> None:
        _check(lib().fmrx_synchronize(self.h))

    def stream(self) -> int:
        return lib().fmrx_stream(self.h)

    def synth_device(self, seed: int, first_pair: int, n_pairs: int, d_out: int) -> None:
        _check(lib().fmrx_synth_device(self.h, seed, self.geo.rf_fs, first_pair, n_pairs, d_out))

    def synth_device_streams(self, seeds, first_pair: int, n_pairs: int, d_out: int, stride: int) -> None:
        """One launch for several streams: stream k (seed seeds[k]) at d_out + k * stride bytes."""
        sd = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64))
        _check(lib().fmrx_synth_device_streams(self.h, sd.ctypes.data, sd.size, self.geo.rf_fs, first_pair,
                                               n_pairs, d_out, stride))

    def kernel_timing(self, reset: int = 0) -> tuple[float, int]:
        ms, n = C.c_double(), C.c_long()
        _check(lib().fmrx_kernel_timing(self.h, reset, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    # ---- state
    def get_state(self) -> bytes:
        n = C.c_size_t()
        _check(lib().fmrx_state_size(self.h, C.byref(n)))
        buf = (C.c_uint8 * n.value)()
        _check(lib().fmrx_get_state(self.h, C.addressof(buf), n.value))
        return bytes(buf)

    def set_state(self, blob: bytes) -> None:
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        _check(lib().fmrx_set_state(self.h, C.addressof(buf), len(blob)))

    def reset(self) -> None:
        _check(lib().fmrx_reset(self.h))

    # ---- time shards of one recording (mono product)
    def history_bytes(self) -> int:
        """Raw bytes before a shard that fully determine the mono product's state there."""
        n = C.c_size_t()
        _check(lib().fmrx_history_bytes(self.h, C.byref(n)))
        return n.value

    def seek(self, prev, n: int | None = None) -> None:
        """Continue, on the next call, a stream whose preceding bytes are `prev`: a host
        array (n_streams x n elements of the input format, or 1-D for one stream) or, with `n` given, a device address
        of n_streams x n bytes."""
        if n is not None:
            _check(lib().fmrx_seek(self.h, prev, n, 1))
            return
        a = np.ascontiguousarray(self._raw(prev).reshape(self.cfg.n_streams, -1))
        _check(lib().fmrx_seek(self.h, a.ctypes.data, a.shape[1] * a.itemsize, 0))

    # ---- filter.h primitives on device pointers
    def resample(self, d_out, d_state, d_in, n_in, d_coeff, taps, up, down) -> int:
        n = C.c_int()
        _check(lib().fmrx_resample(self.h, d_out, d_state, d_in, n_in, d_coeff, taps, up, down, C.byref(n)))
        return n.value

    def fm_demod(self, d_out, d_prev, d_i, d_q, n) -> None:
        _check(lib().fmrx_fm_demod(self.h, d_out, d_prev, d_i, d_q, n))

    def pll(self, d_io, n, freq, fs, nco_scale, phase_adjust, norm_bw, d_state) -> None:
        _check(lib().fmrx_pll(self.h, d_io, n, freq, fs, nco_scale, phase_adjust, norm_bw, d_state))

    def mixer(self, d_out, d_a, d_b, n) -> None:
        _check(lib().fmrx_mixer(self.h, d_out, d_a, d_b, n))

    def lr_extraction(self, d_l, d_r, d_m, d_s, n) -> None:
        _check(lib().fmrx_lr_extraction(self.h, d_l, d_r, d_m, d_s, n))

    def normalize_iq(self, d_iq, n_pairs, d_i, d_q) -> None:
        _check(lib().fmrx_normalize_iq(self.h, d_iq, n_pairs, d_i, d_q))

    def quantize(self, d_x, n, d_out) -> None:
        _check(lib().fmrx_quantize(self.h, d_x, n, d_out))

    def test_pll_fallback(self, kind: int, d_a, d_b, n: int, d_out) -> None:
        """Test hook: the PLL's fallback libm on device (0 sincos, 1 atan2, 2 NCO cos)."""
        _check(lib().fmrx_test_pll_fallback(self.h, kind, d_a, d_b, n, d_out))

    def debug_mono_stamps(self, d_stamps: int | None, n_workgroups: int = 0) -> int:
        """Diagnostic clock stamps of the fused mono kernel (fmrx.h); returns the stamp slots a
        call may need (6 u64 each)."""
        need = _sz()
        _check(lib().fmrx_debug_mono_stamps(self.h, d_stamps, n_workgroups, C.byref(need)))
        return need.value

    def stage_timing(self, op: int) -> dict | None:
        """Per-stage device time of the stereo engine (fmrx_debug_stage_timing): op 1 arms,
        0 reads, -1 reads and disarms; a read returns {stage: (ms, launches, steps)}."""
        n = len(STAGES)
        ms, steps, la = (C.c_double * n)(), (C.c_double * n)(), (C.c_long * n)()
        _check(lib().fmrx_debug_stage_timing(self.h, op, ms, steps, la, n))
        if op == 1:
            return None
        return {STAGES[k]: (ms[k], la[k], steps[k]) for k in range(n) if la[k]}

    def debug_pll_stats(self, d_counts: int | None) -> None:
        """Diagnostic speculative-PLL counters (fmrx.h): d_counts[0] += runner batches that did
        not verify, d_counts[1] += batches checked (2 u64 on the device); None turns it off."""
        _check(lib().fmrx_debug_pll_stats(self.h, d_counts))

    def debug_pll_redos(self, d_counts) -> None:
        """fmrx_debug_pll_redos: per stream and trigOffset range of the self-certifying runners
        (REDO_RANGES), redone intervals and demoted steps (n_streams x 8 u32 on the device, zeroed
        by the caller: [r] redone intervals, [4 + r] demoted steps; None turns it off).  Demoted
        steps are filed under the range of the trigOffset where the stream was demoted: where one
        demoted launch covers several runner launches (the pipelined engine, one a chunk), the later
        launches' steps land in that slot too, also past a range boundary -- [4:].sum() is exact."""
        _check(lib().fmrx_debug_pll_redos(self.h, d_counts))


def build() -> None:
    """Compile libfmrx.so and the fmrx CLI for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess

    subprocess.run(["make", "-s", "-C", PKG_DIR, "-j8"], check=True)
