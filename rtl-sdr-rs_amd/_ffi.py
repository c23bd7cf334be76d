"""ctypes binding of libfmd_hip.so -- exactly the declarations of include/fmd.h."""
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
SO_PATH = os.environ.get("FMD_LIB") or os.path.join(PKG_DIR, "libfmd_hip.so")   # FMD_LIB: tuning builds only
CSRC = os.path.join(PKG_DIR, "csrc")

FMD_OK = 0
FMD_ERR_INVALID_ARG = -1
FMD_ERR_BAD_LENGTH = -2
FMD_ERR_TOO_SHORT = -3
FMD_ERR_BAD_RATES = -4
FMD_ERR_CAPACITY = -5
FMD_ERR_UNSUPPORTED = -6
FMD_ERR_BAD_STATE = -7
FMD_ERR_NO_DEVICE = -8
FMD_ERR_HIP = -9
FMD_ERR_NOMEM = -10
FMD_ERR_IO = -11

DEFAULT_BUF_LENGTH = 16 * 16384      # src/lib.rs:25


class RadioConfig(C.Structure):
    """struct RadioConfig, simple_fm.rs:173-176"""
    _fields_ = [("capture_freq", C.c_uint32), ("capture_rate", C.c_uint32)]


class DemodConfig(C.Structure):
    """struct DemodConfig, simple_fm.rs:179-185"""
    _fields_ = [("rate_in", C.c_uint32), ("rate_out", C.c_uint32), ("rate_resample", C.c_uint32),
                ("downsample", C.c_uint32), ("output_scale", C.c_uint32)]

    def __repr__(self):
        return "DemodConfig(rate_in=%d, rate_out=%d, rate_resample=%d, downsample=%d, output_scale=%d)" % (
            self.rate_in, self.rate_out, self.rate_resample, self.downsample, self.output_scale)


class DemodState(C.Structure):
    """mutable fields of struct Demod, simple_fm.rs:232-239"""
    _fields_ = [("prev_index", C.c_uint32), ("now_lpr", C.c_int32), ("prev_lpr_index", C.c_int32),
                ("lp_now_re", C.c_int32), ("lp_now_im", C.c_int32),
                ("demod_pre_re", C.c_int32), ("demod_pre_im", C.c_int32)]

    def as_dict(self):
        return {"prev_index": self.prev_index, "now_lpr": self.now_lpr, "prev_lpr_index": self.prev_lpr_index,
                "lp_now": [self.lp_now_re, self.lp_now_im], "demod_pre": [self.demod_pre_re, self.demod_pre_im]}


class DeviceConfig(C.Structure):
    _fields_ = [("n_channels", C.c_uint32), ("device_id", C.c_int32), ("flags", C.c_uint32)]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("amplitude", C.c_uint32), ("noise", C.c_uint32),
                ("dev_q32", C.c_uint32), ("mod_period", C.c_uint32)]


# name -> (restype, argtypes); must list every function include/fmd.h declares
_vp, _sz = C.c_void_p, C.c_size_t
_u8p, _i16p, _szp = C.POINTER(C.c_uint8), C.POINTER(C.c_int16), C.POINTER(C.c_size_t)
PROTOTYPES = {
    "fmd_optimal_settings": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RadioConfig), C.POINTER(DemodConfig)]),
    "fmd_demod_new": (C.c_int, [C.POINTER(DemodConfig), C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_demod_free": (None, [_vp]),
    "fmd_demod_reset": (C.c_int, [_vp]),
    "fmd_demod_demodulate": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_demod_demodulate_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_demod_demodulate_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _vp]),
    "fmd_demod_set_block_len": (C.c_int, [_vp, _sz]),
    "fmd_demod_check": (C.c_int, [_vp]),
    "fmd_demod_check_prev": (C.c_int, [_vp]),
    "fmd_demod_check_behind": (C.c_int, [_vp, C.c_uint32]),
    "fmd_demod_set_event_ordering": (C.c_int, [_vp, C.c_int]),
    "fmd_demod_f64_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_demod_last_out_len": (C.c_int, [_vp, _szp]),
    "fmd_host_alloc": (C.c_int, [_sz, C.POINTER(_vp)]),
    "fmd_host_free": (C.c_int, [_vp]),
    "fmd_out_cap": (_sz, [C.POINTER(DemodConfig), _sz]),
    "fmd_demod_get_state": (C.c_int, [_vp, C.c_uint32, C.POINTER(DemodState)]),
    "fmd_demod_set_state": (C.c_int, [_vp, C.c_uint32, C.POINTER(DemodState)]),
    "fmd_synth_fill_device": (C.c_int, [C.c_int, _vp, C.c_uint32, _sz, C.c_uint64, C.POINTER(SynthParams), _vp]),
    "fmd_strerror": (C.c_char_p, [C.c_int]),
    "fmd_last_error": (C.c_char_p, []),
    "fmd_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "fmd_version": (C.c_int, []),
    "fmd_demod_tiling": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fmd_demod_tiling_plan": (C.c_int, [_vp]),
    "fmd_demod_last_kernel": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_demod_set_tiling": (C.c_int, [_vp, C.c_uint32]),
    "fmd_fir_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_fir_free": (None, [_vp]),
    "fmd_fir_reset": (C.c_int, [_vp]),
    "fmd_fir_tap_digits": (C.c_int, [_vp]),
    "fmd_fir_out_cap": (_sz, [C.c_uint32, C.c_uint32, _sz]),
    "fmd_fir_filter_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_fir_filter_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_firdemod_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_firdemod_free": (None, [_vp]),
    "fmd_firdemod_reset": (C.c_int, [_vp]),
    "fmd_firdemod_out_cap": (_sz, [C.c_uint32, C.c_uint32, C.c_uint32, _sz]),
    "fmd_firdemod_demodulate_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_firdemod_demodulate_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_firdemod_check": (C.c_int, [_vp]),
    "fmd_firdemod_get_state": (C.c_int, [_vp, C.c_uint32, C.POINTER(DemodState)]),
    "fmd_firdemod_checkpoint_size": (C.c_size_t, [_vp]),
    "fmd_firdemod_checkpoint": (C.c_int, [_vp, _vp, _sz]),
    "fmd_firdemod_resume": (C.c_int, [_vp, _vp, _sz]),
    "fmd_firdemod_f64_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_firdemod_tiling": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fmd_firdemod_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_fir_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_stations_phase_inc": (C.c_int, [C.c_int32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fmd_stations_nco_table": (C.c_int, [_i16p]),
    "fmd_stations_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_stations_free": (None, [_vp]),
    "fmd_stations_reset": (C.c_int, [_vp]),
    "fmd_stations_out_cap": (_sz, [C.c_uint32, C.c_uint32, C.c_uint32, _sz]),
    "fmd_stations_demodulate_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_stations_demodulate_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_stations_check": (C.c_int, [_vp]),
    "fmd_stations_get_state": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(DemodState)]),
    "fmd_stations_f64_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_stations_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_channelizer_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                      C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_channelizer_free": (None, [_vp]),
    "fmd_channelizer_reset": (C.c_int, [_vp]),
    "fmd_channelizer_out_cap": (_sz, [C.c_uint32, _sz]),
    "fmd_channelizer_run_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_channelizer_run_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_channelizer_check": (C.c_int, [_vp]),
    "fmd_channelizer_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "fmd_channelizer_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_stereo_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, _i16p, C.c_uint32,
                                 _vp, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_stereo_free": (None, [_vp]),
    "fmd_stereo_reset": (C.c_int, [_vp]),
    "fmd_stereo_out_cap": (_sz, [C.c_uint32, C.c_uint32, _sz]),
    "fmd_stereo_run_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_stereo_run_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_stereo_check": (C.c_int, [_vp]),
    "fmd_stereo_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "fmd_stereo_pilot": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "fmd_stereo_pilot_inc": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fmd_stereo_kernel_name": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_size_t]),
    "fmd_rds_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, _i16p, C.c_uint32,
                              _vp, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_rds_free": (None, [_vp]),
    "fmd_rds_reset": (C.c_int, [_vp]),
    "fmd_rds_out_cap": (_sz, [C.c_uint32, C.c_uint32, _sz]),
    "fmd_rds_run_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_rds_run_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_rds_check": (C.c_int, [_vp]),
    "fmd_rds_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "fmd_rds_pilot": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "fmd_rds_kernel_name": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_size_t]),
    "fmd_rds_decoder_new": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "fmd_rds_decoder_free": (None, [_vp]),
    "fmd_rds_decoder_reset": (C.c_int, [_vp]),
    "fmd_rds_decoder_push": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_rds_decoder_info": (C.c_int, [_vp, _vp]),
    "fmd_receiver_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, _i16p, C.c_uint32, _i16p,
                                   C.c_uint32, _vp, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_receiver_free": (None, [_vp]),
    "fmd_receiver_reset": (C.c_int, [_vp]),
    "fmd_receiver_run_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp, _sz, _szp]),
    "fmd_receiver_run_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp, _sz, _szp, _vp]),
    "fmd_receiver_check": (C.c_int, [_vp]),
    "fmd_receiver_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_receiver_pilot": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "fmd_receiver_kernel_name": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_size_t]),
    "fmd_narrow_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, _i16p, _i16p, C.c_uint32,
                                 _vp, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_narrow_free": (None, [_vp]),
    "fmd_narrow_reset": (C.c_int, [_vp]),
    "fmd_narrow_out_cap": (_sz, [C.c_uint32, C.c_uint32, _sz]),
    "fmd_narrow_out_width": (C.c_uint32, [C.c_uint32]),
    "fmd_narrow_run_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_narrow_run_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_narrow_check": (C.c_int, [_vp]),
    "fmd_narrow_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "fmd_narrow_level": (C.c_int, [_vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]),
    "fmd_narrow_kernel_name": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_size_t]),
    "fmd_spectrum_hann":(C.c_int, [C.c_uint32, C.c_uint32, _i16p]),
    "fmd_spectrum_bin_inc": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fmd_spectrum_frames": (_sz, [C.c_uint32, C.c_uint32, _sz]),
    "fmd_spectrum_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_spectrum_free": (None, [_vp]),
    "fmd_spectrum_power_batch": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmd_spectrum_power_device": (C.c_int, [_vp, _vp, _sz, _vp, C.c_int, _vp]),
    "fmd_spectrum_check": (C.c_int, [_vp]),
    "fmd_spectrum_tap_digits": (C.c_int, [_vp]),
    "fmd_spectrum_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_uniform_channel_inc": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "fmd_uniform_out_cap": (_sz, [C.c_uint32, _sz]),
    "fmd_uniform_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                  C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_uniform_free": (None, [_vp]),
    "fmd_uniform_reset": (C.c_int, [_vp]),
    "fmd_uniform_run_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_uniform_run_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_uniform_check": (C.c_int, [_vp]),
    "fmd_uniform_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "fmd_uniform_tap_digits": (C.c_int, [_vp]),
    "fmd_uniform_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_bandplan_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, _i16p, _i16p,
                                   C.c_uint32, _vp, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_bandplan_free": (None, [_vp]),
    "fmd_bandplan_reset": (C.c_int, [_vp]),
    "fmd_bandplan_out_cap": (_sz, [C.c_uint32, C.c_uint32, _sz]),
    "fmd_bandplan_run_batch": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_bandplan_run_device": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp, _vp]),
    "fmd_bandplan_check": (C.c_int, [_vp]),
    "fmd_bandplan_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "fmd_bandplan_levels": (C.c_int, [_vp, _u8p, C.POINTER(C.c_uint32)]),
    "fmd_bandplan_kernel_name": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_size_t]),
    "fmd_resample_ratio": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fmd_resample_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_resample_free": (None, [_vp]),
    "fmd_resample_reset": (C.c_int, [_vp]),
    "fmd_resample_out_cap": (_sz, [C.c_uint32, C.c_uint32, _sz]),
    "fmd_resample_run_batch": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp]),
    "fmd_resample_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp, _vp]),
    "fmd_resample_check": (C.c_int, [_vp]),
    "fmd_resample_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_resample_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_agc_new": (C.c_int, [_vp, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_agc_free": (None, [_vp]),
    "fmd_agc_reset": (C.c_int, [_vp]),
    "fmd_agc_out_cap": (_sz, [C.c_uint32, _sz]),
    "fmd_agc_run_batch": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp]),
    "fmd_agc_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp, _vp]),
    "fmd_agc_check": (C.c_int, [_vp]),
    "fmd_agc_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_agc_gain": (C.c_int, [_vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fmd_agc_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_tonesq_new": (C.c_int, [_vp, _i16p, C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_tonesq_free": (None, [_vp]),
    "fmd_tonesq_reset": (C.c_int, [_vp]),
    "fmd_tonesq_out_cap": (_sz, [_sz]),
    "fmd_tonesq_run_batch": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp]),
    "fmd_tonesq_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp, _vp]),
    "fmd_tonesq_check": (C.c_int, [_vp]),
    "fmd_tonesq_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_tonesq_status": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), _u8p]),
    "fmd_tonesq_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_dcs_new": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_dcs_free": (None, [_vp]),
    "fmd_dcs_reset": (C.c_int, [_vp]),
    "fmd_dcs_out_cap": (_sz, [_sz]),
    "fmd_dcs_run_batch": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp]),
    "fmd_dcs_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp, _vp]),
    "fmd_dcs_check": (C.c_int, [_vp]),
    "fmd_dcs_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_dcs_status": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), _u8p]),
    "fmd_dcs_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_afsk_new": (C.c_int, [_i16p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_afsk_free": (None, [_vp]),
    "fmd_afsk_reset": (C.c_int, [_vp]),
    "fmd_afsk_out_cap": (_sz, [C.c_uint32, _sz]),
    "fmd_afsk_run_batch": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp]),
    "fmd_afsk_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp, _vp]),
    "fmd_afsk_check": (C.c_int, [_vp]),
    "fmd_afsk_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_afsk_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_ax25_decoder_new": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "fmd_ax25_decoder_free": (None, [_vp]),
    "fmd_ax25_decoder_reset": (C.c_int, [_vp]),
    "fmd_ax25_decoder_push": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _szp]),
    "fmd_ax25_decoder_info": (C.c_int, [_vp, _vp]),
    "fmd_hdlc_new": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_hdlc_free": (None, [_vp]),
    "fmd_hdlc_reset": (C.c_int, [_vp]),
    "fmd_hdlc_run_batch": (C.c_int, [_vp, _vp, _sz, _sz]),
    "fmd_hdlc_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp]),
    "fmd_hdlc_check": (C.c_int, [_vp]),
    "fmd_hdlc_inputs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "fmd_hdlc_counts": (C.c_int, [_vp, _vp]),
    "fmd_hdlc_frames": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmd_hdlc_info": (C.c_int, [_vp, _vp]),
    "fmd_hdlc_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_fsk_new": (C.c_int, [_vp, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_fsk_free": (None, [_vp]),
    "fmd_fsk_reset": (C.c_int, [_vp]),
    "fmd_fsk_out_cap": (_sz, [C.c_uint32, _sz]),
    "fmd_fsk_run_batch": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp]),
    "fmd_fsk_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _szp, _vp]),
    "fmd_fsk_check": (C.c_int, [_vp]),
    "fmd_fsk_outputs": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_fsk_hits": (C.c_int, [_vp, _vp, _vp]),
    "fmd_pager_fsk_hits": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "fmd_fsk_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_pocsag_decoder_new": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(_vp)]),
    "fmd_pocsag_decoder_free": (None, [_vp]),
    "fmd_pocsag_decoder_reset": (C.c_int, [_vp]),
    "fmd_pocsag_decoder_push": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _szp]),
    "fmd_pocsag_decoder_info": (C.c_int, [_vp, _vp]),
    "fmd_pocsag_correct": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fmd_pager_new": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_pager_free": (None, [_vp]),
    "fmd_pager_reset": (C.c_int, [_vp]),
    "fmd_pager_run_batch": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp, C.c_uint32]),
    "fmd_pager_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _vp, C.c_uint32, _vp]),
    "fmd_pager_check": (C.c_int, [_vp]),
    "fmd_pager_inputs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "fmd_pager_counts": (C.c_int, [_vp, _vp]),
    "fmd_pager_msgs": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmd_pager_info": (C.c_int, [_vp, _vp]),
    "fmd_pager_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_pager_table": (C.c_int, [C.c_uint32, _vp]),
    "fmd_pager_max_messages": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32, _sz]),
    "fmd_modes_new": (C.c_int, [_vp, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_modes_free": (None, [_vp]),
    "fmd_modes_reset": (C.c_int, [_vp]),
    "fmd_modes_run_batch": (C.c_int, [_vp, _vp, _sz, _sz]),
    "fmd_modes_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp]),
    "fmd_modes_check": (C.c_int, [_vp]),
    "fmd_modes_counts": (C.c_int, [_vp, _vp]),
    "fmd_modes_msgs": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmd_modes_info": (C.c_int, [_vp, _vp]),
    "fmd_modes_kernel_name": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_size_t]),
    "fmd_modes_tile": (C.c_uint32, []),
    "fmd_modes_table": (C.c_int, [C.c_uint32, _vp]),
    "fmd_modes_syndrome": (C.c_int, [_vp, _sz, C.POINTER(C.c_uint32)]),
    "fmd_modes_decode": (C.c_int, [_vp, _sz, _vp]),
    "fmd_modes_cpr_global": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "fmd_pulses_new": (C.c_int, [_vp, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_pulses_free": (None, [_vp]),
    "fmd_pulses_reset": (C.c_int, [_vp]),
    "fmd_pulses_run_batch": (C.c_int, [_vp, _vp, _sz, _sz]),
    "fmd_pulses_run_device": (C.c_int, [_vp, _vp, _sz, _sz, _vp]),
    "fmd_pulses_check": (C.c_int, [_vp]),
    "fmd_pulses_counts": (C.c_int, [_vp, _vp]),
    "fmd_pulses_recs": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmd_pulses_info": (C.c_int, [_vp, _vp]),
    "fmd_pulses_kernel_name": (C.c_int, [_vp, C.c_uint32, C.c_char_p, C.c_size_t]),
    "fmd_pulses_tile": (C.c_uint32, []),
    "fmd_pulse_slicer_new": (C.c_int, [_vp, C.POINTER(_vp)]),
    "fmd_pulse_slicer_free": (None, [_vp]),
    "fmd_pulse_slicer_push": (C.c_int, [_vp, _vp, _sz, C.c_uint64]),
    "fmd_pulse_slicer_idle": (C.c_int, [_vp, C.c_uint32, C.c_uint64]),
    "fmd_pulse_slicer_take": (C.c_int, [_vp, _vp, _sz, C.POINTER(C.c_size_t)]),
    "fmd_packages_new": (C.c_int, [_vp, C.POINTER(DeviceConfig), C.POINTER(_vp)]),
    "fmd_packages_free": (None, [_vp]),
    "fmd_packages_reset": (C.c_int, [_vp]),
    "fmd_packages_run_batch": (C.c_int, [_vp, _vp, _vp, _sz, _vp, _sz]),
    "fmd_packages_run_bank": (C.c_int, [_vp, _vp, _vp]),
    "fmd_packages_flush": (C.c_int, [_vp, _vp]),
    "fmd_packages_check": (C.c_int, [_vp]),
    "fmd_packages_counts": (C.c_int, [_vp, _vp]),
    "fmd_packages_pkgs": (C.c_int, [_vp, _vp, _sz, _vp]),
    "fmd_packages_info": (C.c_int, [_vp, _vp]),
    "fmd_packages_kernel_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "fmd_packages_max": (_sz, [_sz]),
    "fmd_sink_new": (C.c_int, [C.POINTER(DemodConfig), C.c_uint32, C.POINTER(C.c_int32), C.c_uint32, _sz, C.c_uint32, _vp, _vp, C.POINTER(_vp)]),
    "fmd_sink_free": (None, [_vp]),
    "fmd_sink_acquire": (C.c_int, [_vp, C.POINTER(_vp)]),
    "fmd_sink_submit": (C.c_int, [_vp]),
    "fmd_sink_release": (C.c_int, [_vp]),
    "fmd_sink_poll": (C.c_int, [_vp]),
    "fmd_sink_drain": (C.c_int, [_vp]),
    "fmd_sink_info": (C.c_int, [_vp, _szp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fmd_sink_f64_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "fmd_rtltcp_open": (C.c_int, [C.c_char_p, C.c_uint16, C.c_uint32, C.POINTER(_vp)]),
    "fmd_rtltcp_close": (None, [_vp]),
    "fmd_rtltcp_info": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "fmd_rtltcp_read_sync": (C.c_int, [_vp, _vp, _sz, _szp]),
    "fmd_rtltcp_command": (C.c_int, [_vp, C.c_uint8, C.c_uint32]),
    "fmd_rtltcp_read_many": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t, _szp]),
    "fmd_sink_fill_from_rtltcp": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint32)]),
    "fmd_sink_pump_rtltcp": (C.c_int, [_vp, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]),
}

SINK_CALLBACK = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.POINTER(C.c_int16), C.POINTER(C.c_size_t), C.c_size_t, C.c_int)


def build(force=False):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".cpp", ".h", ".hpp"))]
    srcs.append(os.path.join(ROOT, "include", "fmd.h"))
    fresh = os.path.exists(SO_PATH) and all(os.path.getmtime(SO_PATH) >= os.path.getmtime(s) for s in srcs)
    if force or not fresh:
        subprocess.check_call(["make", "-s", "-C", CSRC, "all"])
    return SO_PATH


_lib = None


def lib():
    """Load libfmd_hip.so.  Fails loudly if it is missing: there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). There is no CPU fallback." % SO_PATH)
        # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same soname as
        # /opt/rocm's).  Whichever loads first serves both, and device pointers / streams are
        # only shareable with torch when it is torch's -- so let torch load it first if present.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        l = C.CDLL(SO_PATH)
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(l, name)
            except AttributeError:
                if os.environ.get("FMD_LIB"):             # an older build loaded for an A/B (tools/ab.py): newer entry points absent
                    continue
                raise
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


class FmdError(RuntimeError):
    def __init__(self, status):
        l = lib()
        self.status = status
        super().__init__("%s (%d): %s" % (l.fmd_strerror(status).decode(), status, l.fmd_last_error().decode()))


def check(status):
    if status != FMD_OK:
        raise FmdError(status)


class Handle:
    """A library handle `self._h` whose entry points are fmd_<_prefix>_*: free and kernel_name."""
    _prefix = None

    def _fn(self, name):
        return getattr(lib(), "fmd_%s_%s" % (self._prefix, name))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._fn("free")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:                                                 # (at interpreter shutdown the module globals may be gone already)
            self.close()
        except Exception:
            pass

    def kernel_name(self):
        """The kernel this handle launches, as rocprofv3 --kernel-trace prints it."""
        buf = C.create_string_buffer(128)
        check(self._fn("kernel_name")(self._h, buf, len(buf)))
        return buf.value.decode()


class CheckedHandle(Handle):
    """A Handle with a completion point, fmd_<_prefix>_check."""

    def check(self):
        check(self._fn("check")(self._h))


class BankHandle(CheckedHandle):
    """A CheckedHandle with state carried across calls, which fmd_<_prefix>_reset clears."""

    def reset(self):
        check(self._fn("reset")(self._h))


class DownConverter(BankHandle):
    """Base of the down-converter handles that run through fmd_<_prefix>_run_*: `n_streams` streams in, and for each of them
    `_rows` rows (the attribute named so: stations or selected channels) of `width` int16 per output.  A subclass gives
    out_cap(nbytes); its kernel_name takes the pass where `_passes` is 2."""
    _rows = "n_stations"
    _passes = 1
    width = 2

    def kernel_name(self, which=0):
        """The kernel this handle launches (in pass `which` of `_passes`), as rocprofv3 --kernel-trace prints it."""
        buf = C.create_string_buffer(128)
        which = (int(which),) if self._passes == 2 else ()
        check(self._fn("kernel_name")(self._h, *which, buf, len(buf)))
        return buf.value.decode()

    def outputs(self):
        """Outputs per row produced since creation or reset: the index m of the next one."""
        n = C.c_uint64(0)
        check(self._fn("outputs")(self._h, C.byref(n)))
        return n.value

    def run_batch(self, iq):
        """iq uint8 [n_streams, nbytes] -> int16 array [n_streams, rows, n_out, width]."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim != 2 or iq.shape[0] != self.n_streams:
            raise ValueError("iq must be [n_streams, nbytes]")
        cap = max(1, self.out_cap(iq.shape[1]))
        out = np.empty((self.n_streams, getattr(self, self._rows), cap, self.width), dtype=np.int16)
        n = C.c_size_t(0)
        check(self._fn("run_batch")(self._h, iq.ctypes.data, iq.shape[1], out.ctypes.data, cap, C.byref(n)))
        return out[:, :, :n.value].copy()

    def run_device(self, d_iq, nbytes, d_out, out_cap, stream=None):
        """Enqueue on device pointers (d_out [n_streams][rows][out_cap][width] int16); returns the outputs per row.  `stream` must
        stay alive until the handle's next `run_device` call or `check` has returned (include/fmd.h)."""
        n = C.c_size_t(0)
        check(self._fn("run_device")(self._h, d_iq, nbytes, d_out, out_cap, C.byref(n), stream))
        return n.value


class RowProcessor(BankHandle):
    """Base of the handles that post-process the int16 rows a bank leaves on the device, through fmd_<_prefix>_run_*: `n_rows` rows
    of `width` 1 or 2 int16 per sample.  A subclass gives out_cap(n_in)."""

    def counts(self):
        """(inputs, outputs) per row since creation or reset."""
        i, o = C.c_uint64(0), C.c_uint64(0)
        check(self._fn("outputs")(self._h, C.byref(i), C.byref(o)))
        return i.value, o.value

    def outputs(self):
        return self.counts()[1]

    def run_batch(self, x):
        """x int16 [n_rows, n_in, width] ([n_rows, n_in] at width 1) -> int16 of the same form with n_out outputs per row (none
        when the handle takes a call that completes nothing, as the Agc does with a call that completes no block)."""
        x = np.ascontiguousarray(x, dtype=np.int16)
        flat = x.ndim == 2 and self.width == 1
        if flat:
            x = x[:, :, None]
        if x.ndim != 3 or x.shape[0] != self.n_rows or x.shape[2] != self.width:
            raise ValueError("x must be [n_rows, n_in, width]")
        cap = max(1, self.out_cap(x.shape[1]))
        out = np.empty((self.n_rows, cap, self.width), dtype=np.int16)
        n = C.c_size_t(0)
        check(self._fn("run_batch")(self._h, x.ctypes.data, x.shape[1], x.shape[1], out.ctypes.data, cap, C.byref(n)))
        out = out[:, :n.value].copy()
        return out[:, :, 0] if flat else out

    def run_device(self, d_in, n_in, in_cap, d_out, out_cap, stream=None):
        """Enqueue on device pointers (d_in [n_rows][in_cap][width], the first n_in samples of each row valid; d_out
        [n_rows][out_cap][width]); returns the outputs per row (0 when the Agc's call completes no block).  `stream` must stay
        alive until the handle's next `run_device` call or `check` has returned (include/fmd.h)."""
        n = C.c_size_t(0)
        check(self._fn("run_device")(self._h, d_in, n_in, in_cap, d_out, out_cap, C.byref(n), stream))
        return n.value


class RecordBank(BankHandle):
    """Base of the record banks (fmd_hdlc_*, fmd_pager_*): a decoder per row on the device, which takes the rows' soft decisions and
    leaves up to `cap` records per row and call.  A subclass gives `_cap` (the name its capacity goes by), `_reader` (the entry point
    that reads records), `_record` and `_info` (the ctypes structs), `_as_dict(record)`, max_records(n_in) and its run_*."""

    def _new(self, device_id, **fields):
        """The uint32 `fields` as attributes, range-checked: the arguments of fmd_<_prefix>_new in its order, `n_rows` last."""
        for name, v in fields.items():
            setattr(self, name, int(v))
        for name in fields:
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_rows, device_id, 0)
        check(self._fn("new")(*[getattr(self, name) for name in fields if name != "n_rows"], C.byref(dev), C.byref(self._h)))

    @property
    def cap(self):
        return getattr(self, self._cap)

    def inputs(self):
        """Samples taken per row since creation or reset."""
        n = C.c_uint64(0)
        check(self._fn("inputs")(self._h, C.byref(n)))
        return n.value

    def counts(self):
        """uint32 [n_rows]: the records each row completed in the last call."""
        c = np.zeros(self.n_rows, np.uint32)
        check(self._fn("counts")(self._h, c.ctypes.data))
        return c

    def records(self, rows):
        """The records [len(rows)][cap] of the listed rows, zero behind each row's own."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        buf = (self._record * (self.cap * max(1, rows.shape[0])))()
        check(self._fn(self._reader)(self._h, rows.ctypes.data, rows.shape[0], buf))
        return [[buf[s * self.cap + k] for k in range(self.cap)] for s in range(rows.shape[0])]

    def delivered(self, rows, counts=None):
        """A list per listed row of what the last call delivered for it, as dicts."""
        counts = self.counts() if counts is None else counts
        rec = self.records(rows)
        return [[self._as_dict(m) for m in rec[s][:min(int(counts[r]), self.cap)]] for s, r in enumerate(rows)]

    def info(self):
        """The rows' cumulative counters, a dict per row."""
        buf = (self._info * self.n_rows)()
        check(self._fn("info")(self._h, buf))
        return [{name: int(getattr(i, name)) for name, _ in self._info._fields_} for i in buf]

    def piece(self):
        """The largest power of two of soft decisions whose double still cannot complete more than `cap` records in a row."""
        piece = 1
        while self.max_records(2 * piece) <= self.cap:
            piece *= 2
        return piece

    def harvest(self, found):
        """Behind a call: the counts back, then the records of only the rows whose count is not zero, onto the lists found[row]."""
        counts = self.counts()
        hit = np.nonzero(counts)[0]
        if hit.size:
            for r, got in zip(hit.tolist(), self.delivered(hit, counts)):
                found[r] += got


def bank_rows(bank):
    """(rows, width) of a bank's output: n_streams x stations or selected channels, and the int16 per output."""
    return bank.n_streams * getattr(bank, getattr(bank, "_rows", "n_stations")), bank.width if hasattr(bank, "width") else 2


def stream_phase_incs(phase_incs, n_streams):
    """`phase_incs` as a contiguous uint32 [n_streams, n_stations] (a flat list of n_stations is taken for every stream)."""
    incs = np.asarray(phase_incs, dtype=np.uint32)
    if incs.ndim == 1:
        incs = np.tile(incs, (n_streams, 1))
    if incs.ndim != 2 or incs.shape[0] != n_streams:
        raise ValueError("phase_incs must be [n_streams, n_stations]")
    return np.ascontiguousarray(incs)
