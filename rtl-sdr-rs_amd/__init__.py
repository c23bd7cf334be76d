"""rtl-sdr-rs_amd -- MI355X-native FM demodulation path of ccostes/rtl-sdr-rs' simple_fm example.

Python host-side mirror of the reference interface for this path (Demod, DemodConfig,
optimal_settings; examples/simple_fm.rs:172-269) over the C ABI of include/fmd.h
(libfmd_hip.so: hand-written gfx950 HIP kernels).  No CPU implementation of the path lives
here; without the built library or a GPU every entry point raises.
"""
from ._ffi import (DEFAULT_BUF_LENGTH, DemodConfig, DemodState, DeviceConfig, FmdError, RadioConfig,
                   SynthParams, build, check, lib)
from .demod import Demod, DemodBank, PinnedBuffer, device_count, optimal_settings, out_cap
from .fir import FirBank, FirDemodBank, auto_shift
from .sink import Sink, pump
from .stations import StationBank, phase_inc, stations_auto_shift
from .channelizer import Channelizer, as_complex
from .stereo import StereoBank, stereo_taps
from .rds import RdsBank, RdsDecoder, decode_stations, rds_taps
from .receiver import ReceiverBank, receive_stations
from .narrow import NarrowBank, narrow_auto_shift, narrow_taps
from .spectrum import Spectrum, find_stations, hann_window
from .uniform import UniformChannelizer, uniform_auto_shift, uniform_channel_inc, uniform_channel_offsets, uniform_taps
from .bandplan import BandPlanBank, bandplan_auto_shifts
from .resample import Resampler, bank_rate, fixed_rate, resample_ratio, resample_taps
from .agc import Agc, leveled
from .tonesq import CTCSS_TONES, ToneSquelch, tone_squelched, tone_table
from .dcs import DCS_CODES, CodeSquelch, code_squelched, dcs_codeword, dcs_design, dcs_word
from .afsk import (AfskDemod, Ax25Decoder, Ax25Framer, afsk_stride, afsk_table, ax25_max_frames, ax25_text, decode_rows, decode_rows_gpu,
                   framed, packets)
from .pocsag import (FskDemod, Pager, PocsagDecoder, decode_pages, decode_pages_gpu, fsk_design, paged, pages, pocsag_alpha,
                     pocsag_encode, pocsag_max_messages, pocsag_numeric, pocsag_text)
from .modes import (ModeSBank, cpr_global, modes_dedupe, modes_df11, modes_encode, modes_fields, modes_frame, modes_syndrome,
                    modes_table, modes_tile)
from .pulses import PulseBank, PulseSlicer, ook_encode, package_bits, pulse_thresholds, pulses_tile
from .packages import PackageBank, packages_max, sliced
from . import shard, synth

__all__ = ["DEFAULT_BUF_LENGTH", "Demod", "DemodBank", "PinnedBuffer", "FirBank", "Sink", "pump", "FirDemodBank", "auto_shift", "StationBank", "phase_inc", "stations_auto_shift", "Channelizer", "as_complex", "StereoBank", "stereo_taps", "RdsBank", "RdsDecoder", "decode_stations", "rds_taps", "ReceiverBank", "receive_stations", "NarrowBank", "narrow_taps", "narrow_auto_shift", "Spectrum", "find_stations", "hann_window", "UniformChannelizer", "uniform_auto_shift", "uniform_channel_inc", "uniform_channel_offsets", "uniform_taps", "BandPlanBank", "bandplan_auto_shifts", "Resampler", "bank_rate", "fixed_rate", "resample_ratio", "resample_taps", "Agc", "leveled", "CTCSS_TONES", "ToneSquelch", "tone_squelched", "tone_table", "DCS_CODES", "CodeSquelch", "code_squelched", "dcs_codeword", "dcs_design", "dcs_word", "AfskDemod", "Ax25Decoder", "afsk_stride", "afsk_table", "ax25_text", "decode_rows", "packets", "Ax25Framer", "ax25_max_frames", "decode_rows_gpu", "framed", "FskDemod", "PocsagDecoder", "decode_pages", "fsk_design", "pages", "pocsag_alpha", "pocsag_encode", "pocsag_numeric", "pocsag_text", "Pager", "decode_pages_gpu", "paged", "pocsag_max_messages", "ModeSBank", "cpr_global", "modes_dedupe", "modes_df11", "modes_encode", "modes_fields", "modes_frame", "modes_syndrome", "modes_table", "modes_tile", "PulseBank", "PulseSlicer", "ook_encode", "package_bits", "pulse_thresholds", "pulses_tile", "PackageBank", "packages_max", "sliced", "DemodConfig", "DemodState", "DeviceConfig", "FmdError",
           "RadioConfig", "SynthParams", "build", "check", "lib", "device_count", "optimal_settings", "out_cap",
           "shard", "synth"]
