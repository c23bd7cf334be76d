//! Thin `extern "C"` binding + safe wrapper over `include/fmd.h` (libfmd_hip.so).
//!
//! NOT COMPILED IN THIS REPOSITORY'S CI: the build image has no rustc/cargo.  It is the
//! binding a maintainer of ccostes/rtl-sdr-rs would add so that `examples/simple_fm.rs` can swap its CPU
//! `Demod` (examples/simple_fm.rs:232-427) for the GPU one without touching `receive()`/`process()`:
//! the buffers are exactly what `RtlSdr::read_sync` (src/lib.rs:153) fills.
#![allow(non_camel_case_types)]

use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

/// `struct DemodConfig`, examples/simple_fm.rs:179-185 (same field order as `fmd_demod_config`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct DemodConfig {
    pub rate_in: u32,
    pub rate_out: u32,
    pub rate_resample: u32,
    pub downsample: u32,
    pub output_scale: u32,
}

/// `struct RadioConfig`, examples/simple_fm.rs:173-176.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct RadioConfig {
    pub capture_freq: u32,
    pub capture_rate: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct DeviceConfig {
    pub n_channels: u32,
    pub device_id: i32,
    pub flags: u32,
}

/// Mutable fields of `struct Demod`, examples/simple_fm.rs:232-239.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct DemodState {
    pub prev_index: u32,
    pub now_lpr: i32,
    pub prev_lpr_index: i32,
    pub lp_now_re: i32,
    pub lp_now_im: i32,
    pub demod_pre_re: i32,
    pub demod_pre_im: i32,
}

/// `fmd_synth_params`: the deterministic integer-only FM source that stands in for the absent capture.bin.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SynthParams {
    pub seed: u64,
    pub amplitude: u32,
    pub noise: u32,
    pub dev_q32: u32,
    pub mod_period: u32,
}

#[repr(C)]
pub struct fmd_demod {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_fir {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_firdemod {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_stations {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_channelizer {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_stereo {
    _private: [u8; 0],
}

/// `fmd_stereo_config` of include/fmd.h (stereo station bank).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_stereo_config {
    pub capture_rate: u32,
    pub block: u32,
    pub audio_decim: u32,
    pub audio_shift: u32,
    pub pilot_min: u32,
}

#[repr(C)]
pub struct fmd_rds {
    _private: [u8; 0],
}

/// `fmd_rds_config` of include/fmd.h (RDS bank).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_rds_config {
    pub capture_rate: u32,
    pub block: u32,
    pub out_decim: u32,
    pub rds_shift: u32,
    pub pilot_min: u32,
}

#[repr(C)]
pub struct fmd_receiver {
    _private: [u8; 0],
}

/// `fmd_receiver_config` of include/fmd.h (FM receiver bank).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_receiver_config {
    pub capture_rate: u32,
    pub block: u32,
    pub pilot_min: u32,
    pub audio_decim: u32,
    pub audio_shift: u32,
    pub rds_decim: u32,
    pub rds_shift: u32,
}

#[repr(C)]
pub struct fmd_rds_decoder {
    _private: [u8; 0],
}

/// `fmd_rds_group` of include/fmd.h: one RDS group as the host decoder delivers it.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_rds_group {
    pub block: [u16; 4],
    pub ok_mask: u8,
    pub first_sample: u64,
}

/// `fmd_rds_info` of include/fmd.h: PI, PS (8 characters + NUL), RadioText (up to 64 + NUL) and the decoder's counters.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct fmd_rds_info {
    pub pi: u16,
    pub ps: [c_char; 9],
    pub rt: [c_char; 65],
    pub groups_ok: u64,
    pub blocks_bad: u64,
    pub synced: c_int,
}

#[repr(C)]
pub struct fmd_narrow {
    _private: [u8; 0],
}

/// `fmd_narrow_config` of include/fmd.h (narrow-band bank); `mode` is FMD_NARROW_IQ / _FM / _AM / _SSB.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_narrow_config {
    pub mode: u32,
    pub chan_decim: u32,
    pub chan_shift: u32,
    pub block: u32,
    pub squelch: u32,
    pub gain: u32,
}

pub const FMD_NARROW_IQ: u32 = 0;
pub const FMD_NARROW_FM: u32 = 1;
pub const FMD_NARROW_AM: u32 = 2;
pub const FMD_NARROW_SSB: u32 = 3;

#[repr(C)]
pub struct fmd_spectrum {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_uniform {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_bandplan {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_resample {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_agc {
    _private: [u8; 0],
}

/// `fmd_agc_config` of include/fmd.h (automatic gain control).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_agc_config {
    pub block: u32,
    pub target: u32,
    pub gain_max: u32,
    pub hang: u32,
    pub decay: u32,
}

#[repr(C)]
pub struct fmd_tonesq {
    _private: [u8; 0],
}

/// `fmd_tonesq_config` of include/fmd.h (tone squelch).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_tonesq_config {
    pub block: u32,
    pub guard: u32,
    pub dom_shift: u32,
    pub confirm: u32,
    pub hang: u32,
    pub ramp: u32,
    pub min_power: u64,
    pub accept: u64,
}

#[repr(C)]
pub struct fmd_dcs {
    _private: [u8; 0],
}

/// `fmd_dcs_config` of include/fmd.h (code squelch).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fmd_dcs_config {
    pub block: u32,
    pub box_: u32,
    pub n_taps: u32,
    pub lp: [i16; 64],
    pub lshift: u32,
    pub tap: [u32; 23],
    pub tol: u32,
    pub min_hits: u32,
    pub confirm: u32,
    pub hang: u32,
    pub ramp: u32,
    pub accept: [u64; 2],
}

#[repr(C)]
pub struct fmd_afsk {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_ax25_decoder {
    _private: [u8; 0],
}

/// `fmd_ax25_frame` of include/fmd.h: one AX.25 frame as the host decoder delivers it, without the FCS.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct fmd_ax25_frame {
    pub data: [u8; 512],
    pub len: u32,
    pub end_sample: u64,
}

/// `fmd_ax25_info` of include/fmd.h: the host decoder's counters.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_ax25_info {
    pub frames_ok: u64,
    pub bad_fcs: u64,
    pub aborts: u64,
    pub in_frame: c_int,
}

/// The frame bank of include/fmd.h: an `fmd_ax25_decoder` per row on the device.
#[repr(C)]
pub struct fmd_hdlc {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_fsk {
    _private: [u8; 0],
}

/// The page bank of include/fmd.h: an `fmd_pocsag_decoder` per row on the device.
#[repr(C)]
pub struct fmd_pager {
    _private: [u8; 0],
}

/// `fmd_fsk_config` of include/fmd.h (FSK front end of the pager decoder).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct fmd_fsk_config {
    pub d: u32,
    pub w: u32,
    pub shift: u32,
    pub tap: [u32; 32],
    pub sync: u32,
    pub tol: u32,
    pub min_corr: i32,
    pub hit_cap: u32,
}

/// `fmd_fsk_hit` of include/fmd.h: one place where the sync word ends.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_fsk_hit {
    pub k_rel: u32,
    pub d: u32,
    pub corr: i32,
    pub thr: i32,
}

#[repr(C)]
pub struct fmd_pocsag_decoder {
    _private: [u8; 0],
}

/// `fmd_pocsag_msg` of include/fmd.h: one POCSAG message as the host decoder delivers it.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct fmd_pocsag_msg {
    pub address: u32,
    pub function: u32,
    pub n_bits: u32,
    pub bits: [u8; 320],
    pub corrected: u32,
    pub inverted: u32,
    pub end_sample: u64,
}

/// `fmd_pocsag_info` of include/fmd.h: the host decoder's counters.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_pocsag_info {
    pub messages: u64,
    pub batches: u64,
    pub bad_codewords: u64,
    pub orphans: u64,
    pub locked: c_int,
    pub searching: c_int,
}

/// The Mode S bank of include/fmd.h: ADS-B messages decoded on the device per stream.
#[repr(C)]
pub struct fmd_modes {
    _private: [u8; 0],
}

/// `fmd_modes_config` of include/fmd.h.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_modes_config {
    pub min_power: u32,
    pub fix_errors: u32,
    pub df11: u32,
    pub msg_cap: u32,
}

/// `fmd_modes_msg` of include/fmd.h: one accepted Mode S message.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_modes_msg {
    pub k_rel: i32,
    pub power: u32,
    pub n_bytes: u8,
    pub fixed_bit: u8,
    pub df: u8,
    pub rsv: u8,
    pub bytes: [u8; 14],
    pub pad: [u8; 6],
}

/// `fmd_modes_totals` of include/fmd.h: a stream's cumulative counters.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_modes_totals {
    pub samples: u64,
    pub candidates: u64,
    pub messages: u64,
    pub fixed: u64,
}

/// `fmd_modes_fields` of include/fmd.h: what an extended squitter says.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_modes_fields {
    pub df: u32,
    pub icao: u32,
    pub type_code: u32,
    pub subtype: u32,
    pub has: u32,
    pub altitude_ft: i32,
    pub cpr_odd: u32,
    pub cpr_lat: u32,
    pub cpr_lon: u32,
    pub vrate_fpm: i32,
    pub speed_kt: f64,
    pub track_deg: f64,
    pub callsign: [c_char; 16],
}

/// The pulse bank of include/fmd.h: on-off-keyed pulse and gap records per stream.
#[repr(C)]
pub struct fmd_pulses {
    _private: [u8; 0],
}

/// `fmd_pulses_config` of include/fmd.h.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_pulses_config {
    pub w: u32,
    pub lo: u32,
    pub hi: u32,
    pub pulse_cap: u32,
}

/// `fmd_pulses_rec` of include/fmd.h: one pulse, decided at its fall.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_pulses_rec {
    pub k_rel: i32,
    pub width: u32,
    pub gap: u32,
    pub level: u32,
}

/// `fmd_pulses_totals` of include/fmd.h: a stream's cumulative counters, its state and its run.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_pulses_totals {
    pub samples: u64,
    pub pulses: u64,
    pub rises: u64,
    pub state: u32,
    pub rsv: u32,
    pub run: u64,
}

/// The host slicer behind the pulse bank.
#[repr(C)]
pub struct fmd_pulse_slicer {
    _private: [u8; 0],
}

pub const FMD_PULSE_PWM: u32 = 0;
pub const FMD_PULSE_PPM: u32 = 1;
pub const FMD_PULSE_BAD: u32 = 1;
pub const FMD_PULSE_TRUNCATED: u32 = 2;

/// `fmd_pulse_slicer_config` of include/fmd.h.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_pulse_slicer_config {
    pub modulation: u32,
    pub short_w: u32,
    pub long_w: u32,
    pub tol: u32,
    pub reset: u32,
}

/// `fmd_pulse_package` of include/fmd.h: one closed package of bits.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_pulse_package {
    pub start: u64,
    pub n_pulses: u32,
    pub n_bits: u32,
    pub bits: [u8; 32],
    pub flags: u32,
    pub rsv: u32,
}

/// The package bank: the host slicer for every stream of a pulse bank, on the device.
#[repr(C)]
pub struct fmd_packages {
    _private: [u8; 0],
}

/// `fmd_packages_config` of include/fmd.h.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_packages_config {
    pub slicer: fmd_pulse_slicer_config,
    pub min_bits: u32,
    pub pkg_cap: u32,
}

/// `fmd_packages_totals` of include/fmd.h: a stream's cumulative counters and its open package.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct fmd_packages_totals {
    pub records: u64,
    pub packages: u64,
    pub skipped: u64,
    pub bad: u64,
    pub open: u32,
    pub open_pulses: u32,
}

#[repr(C)]
pub struct fmd_sink {
    _private: [u8; 0],
}

#[repr(C)]
pub struct fmd_rtltcp {
    _private: [u8; 0],
}

/// `fmd_sink_callback`: (user, seq, audio [n_channels][out_cap], out_len [n_channels], out_cap, status).
pub type fmd_sink_callback = Option<unsafe extern "C" fn(*mut c_void, u64, *const i16, *const usize, usize, c_int)>;

extern "C" {
    pub fn fmd_optimal_settings(freq: u32, rate: u32, rate_resample: u32, radio: *mut RadioConfig, demod: *mut DemodConfig) -> c_int;
    pub fn fmd_demod_new(config: *const DemodConfig, dev: *const DeviceConfig, out: *mut *mut fmd_demod) -> c_int;
    pub fn fmd_demod_free(d: *mut fmd_demod);
    pub fn fmd_demod_reset(d: *mut fmd_demod) -> c_int;
    pub fn fmd_demod_demodulate(d: *mut fmd_demod, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_demod_demodulate_batch(d: *mut fmd_demod, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_demod_demodulate_device(d: *mut fmd_demod, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, d_out_len: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn fmd_demod_set_block_len(d: *mut fmd_demod, block_bytes: usize) -> c_int;
    pub fn fmd_demod_check(d: *mut fmd_demod) -> c_int;
    pub fn fmd_demod_check_prev(d: *mut fmd_demod) -> c_int;
    pub fn fmd_demod_check_behind(d: *mut fmd_demod, back: u32) -> c_int;
    pub fn fmd_demod_set_event_ordering(d: *mut fmd_demod, on: c_int) -> c_int;
    pub fn fmd_demod_f64_stats(d: *const fmd_demod, guarded: *mut u64, patched: *mut u64) -> c_int;
    pub fn fmd_demod_last_out_len(d: *const fmd_demod, out_len: *mut usize) -> c_int;
    pub fn fmd_host_alloc(nbytes: usize, ptr: *mut *mut c_void) -> c_int;
    pub fn fmd_host_free(ptr: *mut c_void) -> c_int;
    pub fn fmd_out_cap(config: *const DemodConfig, nbytes: usize) -> usize;
    pub fn fmd_demod_get_state(d: *mut fmd_demod, channel: u32, state: *mut DemodState) -> c_int;
    pub fn fmd_demod_set_state(d: *mut fmd_demod, channel: u32, state: *const DemodState) -> c_int;
    pub fn fmd_strerror(status: c_int) -> *const c_char;
    pub fn fmd_last_error() -> *const c_char;
    pub fn fmd_device_count(count: *mut c_int) -> c_int;
    pub fn fmd_version() -> c_int;
    pub fn fmd_demod_tiling(d: *const fmd_demod, audio_per_tile: *mut u32, lds_bytes: *mut u32, block_threads: *mut u32) -> c_int;
    pub fn fmd_demod_tiling_plan(d: *const fmd_demod) -> c_int;
    pub fn fmd_demod_last_kernel(d: *const fmd_demod, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_demod_set_tiling(d: *mut fmd_demod, audio_per_tile: u32) -> c_int;
    pub fn fmd_synth_fill_device(device_id: c_int, d_iq: *mut c_void, n_channels: u32, nbytes: usize, sample_offset: u64, p: *const SynthParams, stream: *mut c_void) -> c_int;
    pub fn fmd_fir_new(taps: *const i16, n_taps: u32, decim: u32, dev: *const DeviceConfig, out: *mut *mut fmd_fir) -> c_int;
    pub fn fmd_fir_free(f: *mut fmd_fir);
    pub fn fmd_fir_reset(f: *mut fmd_fir) -> c_int;
    pub fn fmd_fir_tap_digits(f: *const fmd_fir) -> c_int;
    pub fn fmd_fir_out_cap(n_taps: u32, decim: u32, nbytes: usize) -> usize;
    pub fn fmd_fir_filter_batch(f: *mut fmd_fir, iq: *const u8, nbytes: usize, out: *mut i32, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_fir_filter_device(f: *mut fmd_fir, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len_each: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_firdemod_new(taps: *const i16, n_taps: u32, decim: u32, shift: u32, rate_out: u32, rate_resample: u32, dev: *const DeviceConfig, out: *mut *mut fmd_firdemod) -> c_int;
    pub fn fmd_firdemod_free(f: *mut fmd_firdemod);
    pub fn fmd_firdemod_reset(f: *mut fmd_firdemod) -> c_int;
    pub fn fmd_firdemod_out_cap(decim: u32, rate_out: u32, rate_resample: u32, nbytes: usize) -> usize;
    pub fn fmd_firdemod_demodulate_batch(f: *mut fmd_firdemod, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_firdemod_demodulate_device(f: *mut fmd_firdemod, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len_each: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_firdemod_check(f: *mut fmd_firdemod) -> c_int;
    pub fn fmd_firdemod_get_state(f: *mut fmd_firdemod, channel: u32, state: *mut DemodState) -> c_int;
    pub fn fmd_firdemod_checkpoint_size(f: *const fmd_firdemod) -> usize;
    pub fn fmd_firdemod_checkpoint(f: *mut fmd_firdemod, blob: *mut c_void, cap: usize) -> c_int;
    pub fn fmd_firdemod_resume(f: *mut fmd_firdemod, blob: *const c_void, size: usize) -> c_int;
    pub fn fmd_firdemod_f64_stats(f: *const fmd_firdemod, guarded: *mut u64, patched: *mut u64) -> c_int;
    pub fn fmd_firdemod_tiling(f: *const fmd_firdemod, audio_per_tile: *mut u32, lds_bytes: *mut u32) -> c_int;
    pub fn fmd_firdemod_kernel_name(f: *const fmd_firdemod, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_fir_kernel_name(f: *const fmd_fir, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_stations_phase_inc(offset_hz: i32, capture_rate: u32, inc: *mut u32) -> c_int;
    pub fn fmd_stations_nco_table(table: *mut i16) -> c_int;
    pub fn fmd_stations_new(taps: *const i16, n_taps: u32, decim: u32, shift: u32, phase_inc: *const u32, n_stations: u32, rate_out: u32, rate_resample: u32, dev: *const DeviceConfig, out: *mut *mut fmd_stations) -> c_int;
    pub fn fmd_stations_free(b: *mut fmd_stations);
    pub fn fmd_stations_reset(b: *mut fmd_stations) -> c_int;
    pub fn fmd_stations_out_cap(decim: u32, rate_out: u32, rate_resample: u32, nbytes: usize) -> usize;
    pub fn fmd_stations_demodulate_batch(b: *mut fmd_stations, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_stations_demodulate_device(b: *mut fmd_stations, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len_each: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_stations_check(b: *mut fmd_stations) -> c_int;
    pub fn fmd_stations_get_state(b: *mut fmd_stations, stream: u32, station: u32, state: *mut DemodState) -> c_int;
    pub fn fmd_stations_f64_stats(b: *const fmd_stations, guarded: *mut u64, patched: *mut u64) -> c_int;
    pub fn fmd_stations_kernel_name(b: *const fmd_stations, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_channelizer_new(taps: *const i16, n_taps: u32, decim: u32, shift: u32, phase_inc: *const u32, n_stations: u32, dev: *const DeviceConfig, out: *mut *mut fmd_channelizer) -> c_int;
    pub fn fmd_channelizer_free(c: *mut fmd_channelizer);
    pub fn fmd_channelizer_reset(c: *mut fmd_channelizer) -> c_int;
    pub fn fmd_channelizer_out_cap(decim: u32, nbytes: usize) -> usize;
    pub fn fmd_channelizer_run_batch(c: *mut fmd_channelizer, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_channelizer_run_device(c: *mut fmd_channelizer, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_channelizer_check(c: *mut fmd_channelizer) -> c_int;
    pub fn fmd_channelizer_outputs(c: *const fmd_channelizer, outputs: *mut u64) -> c_int;
    pub fn fmd_channelizer_kernel_name(c: *const fmd_channelizer, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_stereo_new(taps: *const i16, n_taps: u32, decim: u32, shift: u32, phase_inc: *const u32, n_stations: u32, audio_taps: *const i16, n_audio_taps: u32, cfg: *const fmd_stereo_config, dev: *const DeviceConfig, out: *mut *mut fmd_stereo) -> c_int;
    pub fn fmd_stereo_free(s: *mut fmd_stereo);
    pub fn fmd_stereo_reset(s: *mut fmd_stereo) -> c_int;
    pub fn fmd_stereo_out_cap(decim: u32, audio_decim: u32, nbytes: usize) -> usize;
    pub fn fmd_stereo_run_batch(s: *mut fmd_stereo, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_stereo_run_device(s: *mut fmd_stereo, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_stereo_check(s: *mut fmd_stereo) -> c_int;
    pub fn fmd_stereo_outputs(s: *const fmd_stereo, outputs: *mut u64) -> c_int;
    pub fn fmd_stereo_pilot(s: *mut fmd_stereo, stream: u32, station: u32, present: *mut c_int, level: *mut u32) -> c_int;
    pub fn fmd_stereo_pilot_inc(capture_rate: u32, decim: u32, inc: *mut u32) -> c_int;
    pub fn fmd_stereo_kernel_name(s: *const fmd_stereo, pass: u32, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_rds_new(taps: *const i16, n_taps: u32, decim: u32, shift: u32, phase_inc: *const u32, n_stations: u32, rds_taps: *const i16, n_rds_taps: u32, cfg: *const fmd_rds_config, dev: *const DeviceConfig, out: *mut *mut fmd_rds) -> c_int;
    pub fn fmd_rds_free(s: *mut fmd_rds);
    pub fn fmd_rds_reset(s: *mut fmd_rds) -> c_int;
    pub fn fmd_rds_out_cap(decim: u32, out_decim: u32, nbytes: usize) -> usize;
    pub fn fmd_rds_run_batch(s: *mut fmd_rds, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_rds_run_device(s: *mut fmd_rds, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_rds_check(s: *mut fmd_rds) -> c_int;
    pub fn fmd_rds_outputs(s: *const fmd_rds, outputs: *mut u64) -> c_int;
    pub fn fmd_rds_pilot(s: *mut fmd_rds, stream: u32, station: u32, present: *mut c_int, level: *mut u32) -> c_int;
    pub fn fmd_rds_kernel_name(s: *const fmd_rds, pass: u32, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_receiver_new(taps: *const i16, n_taps: u32, decim: u32, shift: u32, phase_inc: *const u32, n_stations: u32, audio_taps: *const i16, n_audio_taps: u32, rds_taps: *const i16, n_rds_taps: u32, cfg: *const fmd_receiver_config, dev: *const DeviceConfig, out: *mut *mut fmd_receiver) -> c_int;
    pub fn fmd_receiver_free(s: *mut fmd_receiver);
    pub fn fmd_receiver_reset(s: *mut fmd_receiver) -> c_int;
    pub fn fmd_receiver_run_batch(s: *mut fmd_receiver, iq: *const u8, nbytes: usize, audio: *mut i16, audio_cap: usize, n_audio: *mut usize, rds: *mut i16, rds_cap: usize, n_rds: *mut usize) -> c_int;
    pub fn fmd_receiver_run_device(s: *mut fmd_receiver, d_iq: *const c_void, nbytes: usize, d_audio: *mut c_void, audio_cap: usize, n_audio: *mut usize, d_rds: *mut c_void, rds_cap: usize, n_rds: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_receiver_check(s: *mut fmd_receiver) -> c_int;
    pub fn fmd_receiver_outputs(s: *const fmd_receiver, audio: *mut u64, rds: *mut u64) -> c_int;
    pub fn fmd_receiver_pilot(s: *mut fmd_receiver, stream: u32, station: u32, present: *mut c_int, level: *mut u32) -> c_int;
    pub fn fmd_receiver_kernel_name(s: *const fmd_receiver, pass: u32, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_rds_decoder_new(rate_num: u32, rate_den: u32, out: *mut *mut fmd_rds_decoder) -> c_int;
    pub fn fmd_rds_decoder_free(d: *mut fmd_rds_decoder);
    pub fn fmd_rds_decoder_reset(d: *mut fmd_rds_decoder) -> c_int;
    pub fn fmd_rds_decoder_push(d: *mut fmd_rds_decoder, iq: *const i16, n: usize, groups: *mut fmd_rds_group, cap: usize, n_groups: *mut usize) -> c_int;
    pub fn fmd_rds_decoder_info(d: *const fmd_rds_decoder, info: *mut fmd_rds_info) -> c_int;
    pub fn fmd_narrow_new(taps: *const i16, n_taps: u32, decim: u32, shift: u32, phase_inc: *const u32, n_stations: u32, chan_taps_re: *const i16, chan_taps_im: *const i16, n_chan_taps: u32, cfg: *const fmd_narrow_config, dev: *const DeviceConfig, out: *mut *mut fmd_narrow) -> c_int;
    pub fn fmd_narrow_free(s: *mut fmd_narrow);
    pub fn fmd_narrow_reset(s: *mut fmd_narrow) -> c_int;
    pub fn fmd_narrow_out_cap(decim: u32, chan_decim: u32, nbytes: usize) -> usize;
    pub fn fmd_narrow_out_width(mode: u32) -> u32;
    pub fn fmd_narrow_run_batch(s: *mut fmd_narrow, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_narrow_run_device(s: *mut fmd_narrow, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_narrow_check(s: *mut fmd_narrow) -> c_int;
    pub fn fmd_narrow_outputs(s: *const fmd_narrow, outputs: *mut u64) -> c_int;
    pub fn fmd_narrow_level(s: *mut fmd_narrow, stream: u32, station: u32, open: *mut c_int, rms: *mut u32) -> c_int;
    pub fn fmd_narrow_kernel_name(s: *const fmd_narrow, pass: u32, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_spectrum_hann(n_bins: u32, amplitude: u32, window: *mut i16) -> c_int;
    pub fn fmd_spectrum_bin_inc(bin: u32, n_bins: u32, inc: *mut u32) -> c_int;
    pub fn fmd_spectrum_frames(n_bins: u32, hop: u32, nbytes: usize) -> usize;
    pub fn fmd_spectrum_new(window: *const i16, n_bins: u32, hop: u32, shift: u32, dev: *const DeviceConfig, out: *mut *mut fmd_spectrum) -> c_int;
    pub fn fmd_spectrum_free(s: *mut fmd_spectrum);
    pub fn fmd_spectrum_power_batch(s: *mut fmd_spectrum, iq: *const u8, nbytes: usize, power: *mut u64) -> c_int;
    pub fn fmd_spectrum_power_device(s: *mut fmd_spectrum, d_iq: *const c_void, nbytes: usize, d_power: *mut c_void, accumulate: c_int, stream: *mut c_void) -> c_int;
    pub fn fmd_spectrum_check(s: *mut fmd_spectrum) -> c_int;
    pub fn fmd_spectrum_tap_digits(s: *const fmd_spectrum) -> c_int;
    pub fn fmd_spectrum_kernel_name(s: *const fmd_spectrum, name: *mut c_char, cap: usize) -> c_int;
    // uniform channelizer: the declarations only (no safe wrapper yet)
    pub fn fmd_uniform_channel_inc(channel: u32, n_channels: u32, inc: *mut u32) -> c_int;
    pub fn fmd_uniform_out_cap(hop: u32, nbytes: usize) -> usize;
    pub fn fmd_uniform_new(taps: *const i16, n_taps: u32, n_channels: u32, hop: u32, shift: u32, channels: *const u32, n_selected: u32, dev: *const DeviceConfig, out: *mut *mut fmd_uniform) -> c_int;
    pub fn fmd_uniform_free(u: *mut fmd_uniform);
    pub fn fmd_uniform_reset(u: *mut fmd_uniform) -> c_int;
    pub fn fmd_uniform_run_batch(u: *mut fmd_uniform, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_uniform_run_device(u: *mut fmd_uniform, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_uniform_check(u: *mut fmd_uniform) -> c_int;
    pub fn fmd_uniform_outputs(u: *const fmd_uniform, outputs: *mut u64) -> c_int;
    pub fn fmd_uniform_tap_digits(u: *const fmd_uniform) -> c_int;
    pub fn fmd_uniform_kernel_name(u: *const fmd_uniform, name: *mut c_char, cap: usize) -> c_int;
    // band-plan bank: the declarations only (no safe wrapper yet)
    pub fn fmd_bandplan_new(taps: *const i16, n_taps: u32, n_channels: u32, hop: u32, shift: u32, channels: *const u32, n_selected: u32, chan_taps_re: *const i16, chan_taps_im: *const i16, n_chan_taps: u32, cfg: *const fmd_narrow_config, dev: *const DeviceConfig, out: *mut *mut fmd_bandplan) -> c_int;
    pub fn fmd_bandplan_free(b: *mut fmd_bandplan);
    pub fn fmd_bandplan_reset(b: *mut fmd_bandplan) -> c_int;
    pub fn fmd_bandplan_out_cap(hop: u32, chan_decim: u32, nbytes: usize) -> usize;
    pub fn fmd_bandplan_run_batch(b: *mut fmd_bandplan, iq: *const u8, nbytes: usize, out: *mut i16, out_cap: usize, out_len: *mut usize) -> c_int;
    pub fn fmd_bandplan_run_device(b: *mut fmd_bandplan, d_iq: *const c_void, nbytes: usize, d_out: *mut c_void, out_cap: usize, out_len: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_bandplan_check(b: *mut fmd_bandplan) -> c_int;
    pub fn fmd_bandplan_outputs(b: *const fmd_bandplan, outputs: *mut u64) -> c_int;
    pub fn fmd_bandplan_levels(b: *mut fmd_bandplan, open: *mut u8, rms: *mut u32) -> c_int;
    pub fn fmd_bandplan_kernel_name(b: *const fmd_bandplan, pass: u32, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_resample_ratio(rate_in_num: u64, rate_in_den: u64, rate_out: u64, l: *mut u32, m: *mut u32) -> c_int;
    pub fn fmd_resample_new(taps: *const i16, l: u32, m: u32, t: u32, shift: u32, width: u32, dev: *const DeviceConfig, out: *mut *mut fmd_resample) -> c_int;
    pub fn fmd_resample_free(r: *mut fmd_resample);
    pub fn fmd_resample_reset(r: *mut fmd_resample) -> c_int;
    pub fn fmd_resample_out_cap(l: u32, m: u32, n_in: usize) -> usize;
    pub fn fmd_resample_run_batch(r: *mut fmd_resample, input: *const i16, n_in: usize, in_cap: usize, out: *mut i16, out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn fmd_resample_run_device(r: *mut fmd_resample, d_in: *const c_void, n_in: usize, in_cap: usize, d_out: *mut c_void, out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_resample_check(r: *mut fmd_resample) -> c_int;
    pub fn fmd_resample_outputs(r: *const fmd_resample, inputs: *mut u64, outputs: *mut u64) -> c_int;
    pub fn fmd_resample_kernel_name(r: *const fmd_resample, name: *mut c_char, cap: usize) -> c_int;
    // automatic gain control: the declarations only (no safe wrapper yet)
    pub fn fmd_agc_new(cfg: *const fmd_agc_config, width: u32, dev: *const DeviceConfig, out: *mut *mut fmd_agc) -> c_int;
    pub fn fmd_agc_free(a: *mut fmd_agc);
    pub fn fmd_agc_reset(a: *mut fmd_agc) -> c_int;
    pub fn fmd_agc_out_cap(block: u32, n_in: usize) -> usize;
    pub fn fmd_agc_run_batch(a: *mut fmd_agc, input: *const i16, n_in: usize, in_cap: usize, out: *mut i16, out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn fmd_agc_run_device(a: *mut fmd_agc, d_in: *const c_void, n_in: usize, in_cap: usize, d_out: *mut c_void, out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_agc_check(a: *mut fmd_agc) -> c_int;
    pub fn fmd_agc_outputs(a: *const fmd_agc, inputs: *mut u64, outputs: *mut u64) -> c_int;
    pub fn fmd_agc_gain(a: *mut fmd_agc, row: u32, gain: *mut u32, hang: *mut u32) -> c_int;
    pub fn fmd_agc_kernel_name(a: *const fmd_agc, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_tonesq_new(cfg: *const fmd_tonesq_config, table: *const i16, n_tones: u32, width: u32, dev: *const DeviceConfig, out: *mut *mut fmd_tonesq) -> c_int;
    pub fn fmd_tonesq_free(t: *mut fmd_tonesq);
    pub fn fmd_tonesq_reset(t: *mut fmd_tonesq) -> c_int;
    pub fn fmd_tonesq_out_cap(n_in: usize) -> usize;
    pub fn fmd_tonesq_run_batch(t: *mut fmd_tonesq, input: *const i16, n_in: usize, in_cap: usize, out: *mut i16, out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn fmd_tonesq_run_device(t: *mut fmd_tonesq, d_in: *const c_void, n_in: usize, in_cap: usize, d_out: *mut c_void, out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_tonesq_check(t: *mut fmd_tonesq) -> c_int;
    pub fn fmd_tonesq_outputs(t: *const fmd_tonesq, inputs: *mut u64, outputs: *mut u64) -> c_int;
    pub fn fmd_tonesq_status(t: *mut fmd_tonesq, tone: *mut i32, power: *mut u64, open: *mut u8) -> c_int;
    pub fn fmd_tonesq_kernel_name(t: *const fmd_tonesq, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_dcs_new(cfg: *const fmd_dcs_config, words: *const u32, n_words: u32, width: u32, dev: *const DeviceConfig, out: *mut *mut fmd_dcs) -> c_int;
    pub fn fmd_dcs_free(d: *mut fmd_dcs);
    pub fn fmd_dcs_reset(d: *mut fmd_dcs) -> c_int;
    pub fn fmd_dcs_out_cap(n_in: usize) -> usize;
    pub fn fmd_dcs_run_batch(d: *mut fmd_dcs, input: *const i16, n_in: usize, in_cap: usize, out: *mut i16, out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn fmd_dcs_run_device(d: *mut fmd_dcs, d_in: *const c_void, n_in: usize, in_cap: usize, d_out: *mut c_void, out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_dcs_check(d: *mut fmd_dcs) -> c_int;
    pub fn fmd_dcs_outputs(d: *const fmd_dcs, inputs: *mut u64, outputs: *mut u64) -> c_int;
    pub fn fmd_dcs_status(d: *mut fmd_dcs, code: *mut i32, hits: *mut u32, open: *mut u8) -> c_int;
    pub fn fmd_dcs_kernel_name(d: *const fmd_dcs, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_afsk_new(table: *const i16, t: u32, d: u32, pre_shift: u32, out_shift: u32, width: u32, dev: *const DeviceConfig, out: *mut *mut fmd_afsk) -> c_int;
    pub fn fmd_afsk_free(a: *mut fmd_afsk);
    pub fn fmd_afsk_reset(a: *mut fmd_afsk) -> c_int;
    pub fn fmd_afsk_out_cap(d: u32, n_in: usize) -> usize;
    pub fn fmd_afsk_run_batch(a: *mut fmd_afsk, input: *const i16, n_in: usize, in_cap: usize, out: *mut i16, out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn fmd_afsk_run_device(a: *mut fmd_afsk, d_in: *const c_void, n_in: usize, in_cap: usize, d_out: *mut c_void, out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_afsk_check(a: *mut fmd_afsk) -> c_int;
    pub fn fmd_afsk_outputs(a: *const fmd_afsk, inputs: *mut u64, outputs: *mut u64) -> c_int;
    pub fn fmd_afsk_kernel_name(a: *const fmd_afsk, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_ax25_decoder_new(rate_num: u32, rate_den: u32, baud: u32, out: *mut *mut fmd_ax25_decoder) -> c_int;
    pub fn fmd_ax25_decoder_free(d: *mut fmd_ax25_decoder);
    pub fn fmd_ax25_decoder_reset(d: *mut fmd_ax25_decoder) -> c_int;
    pub fn fmd_ax25_decoder_push(d: *mut fmd_ax25_decoder, soft: *const i16, n: usize, frames: *mut fmd_ax25_frame, cap: usize, n_frames: *mut usize) -> c_int;
    pub fn fmd_ax25_decoder_info(d: *const fmd_ax25_decoder, info: *mut fmd_ax25_info) -> c_int;
    pub fn fmd_hdlc_new(rate_num: u32, rate_den: u32, baud: u32, frame_cap: u32, dev: *const DeviceConfig, out: *mut *mut fmd_hdlc) -> c_int;
    pub fn fmd_hdlc_free(f: *mut fmd_hdlc);
    pub fn fmd_hdlc_reset(f: *mut fmd_hdlc) -> c_int;
    pub fn fmd_hdlc_run_batch(f: *mut fmd_hdlc, input: *const i16, n_in: usize, in_cap: usize) -> c_int;
    pub fn fmd_hdlc_run_device(f: *mut fmd_hdlc, d_in: *const c_void, n_in: usize, in_cap: usize, stream: *mut c_void) -> c_int;
    pub fn fmd_hdlc_check(f: *mut fmd_hdlc) -> c_int;
    pub fn fmd_hdlc_inputs(f: *const fmd_hdlc, inputs: *mut u64) -> c_int;
    pub fn fmd_hdlc_counts(f: *mut fmd_hdlc, counts: *mut u32) -> c_int;
    pub fn fmd_hdlc_frames(f: *mut fmd_hdlc, rows: *const u32, n_sel: usize, frames: *mut fmd_ax25_frame) -> c_int;
    pub fn fmd_hdlc_info(f: *mut fmd_hdlc, info: *mut fmd_ax25_info) -> c_int;
    pub fn fmd_hdlc_kernel_name(f: *const fmd_hdlc, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_fsk_new(cfg: *const fmd_fsk_config, width: u32, dev: *const DeviceConfig, out: *mut *mut fmd_fsk) -> c_int;
    pub fn fmd_fsk_free(f: *mut fmd_fsk);
    pub fn fmd_fsk_reset(f: *mut fmd_fsk) -> c_int;
    pub fn fmd_fsk_out_cap(d: u32, n_in: usize) -> usize;
    pub fn fmd_fsk_run_batch(f: *mut fmd_fsk, input: *const i16, n_in: usize, in_cap: usize, out: *mut i16, out_cap: usize, n_out: *mut usize) -> c_int;
    pub fn fmd_fsk_run_device(f: *mut fmd_fsk, d_in: *const c_void, n_in: usize, in_cap: usize, d_out: *mut c_void, out_cap: usize, n_out: *mut usize, stream: *mut c_void) -> c_int;
    pub fn fmd_fsk_check(f: *mut fmd_fsk) -> c_int;
    pub fn fmd_fsk_outputs(f: *const fmd_fsk, inputs: *mut u64, outputs: *mut u64) -> c_int;
    pub fn fmd_fsk_hits(f: *mut fmd_fsk, counts: *mut u32, hits: *mut fmd_fsk_hit) -> c_int;
    pub fn fmd_pager_fsk_hits(f: *mut fmd_fsk, d_counts: *mut *const c_void, d_hits: *mut *const c_void) -> c_int;
    pub fn fmd_fsk_kernel_name(f: *const fmd_fsk, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_pocsag_decoder_new(rate_num: u32, rate_den: u32, baud: u32, max_errors: u32, out: *mut *mut fmd_pocsag_decoder) -> c_int;
    pub fn fmd_pocsag_decoder_free(d: *mut fmd_pocsag_decoder);
    pub fn fmd_pocsag_decoder_reset(d: *mut fmd_pocsag_decoder) -> c_int;
    pub fn fmd_pocsag_decoder_push(d: *mut fmd_pocsag_decoder, soft: *const i16, n: usize, hits: *const fmd_fsk_hit, n_hits: usize, msgs: *mut fmd_pocsag_msg, cap: usize, n_msgs: *mut usize) -> c_int;
    pub fn fmd_pocsag_decoder_info(d: *const fmd_pocsag_decoder, info: *mut fmd_pocsag_info) -> c_int;
    pub fn fmd_pocsag_correct(word: u32, max_errors: u32, cw: *mut u32, n_fixed: *mut u32) -> c_int;
    pub fn fmd_pager_max_messages(rate_num: u32, rate_den: u32, baud: u32, n: usize) -> usize;
    pub fn fmd_pager_new(rate_num: u32, rate_den: u32, baud: u32, max_errors: u32, msg_cap: u32, dev: *const DeviceConfig, out: *mut *mut fmd_pager) -> c_int;
    pub fn fmd_pager_free(p: *mut fmd_pager);
    pub fn fmd_pager_reset(p: *mut fmd_pager) -> c_int;
    pub fn fmd_pager_run_batch(p: *mut fmd_pager, soft: *const i16, n_in: usize, in_cap: usize, counts: *const u32, hits: *const fmd_fsk_hit, hit_cap: u32) -> c_int;
    pub fn fmd_pager_run_device(p: *mut fmd_pager, d_soft: *const c_void, n_in: usize, in_cap: usize, d_counts: *const c_void, d_hits: *const c_void, hit_cap: u32, stream: *mut c_void) -> c_int;
    pub fn fmd_pager_check(p: *mut fmd_pager) -> c_int;
    pub fn fmd_pager_inputs(p: *const fmd_pager, inputs: *mut u64) -> c_int;
    pub fn fmd_pager_counts(p: *mut fmd_pager, counts: *mut u32) -> c_int;
    pub fn fmd_pager_msgs(p: *mut fmd_pager, rows: *const u32, n_sel: usize, msgs: *mut fmd_pocsag_msg) -> c_int;
    pub fn fmd_pager_info(p: *mut fmd_pager, info: *mut fmd_pocsag_info) -> c_int;
    pub fn fmd_pager_kernel_name(p: *const fmd_pager, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_pager_table(max_errors: u32, table: *mut u32) -> c_int;
    pub fn fmd_modes_new(cfg: *const fmd_modes_config, dev: *const DeviceConfig, out: *mut *mut fmd_modes) -> c_int;
    pub fn fmd_modes_free(h: *mut fmd_modes);
    pub fn fmd_modes_reset(h: *mut fmd_modes) -> c_int;
    pub fn fmd_modes_run_batch(h: *mut fmd_modes, iq: *const u8, nbytes: usize, cap_bytes: usize) -> c_int;
    pub fn fmd_modes_run_device(h: *mut fmd_modes, d_iq: *const c_void, nbytes: usize, cap_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn fmd_modes_check(h: *mut fmd_modes) -> c_int;
    pub fn fmd_modes_counts(h: *mut fmd_modes, counts: *mut u32) -> c_int;
    pub fn fmd_modes_msgs(h: *mut fmd_modes, streams: *const u32, n_sel: usize, msgs: *mut fmd_modes_msg) -> c_int;
    pub fn fmd_modes_info(h: *mut fmd_modes, info: *mut fmd_modes_totals) -> c_int;
    pub fn fmd_modes_kernel_name(h: *const fmd_modes, pass: u32, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_modes_tile() -> u32;
    pub fn fmd_modes_table(n_bits: u32, table: *mut u32) -> c_int;
    pub fn fmd_modes_syndrome(bytes: *const u8, n_bytes: usize, syn: *mut u32) -> c_int;
    pub fn fmd_modes_decode(bytes: *const u8, n_bytes: usize, out: *mut fmd_modes_fields) -> c_int;
    pub fn fmd_modes_cpr_global(lat_even: u32, lon_even: u32, lat_odd: u32, lon_odd: u32, latest_odd: c_int, lat: *mut f64, lon: *mut f64) -> c_int;
    pub fn fmd_pulses_new(cfg: *const fmd_pulses_config, dev: *const DeviceConfig, out: *mut *mut fmd_pulses) -> c_int;
    pub fn fmd_pulses_free(h: *mut fmd_pulses);
    pub fn fmd_pulses_reset(h: *mut fmd_pulses) -> c_int;
    pub fn fmd_pulses_run_batch(h: *mut fmd_pulses, iq: *const u8, nbytes: usize, cap_bytes: usize) -> c_int;
    pub fn fmd_pulses_run_device(h: *mut fmd_pulses, d_iq: *const c_void, nbytes: usize, cap_bytes: usize, stream: *mut c_void) -> c_int;
    pub fn fmd_pulses_check(h: *mut fmd_pulses) -> c_int;
    pub fn fmd_pulses_counts(h: *mut fmd_pulses, counts: *mut u32) -> c_int;
    pub fn fmd_pulses_recs(h: *mut fmd_pulses, streams: *const u32, n_sel: usize, recs: *mut fmd_pulses_rec) -> c_int;
    pub fn fmd_pulses_info(h: *mut fmd_pulses, info: *mut fmd_pulses_totals) -> c_int;
    pub fn fmd_pulses_kernel_name(h: *const fmd_pulses, pass: u32, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_pulses_tile() -> u32;
    pub fn fmd_pulse_slicer_new(cfg: *const fmd_pulse_slicer_config, out: *mut *mut fmd_pulse_slicer) -> c_int;
    pub fn fmd_pulse_slicer_free(p: *mut fmd_pulse_slicer);
    pub fn fmd_pulse_slicer_push(p: *mut fmd_pulse_slicer, recs: *const fmd_pulses_rec, n: usize, pos: u64) -> c_int;
    pub fn fmd_pulse_slicer_idle(p: *mut fmd_pulse_slicer, state: u32, run: u64) -> c_int;
    pub fn fmd_pulse_slicer_take(p: *mut fmd_pulse_slicer, packages: *mut fmd_pulse_package, cap: usize, n: *mut usize) -> c_int;
    pub fn fmd_packages_new(cfg: *const fmd_packages_config, dev: *const DeviceConfig, out: *mut *mut fmd_packages) -> c_int;
    pub fn fmd_packages_free(h: *mut fmd_packages);
    pub fn fmd_packages_reset(h: *mut fmd_packages) -> c_int;
    pub fn fmd_packages_run_batch(h: *mut fmd_packages, counts: *const u32, recs: *const fmd_pulses_rec, rec_cap: usize, totals: *const fmd_pulses_totals, n_samples: usize) -> c_int;
    pub fn fmd_packages_run_bank(h: *mut fmd_packages, bank: *mut fmd_pulses, stream: *mut c_void) -> c_int;
    pub fn fmd_packages_flush(h: *mut fmd_packages, stream: *mut c_void) -> c_int;
    pub fn fmd_packages_check(h: *mut fmd_packages) -> c_int;
    pub fn fmd_packages_counts(h: *mut fmd_packages, counts: *mut u32) -> c_int;
    pub fn fmd_packages_pkgs(h: *mut fmd_packages, streams: *const u32, n_sel: usize, pkgs: *mut fmd_pulse_package) -> c_int;
    pub fn fmd_packages_info(h: *mut fmd_packages, info: *mut fmd_packages_totals) -> c_int;
    pub fn fmd_packages_kernel_name(h: *const fmd_packages, name: *mut c_char, cap: usize) -> c_int;
    pub fn fmd_packages_max(n_records: usize) -> usize;
    pub fn fmd_sink_new(config: *const DemodConfig, n_channels: u32, device_ids: *const i32, n_devices: u32, nbytes: usize, depth: u32, callback: fmd_sink_callback, user: *mut c_void, out: *mut *mut fmd_sink) -> c_int;
    pub fn fmd_sink_free(s: *mut fmd_sink);
    pub fn fmd_sink_acquire(s: *mut fmd_sink, iq: *mut *mut u8) -> c_int;
    pub fn fmd_sink_submit(s: *mut fmd_sink) -> c_int;
    pub fn fmd_sink_release(s: *mut fmd_sink) -> c_int;
    pub fn fmd_sink_poll(s: *mut fmd_sink) -> c_int;
    pub fn fmd_sink_drain(s: *mut fmd_sink) -> c_int;
    pub fn fmd_sink_info(s: *const fmd_sink, out_cap: *mut usize, n_devices: *mut u32, in_flight: *mut u32) -> c_int;
    pub fn fmd_sink_f64_stats(s: *const fmd_sink, guarded: *mut u64, patched: *mut u64) -> c_int;
    pub fn fmd_rtltcp_open(host: *const c_char, port: u16, timeout_ms: u32, out: *mut *mut fmd_rtltcp) -> c_int;
    pub fn fmd_rtltcp_close(s: *mut fmd_rtltcp);
    pub fn fmd_rtltcp_info(s: *const fmd_rtltcp, tuner_type: *mut u32, gain_count: *mut u32) -> c_int;
    pub fn fmd_rtltcp_read_sync(s: *mut fmd_rtltcp, buf: *mut u8, nbytes: usize, n_read: *mut usize) -> c_int;
    pub fn fmd_rtltcp_command(s: *mut fmd_rtltcp, opcode: u8, param: u32) -> c_int;
    pub fn fmd_rtltcp_read_many(sources: *const *mut fmd_rtltcp, n: u32, base: *mut u8, row_stride: usize, nbytes: usize, n_read: *mut usize) -> c_int;
    pub fn fmd_sink_fill_from_rtltcp(s: *mut fmd_sink, sources: *const *mut fmd_rtltcp, n_sources: u32, n_short: *mut u32) -> c_int;
    pub fn fmd_sink_pump_rtltcp(s: *mut fmd_sink, sources: *const *mut fmd_rtltcp, n_sources: u32, max_buffers: u64, n_submitted: *mut u64) -> c_int;
}

/// Error in the crate's convention (`src/error.rs:8,40-44`: a Result, never a panic).
#[derive(Debug)]
pub struct FmdError {
    pub status: i32,
    pub message: String,
}

impl std::fmt::Display for FmdError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "fmd error {}: {}", self.status, self.message)
    }
}
impl std::error::Error for FmdError {}

pub type Result<T> = std::result::Result<T, FmdError>;

fn check(status: c_int) -> Result<()> {
    if status == 0 {
        return Ok(());
    }
    let msg = unsafe {
        format!("{}: {}", CStr::from_ptr(fmd_strerror(status)).to_string_lossy(), CStr::from_ptr(fmd_last_error()).to_string_lossy())
    };
    Err(FmdError { status, message: msg })
}

/// `optimal_settings(freq, rate)`, examples/simple_fm.rs:189-214.
pub fn optimal_settings(freq: u32, rate: u32, rate_resample: u32) -> Result<(RadioConfig, DemodConfig)> {
    let (mut r, mut d) = (RadioConfig::default(), DemodConfig::default());
    check(unsafe { fmd_optimal_settings(freq, rate, rate_resample, &mut r, &mut d) })?;
    Ok((r, d))
}

/// Drop-in for the example's `Demod`: `Demod::new(config)` / `demod.demodulate(buf)`.
pub struct Demod {
    handle: *mut fmd_demod,
    pub config: DemodConfig,
}

// One caller at a time, like `&mut self` in the reference; the handle may move between threads.
unsafe impl Send for Demod {}

impl Demod {
    /// examples/simple_fm.rs:243-252
    pub fn new(config: DemodConfig) -> Result<Self> {
        let dev = DeviceConfig { n_channels: 1, device_id: -1, flags: 0 };
        let mut handle: *mut fmd_demod = std::ptr::null_mut();
        check(unsafe { fmd_demod_new(&config, &dev, &mut handle) })?;
        Ok(Demod { handle, config })
    }

    /// examples/simple_fm.rs:256-269.  Where the reference panics (len % 8 != 0, < 2 decimated samples) this
    /// returns Err.
    pub fn demodulate(&mut self, buf: Vec<u8>) -> Result<Vec<i16>> {
        let cap = unsafe { fmd_out_cap(&self.config, buf.len()) } + 1;
        let mut out = vec![0i16; cap];
        let mut n: usize = 0;
        check(unsafe { fmd_demod_demodulate(self.handle, buf.as_ptr(), buf.len(), out.as_mut_ptr(), cap, &mut n) })?;
        out.truncate(n);
        Ok(out)
    }

    /// STREAM LIFETIME for callers of the raw `fmd_demod_demodulate_device` / `fmd_fir_filter_device` / `fmd_firdemod_demodulate_device`
    /// bindings above: the `stream` of a handle's most recent device launch must stay alive until the handle's next device launch or
    /// completion point (`check`, `check_prev`, `state`, `set_state`, a host entry) has returned (include/fmd.h) -- the safe wrappers
    /// of this crate only use the library's own stream and are not affected.
    ///
    /// Completion / verification point after device-side launches (`fmd_demod_check`): waits, surfaces device-side
    /// assertions and settles the guarded f64 samples against the host libm.  The host entry points used by
    /// `demodulate` do this themselves; it is here for callers that drive `fmd_demod_demodulate_device` directly.
    pub fn check(&mut self) -> Result<()> {
        check(unsafe { fmd_demod_check(self.handle) })
    }

    /// The same one launch back (`fmd_demod_check_prev`): with launches 1 ..= n enqueued on the device entry point, waits for launch
    /// n - 1 only and settles its f64 samples while launch n runs -- the `demodulate` -> `output` cadence of `simple_fm.rs:150-156`
    /// without serialising host and device.  Until a launch has been settled its output buffer must stay allocated and unread, its
    /// input buffer unmodified, and the stream of the most recent launch alive (include/fmd.h).
    pub fn check_prev(&mut self) -> Result<()> {
        check(unsafe { fmd_demod_check_prev(self.handle) })
    }

    /// `fmd_demod_check_behind`: the completion point `back` launches back (0 = `check`, 1 = `check_prev`, 2 keeps a whole launch queued
    /// behind the running one and absorbs a late host).  Launches are settled in order; the last THREE launches' output buffers must
    /// stay allocated and unread, their input buffers unmodified, until they are settled.
    pub fn check_behind(&mut self, back: u32) -> Result<()> {
        check(unsafe { fmd_demod_check_behind(self.handle, back) })
    }

    pub fn state(&mut self) -> Result<DemodState> {
        let mut s = DemodState::default();
        check(unsafe { fmd_demod_get_state(self.handle, 0, &mut s) })?;
        Ok(s)
    }
}

impl Drop for Demod {
    fn drop(&mut self) {
        unsafe { fmd_demod_free(self.handle) }
    }
}

/// Many independent streams on one GPU: `n_channels` reference `Demod`s behind one handle (the case the GPU is
/// for).  `iq` is channel-major `[n_channels][nbytes]`, exactly `n_channels` `read_sync` buffers back to back.
pub struct DemodBank {
    handle: *mut fmd_demod,
    pub config: DemodConfig,
    pub n_channels: usize,
}

unsafe impl Send for DemodBank {}

impl DemodBank {
    pub fn new(config: DemodConfig, n_channels: usize, device_id: i32) -> Result<Self> {
        let dev = DeviceConfig { n_channels: n_channels as u32, device_id, flags: 0 };
        let mut handle: *mut fmd_demod = std::ptr::null_mut();
        check(unsafe { fmd_demod_new(&config, &dev, &mut handle) })?;
        Ok(DemodBank { handle, config, n_channels })
    }

    /// One `Demod::demodulate` per channel; returns one `Vec<i16>` per channel.
    pub fn demodulate(&mut self, iq: &[u8]) -> Result<Vec<Vec<i16>>> {
        assert!(iq.len() % self.n_channels == 0, "iq must hold n_channels equal-sized buffers");
        let nbytes = iq.len() / self.n_channels;
        let cap = unsafe { fmd_out_cap(&self.config, nbytes) } + 1;
        let mut out = vec![0i16; cap * self.n_channels];
        let mut lens = vec![0usize; self.n_channels];
        check(unsafe { fmd_demod_demodulate_batch(self.handle, iq.as_ptr(), nbytes, out.as_mut_ptr(), cap, lens.as_mut_ptr()) })?;
        Ok((0..self.n_channels).map(|c| out[c * cap..c * cap + lens[c]].to_vec()).collect())
    }
}

impl Drop for DemodBank {
    fn drop(&mut self) {
        unsafe { fmd_demod_free(self.handle) }
    }
}

/// Station bank (`fmd_stations_*`): `phase_incs.len() / n_streams` FM stations demodulated out of each of `n_streams` wideband
/// streams -- mix by the station's offset, filter with `taps`, decimate by `decim`, then the reference's `fm_demod` and
/// `low_pass_real` per station (include/fmd.h).
pub struct StationBank {
    handle: *mut fmd_stations,
    pub decim: u32,
    pub rate_out: u32,
    pub rate_resample: u32,
    pub n_streams: usize,
    pub n_stations: usize,
}

unsafe impl Send for StationBank {}

/// Phase increment (Q32 cycles per input sample) of a station `offset_hz` away from the capture's centre.
pub fn phase_inc(offset_hz: i32, capture_rate: u32) -> Result<u32> {
    let mut inc = 0u32;
    check(unsafe { fmd_stations_phase_inc(offset_hz, capture_rate, &mut inc) })?;
    Ok(inc)
}

impl StationBank {
    /// `phase_incs` is `[n_streams][n_stations]`.
    pub fn new(taps: &[i16], decim: u32, shift: u32, phase_incs: &[u32], n_streams: usize, rate_out: u32, rate_resample: u32,
               device_id: i32) -> Result<Self> {
        if n_streams == 0 || phase_incs.len() % n_streams != 0 {
            return Err(FmdError { status: -1, message: "phase_incs must hold n_streams equal rows".into() });
        }
        let n_stations = phase_incs.len() / n_streams;
        let dev = DeviceConfig { n_channels: n_streams as u32, device_id, flags: 0 };
        let mut handle: *mut fmd_stations = std::ptr::null_mut();
        check(unsafe {
            fmd_stations_new(taps.as_ptr(), taps.len() as u32, decim, shift, phase_incs.as_ptr(), n_stations as u32, rate_out,
                             rate_resample, &dev, &mut handle)
        })?;
        Ok(StationBank { handle, decim, rate_out, rate_resample, n_streams, n_stations })
    }

    /// `iq` is `[n_streams][nbytes]`; returns audio `[n_streams][n_stations]`.
    pub fn demodulate(&mut self, iq: &[u8]) -> Result<Vec<Vec<Vec<i16>>>> {
        assert!(iq.len() % self.n_streams == 0, "iq must hold n_streams equal-sized buffers");
        let nbytes = iq.len() / self.n_streams;
        let cap = unsafe { fmd_stations_out_cap(self.decim, self.rate_out, self.rate_resample, nbytes) }.max(1);
        let rows = self.n_streams * self.n_stations;
        let mut out = vec![0i16; cap * rows];
        let mut lens = vec![0usize; rows];
        check(unsafe { fmd_stations_demodulate_batch(self.handle, iq.as_ptr(), nbytes, out.as_mut_ptr(), cap, lens.as_mut_ptr()) })?;
        Ok((0..self.n_streams)
            .map(|s| (0..self.n_stations).map(|k| { let r = s * self.n_stations + k; out[r * cap..r * cap + lens[r]].to_vec() }).collect())
            .collect())
    }

    pub fn reset(&mut self) -> Result<()> {
        check(unsafe { fmd_stations_reset(self.handle) })
    }
}

impl Drop for StationBank {
    fn drop(&mut self) {
        unsafe { fmd_stations_free(self.handle) }
    }
}

/// Channelizer (`fmd_channelizer_*`): `phase_incs.len() / n_streams` digital down-converters per wideband stream -- mix by the
/// station's offset, filter with `taps`, decimate by `decim` -- each returning the station's complex baseband as `(yr, yi)` i16
/// pairs (include/fmd.h).
pub struct Channelizer {
    handle: *mut fmd_channelizer,
    pub decim: u32,
    pub n_streams: usize,
    pub n_stations: usize,
}

unsafe impl Send for Channelizer {}

impl Channelizer {
    /// `phase_incs` is `[n_streams][n_stations]`.
    pub fn new(taps: &[i16], decim: u32, shift: u32, phase_incs: &[u32], n_streams: usize, device_id: i32) -> Result<Self> {
        if n_streams == 0 || phase_incs.len() % n_streams != 0 {
            return Err(FmdError { status: -1, message: "phase_incs must hold n_streams equal rows".into() });
        }
        let n_stations = phase_incs.len() / n_streams;
        let dev = DeviceConfig { n_channels: n_streams as u32, device_id, flags: 0 };
        let mut handle: *mut fmd_channelizer = std::ptr::null_mut();
        check(unsafe {
            fmd_channelizer_new(taps.as_ptr(), taps.len() as u32, decim, shift, phase_incs.as_ptr(), n_stations as u32, &dev, &mut handle)
        })?;
        Ok(Channelizer { handle, decim, n_streams, n_stations })
    }

    /// `iq` is `[n_streams][nbytes]`; returns interleaved `(yr, yi)` samples `[n_streams][n_stations]`.
    pub fn run(&mut self, iq: &[u8]) -> Result<Vec<Vec<Vec<i16>>>> {
        assert!(iq.len() % self.n_streams == 0, "iq must hold n_streams equal-sized buffers");
        let nbytes = iq.len() / self.n_streams;
        let cap = unsafe { fmd_channelizer_out_cap(self.decim, nbytes) }.max(1);
        let rows = self.n_streams * self.n_stations;
        let mut out = vec![0i16; 2 * cap * rows];
        let mut n = 0usize;
        check(unsafe { fmd_channelizer_run_batch(self.handle, iq.as_ptr(), nbytes, out.as_mut_ptr(), cap, &mut n) })?;
        Ok((0..self.n_streams)
            .map(|s| (0..self.n_stations).map(|k| { let r = s * self.n_stations + k; out[2 * r * cap..2 * (r * cap + n)].to_vec() }).collect())
            .collect())
    }

    /// Outputs per (stream, station) produced since creation or the last reset.
    pub fn outputs(&self) -> Result<u64> {
        let mut n = 0u64;
        check(unsafe { fmd_channelizer_outputs(self.handle, &mut n) })?;
        Ok(n)
    }

    pub fn reset(&mut self) -> Result<()> {
        check(unsafe { fmd_channelizer_reset(self.handle) })
    }
}

impl Drop for Channelizer {
    fn drop(&mut self) {
        unsafe { fmd_channelizer_free(self.handle) }
    }
}

/// Power spectrum (`fmd_spectrum_*`): the integrated power of `n_bins` DFT bins of each of `n_streams` streams, u64 in natural
/// DFT order (include/fmd.h).
pub struct Spectrum {
    handle: *mut fmd_spectrum,
    pub n_bins: u32,
    pub n_streams: usize,
}

unsafe impl Send for Spectrum {}

/// The library's exact integer Hann window (`amplitude` <= 127: one i8 digit per tap).
pub fn hann_window(n_bins: u32, amplitude: u32) -> Result<Vec<i16>> {
    let mut w = vec![0i16; n_bins as usize];
    check(unsafe { fmd_spectrum_hann(n_bins, amplitude, w.as_mut_ptr()) })?;
    Ok(w)
}

impl Spectrum {
    pub fn new(window: &[i16], hop: u32, shift: u32, n_streams: usize, device_id: i32) -> Result<Self> {
        let dev = DeviceConfig { n_channels: n_streams as u32, device_id, flags: 0 };
        let mut handle: *mut fmd_spectrum = std::ptr::null_mut();
        check(unsafe { fmd_spectrum_new(window.as_ptr(), window.len() as u32, hop, shift, &dev, &mut handle) })?;
        Ok(Spectrum { handle, n_bins: window.len() as u32, n_streams })
    }

    /// `iq` is `[n_streams][nbytes]`; returns `[n_streams][n_bins]`.
    pub fn power(&mut self, iq: &[u8]) -> Result<Vec<Vec<u64>>> {
        assert!(iq.len() % self.n_streams == 0, "iq must hold n_streams equal-sized buffers");
        let mut p = vec![0u64; self.n_streams * self.n_bins as usize];
        check(unsafe { fmd_spectrum_power_batch(self.handle, iq.as_ptr(), iq.len() / self.n_streams, p.as_mut_ptr()) })?;
        Ok(p.chunks(self.n_bins as usize).map(|c| c.to_vec()).collect())
    }

    /// The `StationBank` phase increment that tunes to the centre of `bin`.
    pub fn bin_inc(&self, bin: u32) -> Result<u32> {
        let mut inc = 0u32;
        check(unsafe { fmd_spectrum_bin_inc(bin, self.n_bins, &mut inc) })?;
        Ok(inc)
    }
}

impl Drop for Spectrum {
    fn drop(&mut self) {
        unsafe { fmd_spectrum_free(self.handle) }
    }
}

/// The producer side of the boundary as a trait: `RtlSdr::read_sync(&self, buf: &mut [u8]) -> Result<usize>`
/// (src/lib.rs:153).  The reference has no `read_async`; this does not add one.
pub trait IqSource {
    /// Fill `buf` with interleaved u8 I/Q; the number of bytes written, `< buf.len()` meaning samples were lost
    /// or the source ended (callers of the reference treat that as fatal, examples/simple_fm.rs:122).
    fn read_sync(&mut self, buf: &mut [u8]) -> std::result::Result<usize, Box<dyn std::error::Error>>;
}

/// File / stdin mode of the example (examples/simple_fm.rs:65-84): any `Read` is a source.
impl<R: std::io::Read> IqSource for R {
    fn read_sync(&mut self, buf: &mut [u8]) -> std::result::Result<usize, Box<dyn std::error::Error>> {
        let mut got = 0;
        while got < buf.len() {
            let n = self.read(&mut buf[got..])?;
            if n == 0 {
                break;
            }
            got += n;
        }
        Ok(got)
    }
}

/// An rtl_tcp server (the reference's own examples/rtl_tcp.rs, or osmocom's) as an `IqSource`: a dongle on another host
/// feeding the GPU `Demod`.  Handshake "RTL0" + tuner type + gain count (examples/rtl_tcp.rs:691-697), raw u8 IQ
/// (:609-631), 5-byte big-endian commands (:639-678) -- all behind `fmd_rtltcp_*` of the C ABI.
pub struct RtlTcpSource {
    handle: *mut fmd_rtltcp,
    pub tuner_type: u32,
    pub gain_count: u32,
}

unsafe impl Send for RtlTcpSource {}

impl RtlTcpSource {
    pub fn connect(host: &str, port: u16, timeout_ms: u32) -> Result<Self> {
        let chost = std::ffi::CString::new(host).map_err(|_| FmdError { status: -1, message: "host contains NUL".into() })?;
        let mut handle: *mut fmd_rtltcp = std::ptr::null_mut();
        check(unsafe { fmd_rtltcp_open(chost.as_ptr(), port, timeout_ms, &mut handle) })?;
        let (mut t, mut g) = (0u32, 0u32);
        check(unsafe { fmd_rtltcp_info(handle, &mut t, &mut g) })?;
        Ok(RtlTcpSource { handle, tuner_type: t, gain_count: g })
    }

    /// One 5-byte command (opcode + big-endian parameter); `config_sdr` of the example (examples/simple_fm.rs:217-229)
    /// maps to 0x03 (gain mode), 0x0e (bias tee), 0x01 (frequency), 0x02 (sample rate).
    pub fn command(&mut self, opcode: u8, param: u32) -> Result<()> {
        check(unsafe { fmd_rtltcp_command(self.handle, opcode, param) })
    }
}

impl IqSource for RtlTcpSource {
    fn read_sync(&mut self, buf: &mut [u8]) -> std::result::Result<usize, Box<dyn std::error::Error>> {
        let mut n: usize = 0;
        check(unsafe { fmd_rtltcp_read_sync(self.handle, buf.as_mut_ptr(), buf.len(), &mut n) })?;
        Ok(n)
    }
}

impl Drop for RtlTcpSource {
    fn drop(&mut self) {
        unsafe { fmd_rtltcp_close(self.handle) }
    }
}

/// `receive()` + `process()` of the example (examples/simple_fm.rs:100-170) in one loop: blocks of
/// `block_len` bytes (the reference uses DEFAULT_BUF_LENGTH = 262144, src/lib.rs:25) from `source` through the GPU
/// `Demod` into `sink` as raw native-endian s16 (`output()`, examples/simple_fm.rs:430-438).  A short final block
/// ends the stream as in the reference (:122-125).
pub fn run<S: IqSource, W: std::io::Write>(source: &mut S, demod: &mut Demod, sink: &mut W, block_len: usize)
    -> std::result::Result<u64, Box<dyn std::error::Error>> {
    let mut total = 0u64;
    let mut buf = vec![0u8; block_len];
    loop {
        let n = source.read_sync(&mut buf)?;
        if n < block_len {
            break;
        }
        let audio = demod.demodulate(buf.clone())?;
        let bytes = unsafe { std::slice::from_raw_parts(audio.as_ptr() as *const u8, audio.len() * 2) };
        sink.write_all(bytes)?;
        sink.flush()?;
        total += audio.len() as u64;
    }
    Ok(total)
}
