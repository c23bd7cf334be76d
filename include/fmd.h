/*
 * fmd.h -- C ABI of the MI355X-native FM demodulation path (libfmd_hip.so).
 *
 * Drop-in boundary for ONE path of ccostes/rtl-sdr-rs v0.3.1: the `Demod` chain of
 * examples/simple_fm.rs (u8 IQ -> rotate_90 -> centre -> boxcar decimate -> polar
 * discriminator -> fractional boxcar resampler -> s16).  Every entry point cites the
 * reference interface it replaces.  Plain pointers and sizes only; no C++/torch types.
 *
 * Threading: a handle is like the reference's `&mut Demod` -- one caller at a time.
 * Use one handle per host thread / per GPU.  Consecutive launches of one handle may go to different streams:
 * the library orders them (the new stream waits for the handle's previous launch); a stream handed to a
 * *_device entry point must stay alive until the handle's next call or fmd_demod_check.  Every entry point
 * leaves the caller's current HIP device as it found it.  All functions return FMD_OK (0) or a negative
 * fmd_status; nothing panics or aborts where the reference would.
 *
 * There is NO CPU fallback in this library: without a usable gfx950 device fmd_demod_new
 * fails with FMD_ERR_NO_DEVICE / FMD_ERR_HIP.
 */
#ifndef FMD_H
#define FMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FMD_VERSION_MAJOR 0
#define FMD_VERSION_MINOR 3

/* DEFAULT_BUF_LENGTH, src/lib.rs:25 -- the buffer size RtlSdr::read_sync callers use. */
#define FMD_DEFAULT_BUF_LENGTH (16 * 16384)

typedef enum fmd_status {
    FMD_OK = 0,
    FMD_ERR_INVALID_ARG   = -1,  /* NULL pointer, zero channels, ...                                */
    FMD_ERR_BAD_LENGTH    = -2,  /* nbytes % 8 != 0 -- reference: index panic, simple_fm.rs:286     */
    FMD_ERR_TOO_SHORT     = -3,  /* < 2 decimated samples -- reference: assert!, simple_fm.rs:356   */
    FMD_ERR_BAD_RATES     = -4,  /* rate_out < rate_resample or 0 -- reference: div by zero, :421   */
    FMD_ERR_CAPACITY      = -5,  /* out_cap smaller than the number of samples produced             */
    FMD_ERR_UNSUPPORTED   = -6,  /* configuration outside this implementation's documented domain   */
    FMD_ERR_BAD_STATE     = -7,  /* fmd_demod_set_state with a state no Demod can reach             */
    FMD_ERR_NO_DEVICE     = -8,  /* no gfx950 device / bad device_id                                */
    FMD_ERR_HIP           = -9,  /* a HIP runtime call failed; see fmd_last_error()                 */
    FMD_ERR_NOMEM         = -10,
    FMD_ERR_IO            = -11  /* rtl_tcp source: connect / handshake / socket error, see fmd_last_error()  */
} fmd_status;

/* struct RadioConfig, simple_fm.rs:173-176 */
typedef struct fmd_radio_config {
    uint32_t capture_freq;
    uint32_t capture_rate;
} fmd_radio_config;

/* struct DemodConfig, simple_fm.rs:179-185 (same field order). */
typedef struct fmd_demod_config {
    uint32_t rate_in;        /* stored, unused in arithmetic (reference: :180, logged :139)       */
    uint32_t rate_out;       /* "fast" rate of the audio resampler, :412                          */
    uint32_t rate_resample;  /* "slow" rate of the audio resampler, :411                          */
    uint32_t downsample;     /* boxcar length / decimation, :343                                  */
    uint32_t output_scale;   /* computed, unused in arithmetic (reference: :184,197-200)          */
} fmd_demod_config;

/* The mutable fields of struct Demod, simple_fm.rs:232-239.  This is the resumable state. */
typedef struct fmd_demod_state {
    uint32_t prev_index;      /* boxcar phase, 0 .. downsample-1                                  */
    int32_t  now_lpr;         /* partial audio sum                                                */
    int32_t  prev_lpr_index;  /* resampler phase, 0 .. rate_out-1                                 */
    int32_t  lp_now_re, lp_now_im;       /* partial boxcar sum                                    */
    int32_t  demod_pre_re, demod_pre_im; /* last decimated sample of the previous call            */
} fmd_demod_state;

/* Placement of a Demod bank on the machine (no reference counterpart: the reference is
 * one Demod on one CPU thread, simple_fm.rs:137). */
typedef struct fmd_device_config {
    uint32_t n_channels;  /* independent IQ streams (one reference `Demod` each); >= 1           */
    int32_t  device_id;   /* HIP device ordinal; -1 = current device                             */
    uint32_t flags;       /* reserved, 0                                                          */
} fmd_device_config;

typedef struct fmd_demod fmd_demod;   /* opaque; owns device buffers + per-channel state */

/* ---- configuration ------------------------------------------------------------------- */

/* optimal_settings(freq, rate), simple_fm.rs:189-214.  rate_resample is the reference's
 * RATE_RESAMPLE const (:27, 32000).  FMD_ERR_BAD_RATES where the reference divides by zero. */
int fmd_optimal_settings(uint32_t freq, uint32_t rate, uint32_t rate_resample,
                         fmd_radio_config *radio, fmd_demod_config *demod);

/* ---- lifecycle ------------------------------------------------------------------------ */

/* Demod::new(config), simple_fm.rs:243-252, for a bank of n_channels independent streams,
 * all with zeroed state.  downsample 1 ... 512 (FMD_ERR_UNSUPPORTED beyond).  From 129 up the
 * reference's own i32 arithmetic wraps at full-scale input (reproduced bit for bit); where a
 * release build of the reference would PANIC -- a zero divisor inside fast_atan2 after such a
 * wrap, reachable from downsample 305 with particular full-scale inputs -- the audio sample
 * that contains the discriminator value is unspecified (no status is raised). */
int fmd_demod_new(const fmd_demod_config *config, const fmd_device_config *dev, fmd_demod **out);

/* Drop for Demod. NULL is a no-op. */
void fmd_demod_free(fmd_demod *d);

/* Zero every channel's state (== dropping and re-creating the Demods). */
int fmd_demod_reset(fmd_demod *d);

/* ---- the hot path --------------------------------------------------------------------- */

/* Demod::demodulate(&mut self, buf: Vec<u8>) -> Vec<i16>, simple_fm.rs:256-269, for a
 * single-channel handle and HOST buffers: `iq` is exactly what RtlSdr::read_sync
 * (src/lib.rs:153) filled -- interleaved offset-binary u8 I,Q,I,Q...  Writes *out_len
 * samples to out (capacity out_cap samples; see fmd_out_cap).  The input is not modified. */
int fmd_demod_demodulate(fmd_demod *d, const uint8_t *iq, size_t nbytes,
                         int16_t *out, size_t out_cap, size_t *out_len);

/* The same for every channel of the bank, HOST buffers:
 *   iq      [n_channels][nbytes]   channel-major, contiguous
 *   out     [n_channels][out_cap]
 *   out_len [n_channels]
 * Elements of a row beyond its out_len (up to out_cap) are unspecified after the call. */
int fmd_demod_demodulate_batch(fmd_demod *d, const uint8_t *iq, size_t nbytes,
                               int16_t *out, size_t out_cap, size_t *out_len);

/* The same with DEVICE-resident buffers (the measured path): d_iq / d_out / d_out_len are
 * device pointers on the handle's GPU with the layouts above (d_iq 16-byte aligned;
 * d_out_len uint32, may be NULL).  Enqueues on `stream` (a hipStream_t; NULL = the
 * default stream) and returns without synchronising; the per-channel counts are also
 * available on the host, without a sync, from fmd_demod_last_out_len.
 * Stream lifetime: the library orders a handle's consecutive launches itself, also across different
 * streams, and fmd_demod_check completes behind the most recent launch ON ITS STREAM -- so the `stream`
 * of a handle's most recent _device call must stay alive until the handle's next _device call or
 * completion point (fmd_demod_check, _get_state, _set_state, a host entry point) has returned.  The
 * same rule holds for fmd_fir_filter_device and fmd_firdemod_demodulate_device.
 * Fast path: nbytes % 16 == 0 (every read_sync buffer: DEFAULT_BUF_LENGTH = 262144) and a bank whose
 * channels share one phase (banks fed equal-length buffers always do) take the kernels' short
 * prologues.  nbytes % 16 == 8 is legal (the reference only demands % 8, :284) and bit-exact, but runs the
 * general prologue -- a few percent slower, and for downsample 2 / 4 the LDS kernel instead of the
 * register-streaming one; fmd_demod_last_kernel reports which kernel a launch ran. */
int fmd_demod_demodulate_device(fmd_demod *d, const void *d_iq, size_t nbytes,
                                void *d_out, size_t out_cap, void *d_out_len, void *stream);

/* Several reference calls per launch.  Demod::demodulate takes the f64 atan2 path for the first
 * decimated sample of EVERY call (simple_fm.rs:359), so the audio of a stream depends on where
 * the caller cut it into buffers.  After fmd_demod_set_block_len(d, block_bytes) every
 * demodulate_* call is treated as the concatenation of nbytes / block_bytes consecutive
 * reference calls of block_bytes each (nbytes must be a multiple): one launch then returns
 * exactly the concatenated audio -- and leaves exactly the state -- of feeding the reference
 * those blocks one by one, e.g. 256 x DEFAULT_BUF_LENGTH in one 64 MiB launch.  block_bytes
 * % 8 == 0 and >= 4 * downsample bytes (every block yields >= 2 decimated samples, :356);
 * 0 (the default) switches it off: one call = one reference call. */
int fmd_demod_set_block_len(fmd_demod *d, size_t block_bytes);

/* Completion + verification point for the DEVICE entry point: waits for everything this handle has enqueued,
 * returns FMD_ERR_HIP if a device-side sizing assertion fired (fmd_last_error() has the bits), and settles the
 * one f64 sample of every reference call (Demod::polar_discriminant, simple_fm.rs:359,370-374 -- `atan2` from
 * the system libm in the reference): the kernel decides the axis / diagonal directions with integers and reports
 * every other sample whose value lies within 2^-20 of an integer; those few are re-evaluated here with the HOST
 * libm (the function the reference calls) and, if the truncated value differs, the audio sample (in the device
 * output buffer the launch wrote, which must still be allocated) or the carried partial sum is patched.
 * Outside that band the two results are provably equal.  The HOST entry points and fmd_demod_get_state do this
 * themselves before returning; after fmd_demod_demodulate_device call it before reading the output.  Only the output
 * buffers of the THREE most recent launches are ever written by a patch (they must still be allocated; round 5: the most recent
 * one only); a sample of an OLDER launch that turns out to need one (probability ~2^-36 per reference call) makes this function
 * return FMD_ERR_HIP instead of touching memory the caller may have reused: for the strict bit-exactness guarantee call it --
 * or fmd_demod_check_behind, which does not serialise -- for every launch. */
int fmd_demod_check(fmd_demod *d);

/* The same completion point ONE or TWO LAUNCHES BACK (round 6): with launches 1 ... n enqueued through fmd_demod_demodulate_device,
 * fmd_demod_check_behind(d, back) waits until launch n - back has completed -- not for the newer ones -- and settles ITS f64 samples,
 * so that the reference's cadence
 *     loop { buf = read_sync(); audio = demod.demodulate(buf); output(audio); }        (simple_fm.rs:150-156)
 * runs as  enqueue(buf n); fmd_demod_check_behind(d, 2); output(audio n - 2);  with the GPU never idle between launches and the
 * strict bit-exactness guarantee intact (fmd_demod_check after every launch serialises host and device: ~8 % at the headline
 * configuration; this cadence: 1.00 - 1.01 x the bare launches, extra.check_pipelined of the bench line).  back = 2 keeps a whole
 * launch queued behind the running one, which absorbs a late host; back = 1 keeps none; back = 0 is fmd_demod_check.  How: launch
 * s + 1 cannot start before launch s has completed, so its first tile posts "s is done" together with whether s reported anything
 * into host-mapped memory; everything a launch leaves behind -- its report buffer, the state it wrote, its launch record -- lives in
 * a ring of three.  A launch that DID report guarded samples is settled while the newer ones run as well (its records are copied and
 * its audio samples patched on the handle's own stream); only a correction of the sum it carried into the next launch, or a device
 * assertion, waits for everything.
 * Contract: until a launch has been settled by this function or by fmd_demod_check, (a) its OUTPUT buffer stays allocated and
 * unread -- a patch goes into the buffer of the launch that produced the sample, for the last THREE launches -- and (b) its INPUT
 * buffer stays unmodified: in the one case where a launch's corrected sample lies in the partial sum it carried into the next launch
 * (probability ~2^-36 per reference call), the launches behind it are run again on the corrected state, inside this call.  Launches
 * are settled IN ORDER (an older unsettled launch turns the call into fmd_demod_check).  Returns FMD_OK at once when fewer than
 * back + 1 launches are outstanding; falls back to fmd_demod_check where no post is coming (generic kernel).  Call fmd_demod_check
 * after the LAST launch of a run.  (fmd_firdemod / the pipelined sink have their own completion points.) */
int fmd_demod_check_behind(fmd_demod *d, uint32_t back);
/* fmd_demod_check_behind(d, 1). */
int fmd_demod_check_prev(fmd_demod *d);

/* EVENT ORDERING (opt-in, round 6): with on != 0 the handle records an event behind every launch and every later wait -- the next
 * launch on another stream, fmd_demod_check / _check_prev / _get_state -- goes to that EVENT: a `stream` handed to
 * fmd_demod_demodulate_device is never used again once that call has returned, so the stream lifetime rule above does not apply (for
 * callers whose streams come from a pool that may destroy them).  Costs the record: +2 - 3 % per launch at the headline rates, which
 * is why it is not the default.  Synchronises the device; call it between launches. */
int fmd_demod_set_event_ordering(fmd_demod *d, int on);

/* Diagnostics of the above: f64 samples that fell into the guard band / whose value had to be patched. */
int fmd_demod_f64_stats(const fmd_demod *d, uint64_t *guarded, uint64_t *patched);

/* Per-channel sample counts of the most recent demodulate_* call (host bookkeeping). */
int fmd_demod_last_out_len(const fmd_demod *d, size_t *out_len /* [n_channels] */);

/* Upper bound of samples one call can produce per channel for nbytes of input. */
size_t fmd_out_cap(const fmd_demod_config *config, size_t nbytes);

/* Page-locked host buffers for the HOST entry points above.  The reference reads into a pageable
 * heap buffer and sends a copy of it per block (simple_fm.rs:114,127 `buf.to_vec()`); a binding that takes
 * its read buffers from here instead lets the copy engine DMA straight out of them (no staging
 * copy through the runtime's bounce buffers).  Plain pageable pointers keep working. */
int fmd_host_alloc(size_t nbytes, void **ptr);
int fmd_host_free(void *ptr);

/* ---- state (checkpoint / resume; simple_fm.rs:232-239) -------------------------------- */
int fmd_demod_get_state(fmd_demod *d, uint32_t channel, fmd_demod_state *state);
int fmd_demod_set_state(fmd_demod *d, uint32_t channel, const fmd_demod_state *state);

/* ---- synthetic IQ source (stands in for the absent capture.bin) -------- */

typedef struct fmd_synth_params {
    uint64_t seed;          /* channel c uses seed + c                                            */
    uint32_t amplitude;     /* carrier amplitude in LSB, <= 120                                   */
    uint32_t noise;         /* uniform noise in [-noise, +noise] LSB                              */
    uint32_t dev_q32;       /* peak frequency deviation, cycles/sample in Q32                     */
    uint32_t mod_period;    /* triangle modulation period in samples (even, >= 2)                 */
} fmd_synth_params;

/* Fill d_iq [n_channels][nbytes] (device pointer) with a deterministic integer-only FM
 * signal sitting at -Fs/4 (what offset tuning, simple_fm.rs:194-195, delivers).
 * rtl-sdr-rs_amd/synth.py generates identical bytes with numpy. */
int fmd_synth_fill_device(int device_id, void *d_iq, uint32_t n_channels, size_t nbytes,
                          uint64_t sample_offset, const fmd_synth_params *p, void *stream);

/* ---- generalised tapped decimating FIR (SURVEY 8a row G', BASELINE config 4) ----------- */
/* NOT a reference interface: the reference's only tapped FIR lives in the RTL2832U chip
 * (src/rtlsdr.rs:525-558).  Definition (also oracle/fm_oracle.h):
 *     y[m] = sum_{t < n_taps} taps[t] * x[decim * m + t]
 * over the stream x[n] of rotated (rotate_90, simple_fm.rs:276-299) and centred (`- 127`, :258)
 * complex samples of one channel, counted from the first sample fed after fmd_fir_new /
 * fmd_fir_reset; y[m] is produced by the call in which x[decim*m + n_taps - 1] arrives.
 * With taps = 1...1 and n_taps == decim == downsample it is Demod::low_pass_complex (:337-352).
 * decim must be even (whole-dword windows), 1 <= n_taps <= 1024, |taps| <= 2047. */
typedef struct fmd_fir fmd_fir;
int fmd_fir_new(const int16_t *taps, uint32_t n_taps, uint32_t decim, const fmd_device_config *dev,
                fmd_fir **out);
void fmd_fir_free(fmd_fir *f);
int fmd_fir_reset(fmd_fir *f);
/* Which form the handle runs (introspection for tests and bench lines): 1 = matrix cores with one i8 digit per tap (every
 * |tap| <= 127: eight outputs per operand column), 2 = two digits (|tap| <= 2047: four), 0 = the vector-pipe kernel
 * (decim > 64 or a filter too long for the matrix-core form). */
int fmd_fir_tap_digits(const fmd_fir *f);
/* Name of the kernel this handle launches, as `rocprofv3 --kernel-trace` prints it (see fmd_demod_last_kernel). */
int fmd_fir_kernel_name(const fmd_fir *f, char *name, size_t cap);
/* Complex outputs one call of nbytes can produce per channel (upper bound). */
size_t fmd_fir_out_cap(uint32_t n_taps, uint32_t decim, size_t nbytes);
/* HOST buffers: iq [n_channels][nbytes]; out [n_channels][out_cap][2] int32 (re, im);
 * out_len [n_channels] complex samples written. */
int fmd_fir_filter_batch(fmd_fir *f, const uint8_t *iq, size_t nbytes, int32_t *out, size_t out_cap,
                         size_t *out_len);
/* DEVICE buffers with the same layouts, enqueued on `stream` without synchronising; the
 * per-channel count (identical for all channels) is returned in *out_len_each. */
int fmd_fir_filter_device(fmd_fir *f, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap,
                          size_t *out_len_each, void *stream);

/* ---- tapped FIR -> discriminator -> resampler in one kernel (BASELINE north_star: "FIR + demod + resample fused") -- */
/* NOT a reference interface either.  Definition: Demod::demodulate (simple_fm.rs:256-269) with low_pass_complex
 * (:337-352) replaced by the tapped decimating FIR above, normalised by a right shift,
 *     lp[m] = floor( sum_{t < n_taps} taps[t] * x[decim * m + t] / 2^shift ),
 * followed by the reference's own fm_demod (:355-367, the f64 sample at the first filter output of every call) and
 * low_pass_real (:408-426, rate_out -> rate_resample).  With taps = 1...1, n_taps == decim == downsample, shift == 0
 * it returns exactly what fmd_demod_* (and the oracle of the reference chain) return -- tested bit for bit; that is
 * its anchor.  (An 8-bit filter -- every |tap| <= 127 -- takes a form of the matrix-core kernels with one i8 digit per tap and
 * eight outputs per operand column, here and in fmd_fir_*: same results, fewer matrix instructions.)
 * Domain: decim even and <= 64, 1 <= n_taps <= 1024, |taps| <= 2047, (128 * sum|taps|) >> shift <= 16384 (so that
 * |lp| stays in the discriminator's range, the boxcar's bound at downsample 128), shift <= 24.  A shift that brings
 * (128 * sum|taps|) >> shift down to 2048 -- the boxcar's range at downsample 16 -- selects the kernel's f32 form of
 * the discriminator (same results, ~8 % faster); the Python mirror's auto_shift() picks that one by default.
 * A call that yields fewer than 2 filter outputs returns FMD_ERR_TOO_SHORT (assert at :356) and changes nothing.
 * All channels of a bank advance together (equal-sized buffers), so there is no per-channel set_state; the bank as a
 * whole is saved and restored with fmd_firdemod_checkpoint / fmd_firdemod_resume. */
typedef struct fmd_firdemod fmd_firdemod;
int fmd_firdemod_new(const int16_t *taps, uint32_t n_taps, uint32_t decim, uint32_t shift, uint32_t rate_out,
                     uint32_t rate_resample, const fmd_device_config *dev, fmd_firdemod **out);
void fmd_firdemod_free(fmd_firdemod *f);
int fmd_firdemod_reset(fmd_firdemod *f);
/* Audio samples one call of nbytes can produce per channel (upper bound). */
size_t fmd_firdemod_out_cap(uint32_t decim, uint32_t rate_out, uint32_t rate_resample, size_t nbytes);
/* HOST buffers: iq [n_channels][nbytes]; out [n_channels][out_cap] s16; out_len [n_channels]. */
int fmd_firdemod_demodulate_batch(fmd_firdemod *f, const uint8_t *iq, size_t nbytes, int16_t *out, size_t out_cap,
                                  size_t *out_len);
/* DEVICE buffers, enqueued on `stream` without synchronising; the per-channel count (identical for all channels)
 * is returned in *out_len_each.  fmd_firdemod_check is its completion / verification point (see fmd_demod_check). */
int fmd_firdemod_demodulate_device(fmd_firdemod *f, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap,
                                   size_t *out_len_each, void *stream);
int fmd_firdemod_check(fmd_firdemod *f);
/* demod_pre, now_lpr, prev_lpr_index of one channel (prev_index / lp_now are 0: the FIR owns the decimation). */
int fmd_firdemod_get_state(fmd_firdemod *f, uint32_t channel, fmd_demod_state *state);
/* Checkpoint / resume of the WHOLE bank (its channels advance together, so the unit is the bank, not a channel): the
 * sample position, the resampler phase, and per channel now_lpr, demod_pre and the filter's history (the last
 * n_taps - 1 samples).  A bank resumed from a checkpoint continues bit for bit as the one it was taken from would
 * have; the blob is host memory, little-endian, and names the filter (taps, decim, shift, rates, channel count) it
 * belongs to -- fmd_firdemod_resume on any other bank, or on a damaged blob, returns FMD_ERR_BAD_STATE and changes
 * nothing.  Both calls synchronise the device first. */
size_t fmd_firdemod_checkpoint_size(const fmd_firdemod *f);
int fmd_firdemod_checkpoint(fmd_firdemod *f, void *blob, size_t cap);
int fmd_firdemod_resume(fmd_firdemod *f, const void *blob, size_t size);
int fmd_firdemod_f64_stats(const fmd_firdemod *f, uint64_t *guarded, uint64_t *patched);
int fmd_firdemod_tiling(const fmd_firdemod *f, uint32_t *audio_per_tile, uint32_t *lds_bytes);
/* Name of the kernel this handle launches, as `rocprofv3 --kernel-trace` prints it (see fmd_demod_last_kernel). */
int fmd_firdemod_kernel_name(const fmd_firdemod *f, char *name, size_t cap);

/* ---- station bank: many FM stations out of one wideband stream --------------------------------------------- */
/* NEW SURFACE (the reference demodulates ONE station per stream, the one offset tuning puts at -Fs/4, simple_fm.rs:194-195).
 * A bank runs K digital down-converters per input stream -- mix by the station's offset, filter, decimate -- each followed by
 * the reference's own fm_demod (:355-367) and low_pass_real (:408-426).  Definition (integers only; tests/stations_ref.py):
 *   c[n]      = (b[2n] - 127) + j (b[2n+1] - 127)                 raw read_sync bytes, NO rotate_90 (the mixer tunes)
 *   TAB[i]    = round(16384 cos(2 pi i / 1024)); cosq(p) = TAB[p >> 22], sinq(p) = TAB[((p >> 22) - 256) & 1023]
 *   W[k][t]   = rnd(h[t] cosq(t inc_k)) + j rnd(-h[t] sinq(t inc_k)),  rnd(v) = (v + 8192) >> 14   (one real prototype h)
 *   z[k][m]   = sum_{t < n_taps} W[k][t] c[decim m + t]               (output m comes with the call in which its last sample arrives)
 *   y[k][m]   = (z * (cosq(psi) + j sinq(psi))) >> (14 + shift),  psi = m decim inc_k mod 2^32 (floor, per component, in i64)
 * then fm_demod (f64 sample at the first output of every call, demod_pre carried) and low_pass_real per (stream, station), s16 out.
 * With inc = 0 the taps are h, y = floor(z / 2^shift): fmd_firdemod on UNROTATED samples.  Feeding rot(B) -- the bytes rotate_90
 * would make -- with h = 1...1, n_taps == decim, shift = 0 gives exactly fmd_demod(B).
 * Domain: decim even, 2 ... 64; 1 <= n_taps <= 256; |h| <= 2047; 1 <= n_stations <= 32; any phase_inc; shift <= 24;
 * ceil(256 * max_k sum_t (|Wr| + |Wi|) / 2^shift) <= 16384 (|y| <= 16384; <= 2048 selects the f32 discriminator, same results);
 * rate_out >= rate_resample >= 1 (else FMD_ERR_BAD_RATES); nbytes % 8 == 0 (else FMD_ERR_BAD_LENGTH).  Rates, with g = gcd(rate_out,
 * rate_resample) and c = ceil(rate_out / rate_resample): rate_out / g <= 2^24, 3 rate_resample / g < 2^24, and one audio sample must
 * fit a tile -- 2c + 3 <= 256 filter outputs (c <= 126) in raw + 2048 + 4 n_stations (2c + 3) + 24 <= 65536 bytes of LDS, where
 * raw = roundup16(max(12 + 6 decim + 8 decim (16 ceil((2c + 3) / 64) - 1) + 64 ceil((12 + 2 n_taps) / 64), 12 + 2 decim (2c + 2) +
 * 2 n_taps + 15)).  So c <= 116 fits every shape, c > 126 none (decim 2 from 2.4 Msps to 8 kHz: c = 150).  Everything else outside
 * it is FMD_ERR_UNSUPPORTED, decided before a device is touched.  A call with fewer than 2 filter outputs returns
 * FMD_ERR_TOO_SHORT and changes nothing.
 * Layouts: iq [n_streams][nbytes], out [n_streams][n_stations][out_cap], phase_inc [n_streams][n_stations]; n_streams is
 * dev->n_channels.  Stream lifetime and completion points: as fmd_firdemod_* (fmd_stations_check).  The f64 reports name the
 * logical channel stream * n_stations + station. */
typedef struct fmd_stations fmd_stations;
/* floor((offset_hz * 2^32 + floor(capture_rate / 2)) / capture_rate) mod 2^32 in exact integers; needs 2 |offset_hz| <= capture_rate. */
int fmd_stations_phase_inc(int32_t offset_hz, uint32_t capture_rate, uint32_t *inc);
/* The NCO table TAB above, 1024 entries. */
int fmd_stations_nco_table(int16_t *table);
int fmd_stations_new(const int16_t *taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t *phase_inc,
                     uint32_t n_stations, uint32_t rate_out, uint32_t rate_resample, const fmd_device_config *dev,
                     fmd_stations **out);
void fmd_stations_free(fmd_stations *b);
int fmd_stations_reset(fmd_stations *b);
/* Audio samples one call of nbytes can produce per (stream, station) (upper bound); 0 for decim or rate_out 0. */
size_t fmd_stations_out_cap(uint32_t decim, uint32_t rate_out, uint32_t rate_resample, size_t nbytes);
/* HOST buffers; out_len [n_streams * n_stations]. */
int fmd_stations_demodulate_batch(fmd_stations *b, const uint8_t *iq, size_t nbytes, int16_t *out, size_t out_cap,
                                  size_t *out_len);
/* DEVICE buffers, enqueued on `stream` without synchronising; *out_len_each = audio samples per (stream, station). */
int fmd_stations_demodulate_device(fmd_stations *b, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap,
                                   size_t *out_len_each, void *stream);
int fmd_stations_check(fmd_stations *b);
/* demod_pre, now_lpr, prev_lpr_index of one (stream, station); prev_index / lp_now are 0. */
int fmd_stations_get_state(fmd_stations *b, uint32_t stream, uint32_t station, fmd_demod_state *state);
int fmd_stations_f64_stats(const fmd_stations *b, uint64_t *guarded, uint64_t *patched);
/* Name of the kernel this bank launches, as `rocprofv3 --kernel-trace` prints it. */
int fmd_stations_kernel_name(const fmd_stations *b, char *name, size_t cap);

/* ---- channelizer: each station's narrowband IQ out of one wideband stream ---------------------------------- */
/* NEW SURFACE (rtl_fm -M raw in the rtl-sdr ecosystem; the reference has none).  K digital down-converters per input stream, each
 * returning the station's decimated complex baseband -- the station bank's y, before any demodulator.  Definition (integers only;
 * tests/channelizer_ref.py): the station bank's c, TAB, cosq / sinq, W[k][t], z[k][m] and
 *   y[k][m]   = (z * (cosq(psi) + j sinq(psi))) >> (14 + shift),  psi = m decim inc_k mod 2^32 (floor, per component, in i64)
 * exactly as above (output m comes with the call in which its last sample arrives; the filter history and m carry across calls),
 * stored as the int16 pair (yr, yi).  No fm_demod, no resampler: the station bank is this followed by fm_demod + low_pass_real.
 * With inc = 0, h = 1...1, n_taps == decim and shift = 0, fed rot(B), it is low_pass_complex (simple_fm.rs:337-352) of B.
 * Domain: the station bank's filter domain -- decim even, 2 ... 64; 1 <= n_taps <= 256; |h| <= 2047; 1 <= n_stations <= 32; any
 * phase_inc; shift <= 24; ceil(256 * max_k sum_t (|Wr| + |Wi|) / 2^shift) <= 16384, so |y| <= 16384 and the int16 output is exact.
 * nbytes % 8 != 0 -> FMD_ERR_BAD_LENGTH; a call that completes no output -> FMD_ERR_TOO_SHORT and nothing changes; everything else
 * outside the domain -> FMD_ERR_UNSUPPORTED, decided before a device is touched.
 * Layouts: iq [n_streams][nbytes], out [n_streams][n_stations][out_cap][2] int16 (yr, yi), phase_inc [n_streams][n_stations];
 * n_streams is dev->n_channels.  Stream lifetime and completion points: as fmd_stations_* (fmd_channelizer_check). */
typedef struct fmd_channelizer fmd_channelizer;
int fmd_channelizer_new(const int16_t *taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t *phase_inc,
                        uint32_t n_stations, const fmd_device_config *dev, fmd_channelizer **out);
void fmd_channelizer_free(fmd_channelizer *c);
int fmd_channelizer_reset(fmd_channelizer *c);
/* ceil(nbytes / (2 decim)): outputs one call of nbytes can produce per (stream, station), whatever the history; 0 for decim 0. */
size_t fmd_channelizer_out_cap(uint32_t decim, size_t nbytes);
/* HOST buffers; *out_len = outputs per (stream, station) (the same for all). */
int fmd_channelizer_run_batch(fmd_channelizer *c, const uint8_t *iq, size_t nbytes, int16_t *out, size_t out_cap,
                              size_t *out_len);
/* DEVICE buffers (d_iq and d_out 4-byte aligned), enqueued on `stream` without synchronising; *out_len as above. */
int fmd_channelizer_run_device(fmd_channelizer *c, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap,
                               size_t *out_len, void *stream);
int fmd_channelizer_check(fmd_channelizer *c);
/* Outputs per (stream, station) produced since creation or the last reset: the next output's index m (to timestamp samples). */
int fmd_channelizer_outputs(const fmd_channelizer *c, uint64_t *outputs);
/* Name of the kernel this handle launches, as `rocprofv3 --kernel-trace` prints it. */
int fmd_channelizer_kernel_name(const fmd_channelizer *c, char *name, size_t cap);

/* ---- stereo station bank: pilot-locked L/R audio per FM station ---------------------------------------------- */
/* NEW SURFACE (the reference demodulates mono only).  This is the project's own operator, not the reference's chain: the
 * channelizer's y, the reference's integer discriminator at the multiplex (MPX) rate, a block-wise pilot estimate and a
 * FIR on the sum and the difference signal.  Definition (integers only; tests/stereo_ref.py), per (stream, station k):
 *   y[m]      the channelizer's output (above), m counted from creation or reset
 *   x[m]      = (i16) polar_discriminant_fast(y[m], y[m-1])        (simple_fm.rs:377-405; y[-1] = 0, y[m-1] carries across calls)
 *   inc_p     = floor((19000 decim 2^32 + floor(capture_rate / 2)) / capture_rate) mod 2^32,  theta_m = m inc_p mod 2^32
 *   block j   = the samples m with floor(m / P) = j;  I_j = sum x[m] cosq(theta_m),  Q_j = sum x[m] sinq(theta_m)  (exact, i64)
 *   present_j = pilot_min > 0 && I_j^2 + Q_j^2 >= (pilot_min P 8192)^2                                          (exact, 128-bit)
 *   e = max(0, bitlen(max(|I_j|, |Q_j|)) - 23),  a = I_j >> e,  b = Q_j >> e,  E = a^2 + b^2
 *   c2_j = tdiv((b^2 - a^2) << 14, E),  s2_j = tdiv((2 a b) << 14, E)          (cos 2 alpha, sin 2 alpha in Q14; tdiv truncates)
 *   kc[m] = (sinq(2 theta_m) c2 + cosq(2 theta_m) s2) >> 13 with the estimate of block j - 1 = floor(m / P) - 1 when that block is
 *           present, 0 otherwise (block -1 is absent): 2 sin(2 theta + 2 alpha) in Q14 for a pilot A sin(theta + alpha)
 *   s[m]  = (x[m] kc[m]) >> 14
 *   M[n]  = sum_t g[t] x[R n + t],  S[n] = sum_t g[t] s[R n + t]     (t < Ta; exact in i32)
 *   L[n]  = sat16((M + S) >> (audio_shift + 1)),  Rch[n] = sat16((M - S) >> (audio_shift + 1))
 * Shifts are arithmetic (floor).  Audio sample n comes with the call in which x[R n + Ta - 1] arrives; out is
 * [n_streams][n_stations][out_cap][2] int16 (L, R): interleaved stereo s16 at capture_rate / (decim R).
 * Domain (else FMD_ERR_UNSUPPORTED, decided before a device is queried): the channelizer's filter domain; capture_rate >=
 * 106000 decim; P a power of two in [1024, 16384]; 1 <= R <= 32; 1 <= Ta <= 256; sum |g| <= 16383; audio_shift <= 16;
 * pilot_min <= 16384 (0: every block is absent, the output is mono).  nbytes % 8 != 0 -> FMD_ERR_BAD_LENGTH; a call that completes
 * no audio sample -> FMD_ERR_TOO_SHORT and changes nothing.  Stream lifetime and completion points: as fmd_channelizer_*. */
typedef struct fmd_stereo fmd_stereo;
typedef struct fmd_stereo_config {
    uint32_t capture_rate;   /* Hz: sets the pilot step inc_p                                         */
    uint32_t block;          /* P: pilot-estimate block length in MPX samples                         */
    uint32_t audio_decim;    /* R                                                                     */
    uint32_t audio_shift;
    uint32_t pilot_min;      /* presence threshold in discriminator units (the pilot's amplitude in x) */
} fmd_stereo_config;
int fmd_stereo_new(const int16_t *taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t *phase_inc,
                   uint32_t n_stations, const int16_t *audio_taps, uint32_t n_audio_taps, const fmd_stereo_config *cfg,
                   const fmd_device_config *dev, fmd_stereo **out);
void fmd_stereo_free(fmd_stereo *s);
int fmd_stereo_reset(fmd_stereo *s);
/* ceil(nbytes / (2 decim R)): audio samples one call of nbytes can complete per (stream, station), whatever the history;
 * 0 for decim 0 or R 0. */
size_t fmd_stereo_out_cap(uint32_t decim, uint32_t audio_decim, size_t nbytes);
/* HOST buffers; *out_len = audio samples per (stream, station) (the same for all). */
int fmd_stereo_run_batch(fmd_stereo *s, const uint8_t *iq, size_t nbytes, int16_t *out, size_t out_cap, size_t *out_len);
/* DEVICE buffers (d_iq and d_out 4-byte aligned), enqueued on `stream` without synchronising; *out_len as above. */
int fmd_stereo_run_device(fmd_stereo *s, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap, size_t *out_len,
                          void *stream);
int fmd_stereo_check(fmd_stereo *s);
/* Audio samples per (stream, station) produced since creation or the last reset. */
int fmd_stereo_outputs(const fmd_stereo *s, uint64_t *outputs);
/* The last completed block's pilot: *present = present_j, *level = isqrt(I_j^2 + Q_j^2) / (P 8192), the pilot amplitude in
 * discriminator units (0 and 0 before the first block completes).  Synchronises first. */
int fmd_stereo_pilot(fmd_stereo *s, uint32_t stream, uint32_t station, int *present, uint32_t *level);
/* inc_p of the definition; FMD_ERR_INVALID_ARG for capture_rate 0 or decim 0. */
int fmd_stereo_pilot_inc(uint32_t capture_rate, uint32_t decim, uint32_t *inc);
/* Name of pass 0 (front end + discriminator + pilot sums) or 1 (carrier, FIRs, matrix), as `rocprofv3 --kernel-trace` prints it. */
int fmd_stereo_kernel_name(const fmd_stereo *s, uint32_t pass, char *name, size_t cap);

/* ---- RDS bank: each FM station's 57 kHz subcarrier as a low-rate complex baseband --------------------------- */
/* NEW SURFACE (the reference has none).  The wideband half of RDS reception, feed-forward and in integers; the sequential half
 * (carrier and symbol timing, block synchronisation, groups) is fmd_rds_decoder_* below, on the host.  Definition (integers only;
 * tests/rds_ref.py), per (stream, station k):
 *   y[m], x[m], inc_p, theta_m, I_j, Q_j   exactly the stereo station bank's (above); m counted from creation or reset, y[m-1]
 *                                          carried across calls
 *   phi_m  = 3 m inc_p mod 2^32                                (the free-running 57 kHz carrier: three times the pilot step)
 *   qr[m]  = (x[m] cosq(phi_m)) >> 14,   qi[m] = (-x[m] sinq(phi_m)) >> 14                                    (|q| <= 32768)
 *   vr[n]  = sum_{t < Ta} g[t] qr[R n + t],   vi[n] likewise            (exact in i32: sum |g| <= 16383, so |v| < 2^29)
 *   u[n]   = (vr >> rds_shift, vi >> rds_shift)                          stored as the int16 pair (ur, ui)
 * Shifts are arithmetic (floor).  Sample n comes with the call in which x[R n + Ta - 1] arrives; out is
 * [n_streams][n_stations][out_cap][2] int16 at capture_rate / (decim R).  The carrier is NOT corrected by the pilot estimate: the
 * residual (three times the transmitter's pilot error plus the rounding of inc_p, a few Hz) is left to the host decoder, which
 * keeps the device operator free of per-block divisions.  The output does not depend on how the stream is cut into calls.
 * Domain (else FMD_ERR_UNSUPPORTED, decided before a device is queried): the channelizer's filter domain; capture_rate >=
 * 120000 decim (the subcarrier's upper sideband at 59.4 kHz lies below half the multiplex rate); P a power of two in
 * [1024, 16384]; 1 <= R <= 32; 1 <= Ta <= 256; sum |g| <= 16383; rds_shift <= 24 and ceil(32768 sum |g| / 2^rds_shift) <= 32767,
 * so the int16 store is exact; pilot_min <= 16384.  nbytes % 8 != 0 -> FMD_ERR_BAD_LENGTH; a call that completes no output ->
 * FMD_ERR_TOO_SHORT and changes nothing.  Stream lifetime and completion points: as fmd_channelizer_* (fmd_rds_check). */
typedef struct fmd_rds fmd_rds;
typedef struct fmd_rds_config {
    uint32_t capture_rate;   /* Hz: sets the pilot step inc_p                                         */
    uint32_t block;          /* P: pilot block length in MPX samples (fmd_rds_pilot)                  */
    uint32_t out_decim;      /* R                                                                     */
    uint32_t rds_shift;
    uint32_t pilot_min;      /* presence threshold of fmd_rds_pilot, in discriminator units           */
} fmd_rds_config;
int fmd_rds_new(const int16_t *taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t *phase_inc,
                uint32_t n_stations, const int16_t *rds_taps, uint32_t n_rds_taps, const fmd_rds_config *cfg,
                const fmd_device_config *dev, fmd_rds **out);
void fmd_rds_free(fmd_rds *s);
int fmd_rds_reset(fmd_rds *s);
/* ceil(nbytes / (2 decim R)): outputs one call of nbytes can complete per (stream, station), whatever the history; 0 for decim 0
 * or R 0. */
size_t fmd_rds_out_cap(uint32_t decim, uint32_t out_decim, size_t nbytes);
/* HOST buffers; *out_len = outputs per (stream, station) (the same for all). */
int fmd_rds_run_batch(fmd_rds *s, const uint8_t *iq, size_t nbytes, int16_t *out, size_t out_cap, size_t *out_len);
/* DEVICE buffers (d_iq and d_out 4-byte aligned), enqueued on `stream` without synchronising; *out_len as above. */
int fmd_rds_run_device(fmd_rds *s, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap, size_t *out_len,
                       void *stream);
int fmd_rds_check(fmd_rds *s);
/* Outputs per (stream, station) produced since creation or the last reset. */
int fmd_rds_outputs(const fmd_rds *s, uint64_t *outputs);
/* The last completed block's pilot, with the semantics of fmd_stereo_pilot: a station without a pilot has no multiplex to decode.
 * Synchronises first. */
int fmd_rds_pilot(fmd_rds *s, uint32_t stream, uint32_t station, int *present, uint32_t *level);
/* Name of pass 0 (the stereo bank's multiplex pass) or 1 (carrier, FIRs, shift), as `rocprofv3 --kernel-trace` prints it. */
int fmd_rds_kernel_name(const fmd_rds *s, uint32_t pass, char *name, size_t cap);

/* ---- RDS decoder (host): groups, PI, PS and RadioText from one station's RDS baseband ----------------------- */
/* No GPU.  One decoder handles one (stream, station) of an RDS bank and keeps its state across pushes; what it returns does not
 * depend on how the samples are cut into pushes.  Floating point inside: this layer is defined by what it decodes (IEC 62106:
 * 1187.5 bit/s, biphase symbols, differential coding, 26-bit blocks with the generator x^10 + x^8 + x^7 + x^5 + x^4 + x^3 + 1 and
 * the offset words A 0x0FC, B 0x198, C 0x168, C' 0x350, D 0x1B4), not bit for bit.
 *   carrier   a Costas loop on the matched-filter output (residual up to +-20 Hz; the pi ambiguity is harmless)
 *   timing    the 1187.5 Hz line of the squared matched-filter envelope (feed-forward), linear interpolation at the bit centre
 *   blocks    a block is used only when its syndrome -- the remainder of the 26 bits by the generator -- equals its offset word; no
 *             error correction.  Lock on two consecutive valid blocks in sequence; lock is dropped after 10 bad blocks in a row.
 *   groups    PI from block A; PS from 0A / 0B; RadioText from 2A / 2B (a change of the text A/B flag clears the buffer, 0x0D ends
 *             the text); every group completed while locked is delivered raw, whatever its type.
 * rate_num / rate_den Hz is the sample rate: 4 kHz ... 32 kHz, else FMD_ERR_UNSUPPORTED. */
typedef struct fmd_rds_decoder fmd_rds_decoder;
typedef struct fmd_rds_group {
    uint16_t block[4];       /* the 16 information bits of blocks A, B, C / C', D                      */
    uint8_t ok_mask;         /* bit i: block i passed its check                                        */
    uint64_t first_sample;   /* index, since creation or reset, of the sample at the group's first bit */
} fmd_rds_group;
typedef struct fmd_rds_info {
    uint16_t pi;             /* 0 until a block A (or a C' of a B group) passed                         */
    char ps[9];              /* 8 characters, spaces where nothing arrived yet, NUL-terminated         */
    char rt[65];             /* the text up to 0x0D or the first segment not yet received, NUL-terminated */
    uint64_t groups_ok;      /* groups with all four blocks valid                                      */
    uint64_t blocks_bad;     /* blocks that failed their check while locked                            */
    int synced;
} fmd_rds_info;
int fmd_rds_decoder_new(uint32_t rate_num, uint32_t rate_den, fmd_rds_decoder **out);
void fmd_rds_decoder_free(fmd_rds_decoder *d);
int fmd_rds_decoder_reset(fmd_rds_decoder *d);
/* n (ur, ui) pairs in; up to `cap` groups out, oldest first.  Groups that do not fit stay queued and come with the next push
 * (n may be 0, iq then NULL). */
int fmd_rds_decoder_push(fmd_rds_decoder *d, const int16_t *iq, size_t n, fmd_rds_group *groups, size_t cap, size_t *n_groups);
int fmd_rds_decoder_info(const fmd_rds_decoder *d, fmd_rds_info *info);

/* ---- FM receiver bank: stereo audio and the RDS baseband out of one multiplex pass ---------------------------- */
/* NEW SURFACE (the reference has none).  A stereo station bank and an RDS bank over the same stations in one handle: the multiplex
 * pass (front end, discriminator, pilot block sums) runs once per call and both second stages read its x[m].  No new arithmetic.
 * Per (stream, station): `audio` is bit for bit fmd_stereo_*'s for the same front-end arguments, capture_rate, block, pilot_min,
 * audio_taps, audio_decim and audio_shift; `rds` is bit for bit fmd_rds_*'s for the same front-end arguments and rds_taps,
 * rds_decim (its out_decim), rds_shift; the pilot report is theirs.  Neither output depends on how the stream is cut into calls.
 * Domain (else FMD_ERR_UNSUPPORTED, decided before a device is queried): the intersection of the two banks' -- capture_rate >=
 * 120000 decim (the RDS bank's floor), each stage's own limits on its stride, taps, sum |g| and shift (the exact-store rule on
 * rds_shift included), one block and one pilot_min.  nbytes % 8 != 0 -> FMD_ERR_BAD_LENGTH.  A call is accepted only if it completes
 * at least one output of EACH stage; otherwise FMD_ERR_TOO_SHORT, and nothing changes (send the bytes again with the next ones).
 * Stream lifetime and completion points: as fmd_channelizer_* (fmd_receiver_check). */
typedef struct fmd_receiver fmd_receiver;
typedef struct fmd_receiver_config {
    uint32_t capture_rate;   /* Hz: sets the pilot step inc_p                                         */
    uint32_t block;          /* P: pilot block length in MPX samples                                  */
    uint32_t pilot_min;      /* presence threshold, in discriminator units                            */
    uint32_t audio_decim;    /* the audio stage's R                                                   */
    uint32_t audio_shift;
    uint32_t rds_decim;      /* the RDS stage's R                                                     */
    uint32_t rds_shift;
} fmd_receiver_config;
int fmd_receiver_new(const int16_t *taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t *phase_inc,
                     uint32_t n_stations, const int16_t *audio_taps, uint32_t n_audio_taps, const int16_t *rds_taps,
                     uint32_t n_rds_taps, const fmd_receiver_config *cfg, const fmd_device_config *dev, fmd_receiver **out);
void fmd_receiver_free(fmd_receiver *s);
int fmd_receiver_reset(fmd_receiver *s);
/* HOST buffers: audio [n_streams][n_stations][audio_cap][2] (L, R), rds [n_streams][n_stations][rds_cap][2] (ur, ui); the
 * capacities are fmd_stereo_out_cap(decim, audio_decim, nbytes) and fmd_rds_out_cap(decim, rds_decim, nbytes) at least.
 * *n_audio, *n_rds = outputs per (stream, station) of each (the same for all). */
int fmd_receiver_run_batch(fmd_receiver *s, const uint8_t *iq, size_t nbytes, int16_t *audio, size_t audio_cap, size_t *n_audio,
                           int16_t *rds, size_t rds_cap, size_t *n_rds);
/* DEVICE buffers (d_iq, d_audio and d_rds 4-byte aligned), enqueued on `stream` without synchronising; counts as above. */
int fmd_receiver_run_device(fmd_receiver *s, const void *d_iq, size_t nbytes, void *d_audio, size_t audio_cap, size_t *n_audio,
                            void *d_rds, size_t rds_cap, size_t *n_rds, void *stream);
int fmd_receiver_check(fmd_receiver *s);
/* Audio samples and RDS baseband samples per (stream, station) produced since creation or the last reset. */
int fmd_receiver_outputs(const fmd_receiver *s, uint64_t *audio, uint64_t *rds);
/* The last completed block's pilot, with the semantics of fmd_stereo_pilot.  Synchronises first. */
int fmd_receiver_pilot(fmd_receiver *s, uint32_t stream, uint32_t station, int *present, uint32_t *level);
/* Name of pass 0 (the stereo bank's multiplex pass) or 1 (both second stages in one launch), as `rocprofv3 --kernel-trace` prints
 * it. */
int fmd_receiver_kernel_name(const fmd_receiver *s, uint32_t pass, char *name, size_t cap);

/* ---- narrow-band bank: AM, NFM, SSB and IQ channels with squelch --------------------------------------------- */
/* NEW SURFACE (rtl_fm's -M fm / am / usb / lsb / raw with a squelch, in the rtl-sdr ecosystem; the reference has none).  This is
 * the project's own operator, not the reference's chain: the channelizer's y, a second, COMPLEX decimating FIR that reaches
 * channels narrower than capture_rate / 64, one of four detectors and a block-wise squelch.  In IQ mode it is a two-stage
 * channelizer with total decimation up to 64 x 32.  Definition (integers only; tests/narrow_ref.py), per (stream, station k):
 *   y[m]    the channelizer's output (above), m counted from creation or reset
 *   v[n]    = sum_{t < Ta} (gr[t] + j gi[t]) y[R n + t]                                                  (exact in i32)
 *   u[n]    = (vr >> chan_shift) + j (vi >> chan_shift)                          arithmetic shifts (floor), per component
 *   a[n]    = isqrt(ur^2 + ui^2)                                                 floor integer square root, exact
 *   block j = the audio samples n with floor(n / P) = j;  E_j = sum (ur^2 + ui^2),  A_j = sum a[n]          (exact, i64)
 *   open_j  = squelch == 0 || E_j >= squelch^2 P,  open_{-1} = (squelch == 0);   dc_j = A_j >> log2(P),  dc_{-1} = 0
 *   w[n]    by mode:  FMD_NARROW_IQ   the pair (ur, ui)
 *                     FMD_NARROW_FM   (i16) polar_discriminant_fast(u[n], u[n-1])   (simple_fm.rs:377-405; u[-1] = 0; u[n-1]
 *                                     carries across calls, muted or not)
 *                     FMD_NARROW_AM   a[n] - dc_{j-1},  j = floor(n / P)
 *                     FMD_NARROW_SSB  ur                                            (the complex taps choose the sideband)
 *   out[n]  = 0 (both halves in IQ mode) if !open_{j-1};  (ur, ui) as int16 in IQ mode (gain is not applied);
 *             sat16((w[n] gain) >> 8) otherwise
 * Audio sample n comes with the call in which y[R n + Ta - 1] arrives; blocks are counted from reset, so the output does not
 * depend on how the stream is cut into calls.  The PREVIOUS block's estimates are used: every stage is causal and non-recursive.
 * out is [n_streams][n_stations][out_cap][width] int16, width = fmd_narrow_out_width(mode): 2 in IQ mode, 1 otherwise, at
 * capture_rate / (decim R).
 * Domain (else FMD_ERR_UNSUPPORTED, decided before a device is queried): the channelizer's filter domain, whose bound is
 * B_y = ceil(256 max_k sum_t (|Wr| + |Wi|) / 2^shift) <= 16384; 1 <= R <= 32; 1 <= Ta <= 256; chan_taps_im may be NULL (real
 * taps); every |gr|, |gi| <= 16383; G = sum_t (|gr| + |gi|) <= 65535; chan_shift <= 30; ceil(B_y G / 2^chan_shift) <= 16384; P a
 * power of two in [16, 4096]; squelch <= 23170; 1 <= gain <= 65535; mode <= 3.  Hence |v| <= B_y G < 2^30, |u| <= 16384,
 * |u|^2 <= 2^29, a <= 23170, E_j <= 2^41, |w gain| < 2^31.  nbytes % 8 != 0 -> FMD_ERR_BAD_LENGTH; a call that completes no
 * audio sample -> FMD_ERR_TOO_SHORT and changes nothing.  Stream lifetime and completion points: as fmd_channelizer_*. */
#define FMD_NARROW_IQ 0u
#define FMD_NARROW_FM 1u
#define FMD_NARROW_AM 2u
#define FMD_NARROW_SSB 3u
typedef struct fmd_narrow fmd_narrow;
typedef struct fmd_narrow_config {
    uint32_t mode;           /* FMD_NARROW_*                                                           */
    uint32_t chan_decim;     /* R                                                                      */
    uint32_t chan_shift;
    uint32_t block;          /* P: squelch / carrier-level block length in audio samples               */
    uint32_t squelch;        /* opens at an RMS |u| of this much (0: always open)                      */
    uint32_t gain;           /* Q8                                                                     */
} fmd_narrow_config;
int fmd_narrow_new(const int16_t *taps, uint32_t n_taps, uint32_t decim, uint32_t shift, const uint32_t *phase_inc,
                   uint32_t n_stations, const int16_t *chan_taps_re, const int16_t *chan_taps_im, uint32_t n_chan_taps,
                   const fmd_narrow_config *cfg, const fmd_device_config *dev, fmd_narrow **out);
void fmd_narrow_free(fmd_narrow *s);
int fmd_narrow_reset(fmd_narrow *s);
/* ceil(nbytes / (2 decim R)): audio samples one call of nbytes can complete per (stream, station), whatever the history;
 * 0 for decim 0 or R 0. */
size_t fmd_narrow_out_cap(uint32_t decim, uint32_t chan_decim, size_t nbytes);
/* int16 values per output sample: 2 in IQ mode, 1 otherwise. */
uint32_t fmd_narrow_out_width(uint32_t mode);
/* HOST buffers; *out_len = audio samples per (stream, station) (the same for all). */
int fmd_narrow_run_batch(fmd_narrow *s, const uint8_t *iq, size_t nbytes, int16_t *out, size_t out_cap, size_t *out_len);
/* DEVICE buffers (d_iq 4-byte aligned, d_out 4-byte aligned in IQ mode and 2-byte otherwise), enqueued on `stream` without
 * synchronising; *out_len as above. */
int fmd_narrow_run_device(fmd_narrow *s, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap, size_t *out_len,
                          void *stream);
int fmd_narrow_check(fmd_narrow *s);
/* Audio samples per (stream, station) produced since creation or the last reset. */
int fmd_narrow_outputs(const fmd_narrow *s, uint64_t *outputs);
/* The last completed block: *open = open_j, *rms = isqrt(E_j >> log2 P), the channel's RMS amplitude in units of u (0 and 0
 * before the first block completes).  Synchronises first. */
int fmd_narrow_level(fmd_narrow *s, uint32_t stream, uint32_t station, int *open, uint32_t *rms);
/* Name of pass 0 (front end) or 1 (channel FIR, detector, squelch), as `rocprofv3 --kernel-trace` prints it. */
int fmd_narrow_kernel_name(const fmd_narrow *s, uint32_t pass, char *name, size_t cap);

/* ---- power spectrum: where the stations are ------------------------------------------------------------------ */
/* NEW SURFACE (rtl_power's job in the rtl-sdr ecosystem; the reference has none).  The integrated power of N DFT bins of every
 * stream, to find the offsets a station bank is then tuned to.  A bin is a station-bank filter (the taps and the NCO table above)
 * whose decimation is the frame hop.  Definition (integers only; tests/spectrum_ref.py):
 *   c[n]      = (b[2n] - 127) + j (b[2n+1] - 127)                 raw read_sync bytes, NO rotate_90
 *   N         = n_bins in {16, 32, 64, 128, 256};  hop a multiple of 8, 8 <= hop <= N (frame f starts at byte 2 hop f)
 *   w[0..N)   = int16 window, |w| <= 2047;  inc_k = k 2^32 / N
 *   W[k][t]   = rnd(w[t] cosq(t inc_k)) + j rnd(-w[t] sinq(t inc_k))     (the station bank's taps: |W| <= 2047; one i8 digit
 *               when every |W| <= 127, two otherwise -- fmd_spectrum_tap_digits)
 *   F         = floor((nbytes / 2 - N) / hop) + 1 frames per call, from sample 0 of the call; trailing samples that do not fill
 *               a frame are ignored; NO state is carried between calls
 *   z[k][f]   = sum_{t < N} W[k][t] c[f hop + t]                    (exact: |z| < 2^31)
 *   p[k][f]   = (zr^2 + zi^2) >> shift                              (in 64 bits: zr^2 + zi^2 < 2^63; 0 <= shift <= 63)
 *   P[s][k]   = sum_f p[k][f]  as a u64 modulo 2^64, natural DFT order: bin k lies (k < N/2 ? k : k - N) capture_rate / N Hz
 *               from the centre (a tone at +f0 lands in bin f0 N / capture_rate: the sign convention of fmd_stations_phase_inc).
 * Domain errors are refused before a device is touched: nbytes % 8 != 0 -> FMD_ERR_BAD_LENGTH; fewer than one frame ->
 * FMD_ERR_TOO_SHORT and nothing is written; a bad n_bins, hop, window magnitude or shift > 63 -> FMD_ERR_UNSUPPORTED; NULL
 * pointers or zero streams -> FMD_ERR_INVALID_ARG.
 * Layouts: iq [n_streams][nbytes], power [n_streams][n_bins] u64; n_streams is dev->n_channels.  Stream lifetime and completion
 * points: as fmd_stations_* (fmd_spectrum_check). */
typedef struct fmd_spectrum fmd_spectrum;
/* Exact integer Hann window: w[n] = (amplitude (16384 - TAB[(n 1024 / N) & 1023]) + 16384) >> 15, 1 <= amplitude <= 2047
 * (amplitude <= 127 gives the one-digit form).  `window` holds n_bins entries. */
int fmd_spectrum_hann(uint32_t n_bins, uint32_t amplitude, int16_t *window);
/* inc_k = bin 2^32 / n_bins: the fmd_stations_new phase_inc that tunes a station bank to the centre of `bin`. */
int fmd_spectrum_bin_inc(uint32_t bin, uint32_t n_bins, uint32_t *inc);
/* F above; 0 for fewer than one frame or a bad n_bins / hop. */
size_t fmd_spectrum_frames(uint32_t n_bins, uint32_t hop, size_t nbytes);
int fmd_spectrum_new(const int16_t *window, uint32_t n_bins, uint32_t hop, uint32_t shift, const fmd_device_config *dev,
                     fmd_spectrum **out);
void fmd_spectrum_free(fmd_spectrum *s);
/* HOST buffers; power [n_streams][n_bins] is overwritten. */
int fmd_spectrum_power_batch(fmd_spectrum *s, const uint8_t *iq, size_t nbytes, uint64_t *power);
/* DEVICE buffers (d_iq 4-byte aligned, d_power 8-byte aligned), enqueued on `stream` without synchronising.  accumulate = 0
 * zeroes d_power on `stream` first; accumulate = 1 adds this call's power to it (integrating a long capture). */
int fmd_spectrum_power_device(fmd_spectrum *s, const void *d_iq, size_t nbytes, void *d_power, int accumulate, void *stream);
int fmd_spectrum_check(fmd_spectrum *s);
/* 1 or 2: the i8 digits per tap on the matrix cores. */
int fmd_spectrum_tap_digits(const fmd_spectrum *s);
/* Name of the kernel this handle launches, as `rocprofv3 --kernel-trace` prints it. */
int fmd_spectrum_kernel_name(const fmd_spectrum *s, char *name, size_t cap);

/* ---- uniform channelizer: every channel of a band plan in one pass --------------------------------------------- */
/* NEW SURFACE (the reference has none).  One prototype filter, longer than a frame step, applied to all N equally spaced channels
 * of every stream (or a selection of them): each channel's decimated complex baseband.  Definition (integers only;
 * tests/uniform_ref.py): the channelizer's steps, unchanged, with decim = hop and a fixed grid of phase steps:
 *   inc_k     = floor((k 2^33 / N + 1) / 2) mod 2^32                  channel k of N: centre (k < N/2 ? k : k - N) capture_rate / N Hz
 *                                                                     (for a power-of-two N: fmd_spectrum_bin_inc(k, N))
 *   c, TAB, cosq, sinq, W[k][t] = rnd(h[t] cosq(t inc_k)) + j rnd(-h[t] sinq(t inc_k))      exactly the station bank's
 *   z[k][m]   = sum_{t < n_taps} W[k][t] c[hop m + t]                 (exact in i32)
 *   y[k][m]   = (z * (cosq(psi) + j sinq(psi))) >> (14 + shift),  psi = m hop inc_k mod 2^32 (floor, per component, in i64)
 * Output m comes with the call in which sample hop m + n_taps - 1 arrives; m and the filter history carry across calls.
 * Domain (else FMD_ERR_UNSUPPORTED, decided before a device is queried): 2 <= n_channels <= 256, any integer; hop a multiple of
 * 8 in 8 ... 256, not tied to n_channels (the caller chooses the oversampling); 1 <= n_taps <= 2048; |h| <= 2047; shift <= 24;
 * ceil(256 G / 2^shift) <= 16384 with G = max over the selected channels of sum_t (|Wr| + |Wi|), so |y| <= 16384 (and, G <= 2^23,
 * |z| < 2^31); n_streams <= 65535.  `channels` [n_selected]: strictly increasing, each < n_channels, 1 <= n_selected <=
 * n_channels -- only these rows are computed and stored; NULL means all n_channels (n_selected is then ignored).
 * Calls: nbytes % (2 hop) != 0 -> FMD_ERR_BAD_LENGTH (every power-of-two hop divides a 262144-byte read_sync buffer); a call that
 * completes no output -> FMD_ERR_TOO_SHORT and nothing changes, exactly as the channelizer.  With whole hops per call the carried
 * history is a constant hop (ceil(n_taps / hop) - 1) samples, and every frame start stays 16-byte aligned relative to d_iq.
 * Where both are defined (hop even and <= 64, n_taps <= 256, at most 32 selected channels) the handle returns exactly what
 * fmd_channelizer_* returns for decim = hop and phase_inc = inc_k, call by call.
 * Layouts: iq [n_streams][nbytes], out [n_streams][selected channel][out_cap][2] int16 (yr, yi); n_streams is dev->n_channels.
 * Stream lifetime and completion points: as fmd_channelizer_* (fmd_uniform_check). */
typedef struct fmd_uniform fmd_uniform;
/* inc_k above; FMD_ERR_UNSUPPORTED unless 2 <= n_channels <= 256 and channel < n_channels. */
int fmd_uniform_channel_inc(uint32_t channel, uint32_t n_channels, uint32_t *inc);
/* nbytes / (2 hop): bounds the outputs of every call of nbytes per (stream, channel); 0 for hop 0. */
size_t fmd_uniform_out_cap(uint32_t hop, size_t nbytes);
int fmd_uniform_new(const int16_t *taps, uint32_t n_taps, uint32_t n_channels, uint32_t hop, uint32_t shift,
                    const uint32_t *channels, uint32_t n_selected, const fmd_device_config *dev, fmd_uniform **out);
void fmd_uniform_free(fmd_uniform *u);
/* Position 0 and an all-zero history, after the device has finished. */
int fmd_uniform_reset(fmd_uniform *u);
/* HOST buffers; *out_len = outputs per (stream, channel) (the same for all). */
int fmd_uniform_run_batch(fmd_uniform *u, const uint8_t *iq, size_t nbytes, int16_t *out, size_t out_cap, size_t *out_len);
/* DEVICE buffers (d_iq and d_out 4-byte aligned, any out_cap), enqueued on `stream` without synchronising; *out_len as above. */
int fmd_uniform_run_device(fmd_uniform *u, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap, size_t *out_len,
                           void *stream);
int fmd_uniform_check(fmd_uniform *u);
/* Outputs per (stream, channel) produced since creation or the last reset: the next output's index m. */
int fmd_uniform_outputs(const fmd_uniform *u, uint64_t *outputs);
/* 1 or 2: the i8 digits per tap on the matrix cores (1 when every |W| of the selected channels <= 127). */
int fmd_uniform_tap_digits(const fmd_uniform *u);
/* Name of the kernel this handle launches, as `rocprofv3 --kernel-trace` prints it. */
int fmd_uniform_kernel_name(const fmd_uniform *u, char *name, size_t cap);

/* ---- band-plan bank: audio and squelch for every channel of a plan ---------------------------------------------- */
/* NEW SURFACE (the reference has none).  The uniform channelizer's y of every selected channel of a band plan, fed to the
 * narrow-band bank's second stage: a complex decimating FIR, one of four detectors and a block-wise squelch per channel, plus an
 * activity map of the whole plan.  Definition (integers only; tests/bandplan_ref.py), per stream and selected channel k -- the
 * composition of two definitions above, with no new arithmetic:
 *   y[k][m]   exactly the uniform channelizer's: the same prototype h, n_channels, hop, shift, `channels` selection, history and
 *             call rules
 *   v, u, a, E_j, A_j, open_j, dc_j, w, out   exactly the narrow-band bank's over that y: taps (gr + j gi) at stride R, chan_shift,
 *             blocks of P audio samples using the previous block's estimates, the modes FMD_NARROW_IQ / FM / AM / SSB, the Q8 gain,
 *             sat16, the squelch; cfg is the narrow-band bank's fmd_narrow_config, one for all channels
 * out is [n_streams][n_selected][out_cap][width] int16, width = fmd_narrow_out_width(mode), at capture_rate / (hop R).
 * Domain (else FMD_ERR_UNSUPPORTED, decided before a device is queried): the uniform channelizer's for stage one, whose bound is
 * B_y = ceil(256 G / 2^shift) <= 16384 over the selected channels; the narrow-band bank's for stage two with 1 <= R <= 8,
 * 1 <= Ta <= 64 and ceil(B_y sum(|gr| + |gi|) / 2^chan_shift) <= 16384.
 * Calls are whole hops: nbytes % (2 hop) != 0 -> FMD_ERR_BAD_LENGTH.  A call that completes no audio sample -> FMD_ERR_TOO_SHORT and
 * changes NOTHING -- neither the carried stage-one history nor any output count -- even when it would have completed stage-one
 * outputs.  The output does not depend on how the stream is cut into calls.  Stream lifetime and completion points: as
 * fmd_channelizer_* (fmd_bandplan_check). */
typedef struct fmd_bandplan fmd_bandplan;
int fmd_bandplan_new(const int16_t *taps, uint32_t n_taps, uint32_t n_channels, uint32_t hop, uint32_t shift,
                     const uint32_t *channels, uint32_t n_selected, const int16_t *chan_taps_re, const int16_t *chan_taps_im,
                     uint32_t n_chan_taps, const fmd_narrow_config *cfg, const fmd_device_config *dev, fmd_bandplan **out);
void fmd_bandplan_free(fmd_bandplan *b);
int fmd_bandplan_reset(fmd_bandplan *b);
/* ceil(nbytes / (2 hop R)): audio samples one call of nbytes can complete per (stream, channel), whatever the history; 0 for hop 0
 * or R 0. */
size_t fmd_bandplan_out_cap(uint32_t hop, uint32_t chan_decim, size_t nbytes);
/* HOST buffers; *out_len = audio samples per (stream, channel) (the same for all). */
int fmd_bandplan_run_batch(fmd_bandplan *b, const uint8_t *iq, size_t nbytes, int16_t *out, size_t out_cap, size_t *out_len);
/* DEVICE buffers (d_iq 4-byte aligned, d_out 4-byte aligned in IQ mode and 2-byte otherwise, any out_cap), enqueued on `stream`
 * without synchronising; *out_len as above. */
int fmd_bandplan_run_device(fmd_bandplan *b, const void *d_iq, size_t nbytes, void *d_out, size_t out_cap, size_t *out_len,
                            void *stream);
int fmd_bandplan_check(fmd_bandplan *b);
/* Audio samples per (stream, channel) produced since creation or the last reset. */
int fmd_bandplan_outputs(const fmd_bandplan *b, uint64_t *outputs);
/* The activity map, HOST arrays [n_streams][n_selected], every row in one copy: open = open_j and rms = isqrt(E_j >> log2 P) of the
 * last completed block (zeros before the first block completes).  Synchronises first. */
int fmd_bandplan_levels(fmd_bandplan *b, uint8_t *open, uint32_t *rms);
/* Name of pass 0 (the uniform channelizer's kernel) or 1 (channel FIR, detector, squelch), as `rocprofv3 --kernel-trace` prints
 * it. */
int fmd_bandplan_kernel_name(const fmd_bandplan *b, uint32_t pass, char *name, size_t cap);

/* ---- rational resampler: any bank's int16 output at a fixed rate ------------------------------------------------ */
/* NEW SURFACE (the reference has only the fractional boxcar of low_pass_real).  A polyphase L / M filter over the int16 rows a bank
 * leaves on the device; a row is one (stream, station) or (stream, channel), `width` int16 per sample: 1 for mono audio, 2 for
 * interleaved (L, R) or (I, Q).  Definition (integers only; tests/resample_ref.py), per row and component c < width:
 *   x[i][c]   int16 input, i >= 0 counted from creation or reset
 *   g[p][t]   int16 polyphase taps, p < L phases of T taps each, phase-major: taps[p T + t]
 *   q_n = n M,  i_n = floor(q_n / L),  p_n = q_n mod L                                        (u64)
 *   v[n][c]   = sum_{t < T} g[p_n][t] x[i_n + t][c]         (exact in i32: every phase has sum_t |g[p][t]| <= 32767)
 *   out[n][c] = sat16(v[n][c] >> shift)                     (arithmetic shift: floor)
 * Output n comes with the call in which x[i_n + T - 1] arrives: after N inputs per row, N >= T ? ceil((N - T + 1) L / M) : 0
 * outputs exist, the same for every row, and a call returns the new ones.  The handle carries max(0, N - i_next) <= T - 1 samples,
 * i_next = floor(outputs M / L); where M / L > T, i_next may lie beyond N and the next call skips inputs.  The output does not
 * depend on how the stream is cut into calls that each complete an output.  L = M = 1 is a plain FIR (g = [1]: the identity), L = 1
 * the banks' own rule for a FIR at stride M.
 * Domain (else FMD_ERR_UNSUPPORTED, decided before a device is queried): width 1 or 2; 1 <= L <= 1024 and 1 <= M <= 1024;
 * M <= 32 L; L <= 8 M; 1 <= T <= 256; L T <= 16384; shift <= 24; n_rows = dev->n_channels >= 1; every phase's sum |g| <= 32767.
 * n_in > in_cap or an out_cap below the call's outputs -> FMD_ERR_CAPACITY (nothing is written); a call that completes no output ->
 * FMD_ERR_TOO_SHORT and changes nothing (its samples are not taken).  Stream lifetime and completion points: as fmd_channelizer_*
 * (fmd_resample_check). */
typedef struct fmd_resample fmd_resample;
/* L / M = rate_out rate_in_den / rate_in_num (the input rate is rate_in_num / rate_in_den Hz), reduced by the gcd in u64.  Zero
 * rates, rate_in_den or rate_out of 2^32 and more, or a reduced ratio outside the domain -> FMD_ERR_UNSUPPORTED. */
int fmd_resample_ratio(uint64_t rate_in_num, uint64_t rate_in_den, uint64_t rate_out, uint32_t *L, uint32_t *M);
int fmd_resample_new(const int16_t *taps, uint32_t L, uint32_t M, uint32_t T, uint32_t shift, uint32_t width,
                     const fmd_device_config *dev, fmd_resample **out);
void fmd_resample_free(fmd_resample *r);
int fmd_resample_reset(fmd_resample *r);
/* ceil(n_in L / M) + 1: outputs per row one call of n_in samples can complete at most, whatever the history; 0 for L 0 or M 0. */
size_t fmd_resample_out_cap(uint32_t L, uint32_t M, size_t n_in);
/* HOST buffers: in [n_rows][in_cap][width], the first n_in samples of each row valid; out [n_rows][out_cap][width]; *n_out =
 * outputs per row (the same for all). */
int fmd_resample_run_batch(fmd_resample *r, const int16_t *in, size_t n_in, size_t in_cap, int16_t *out, size_t out_cap,
                           size_t *n_out);
/* DEVICE buffers, enqueued on `stream` without synchronising: d_in is a bank's d_out as it stands, with the bank's out_cap as
 * in_cap; pointers 4-byte aligned at width 2 and 2-byte aligned at width 1, any in_cap and out_cap. */
int fmd_resample_run_device(fmd_resample *r, const void *d_in, size_t n_in, size_t in_cap, void *d_out, size_t out_cap,
                            size_t *n_out, void *stream);
int fmd_resample_check(fmd_resample *r);
/* Samples taken and outputs produced per row since creation or the last reset. */
int fmd_resample_outputs(const fmd_resample *r, uint64_t *inputs, uint64_t *outputs);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_resample_kernel_name(const fmd_resample *r, char *name, size_t cap);

/* ---- automatic gain control: any bank's int16 output at a steady level, without clipping ------------------------ */
/* NEW SURFACE (the reference has no AGC).  A block-peak AGC with one block of look-ahead over the int16 rows a bank leaves on the
 * device -- the other half of the output chain bank -> AGC -> resampler; a row is one (stream, station) or (stream, channel),
 * `width` int16 per sample: 1 for mono audio, 2 for interleaved (L, R) or (I, Q) under one common gain.  With gain = 256 the narrow
 * and band-plan banks' w fits int16 in every mode, so their rows carry the detector's full precision.  Definition (integers only;
 * tests/agc_ref.py), per row, with P = block:
 *   x[i][c]    int16 input, i >= 0 counted from creation or reset, c < width
 *   m[i]       = max_c |x[i][c]|                                  0 ... 32768
 *   block j    = the samples i with floor(i / P) = j;   p_j = max m[i] over block j
 *   e_j        = max(p_j, p_{j+1})                                one block of look-ahead
 *   d_j        = min(gain_max, floor(target 1024 / e_j))          Q10, for e_j > 0
 *   state (G, h), starting at G = gain_max, h = 0; per block j in order:
 *       e_j == 0      : G, h unchanged          (a muted or silent block holds the gain)
 *       d_j <= G      : G = d_j,  h = hang      (attack: complete one block BEFORE the loud block, thanks to the look-ahead)
 *       h > 0         : h = h - 1               (hang)
 *       otherwise     : G = min(d_j, G + max(1, ((d_j - G) decay) >> 8))        (release)
 *   G_j        = G after block j;   G_{-1} := G_0
 *   g[i]       = G_{j-1} + (((G_j - G_{j-1}) (r + 1)) >> log2 P),   j = floor(i / P), r = i mod P    (arithmetic shift: floor)
 *   out[i][c]  = (x[i][c] g[i]) >> 10                             (arithmetic shift)
 * Bounds: |G_j - G_{j-1}| (r + 1) <= 2^18 2^12 = 2^30.  For e_j > 0, G_j <= d_j (attack sets it, hang keeps a smaller G, release
 * takes the minimum), so G_j <= target 1024 / p_j and, as e_{j-1} >= p_j, G_{j-1} <= target 1024 / p_j too (where e_j or e_{j-1}
 * is 0, p_j is 0 and block j is all zeros).  g[i] lies between the two ends of the ramp, hence |x g| <= 1024 target < 2^25 and
 * |out| <= target: the AGC never clips and needs no sat16, and everything is exact in i32.
 * Calls: output block j needs p_{j+1}.  After N inputs per row P max(0, floor(N / P) - 1) outputs exist, the same for every row,
 * and a call returns the new ones.  The handle carries the N - outputs samples not yet emitted (at most 2 P - 1) and (G, h) per
 * row.  A call that completes no block is accepted: FMD_OK, *n_out = 0, and its samples go into the history.  n_in == 0 is FMD_OK,
 * launches nothing and changes nothing.  n_in > in_cap or an out_cap below the call's outputs -> FMD_ERR_CAPACITY (nothing is
 * written or taken).  The output does not depend on how the stream is cut into calls.  The last P ... 2 P - 1 samples of a stream
 * never come out on their own: a caller who wants them appends 2 P zero samples.
 * Domain (else FMD_ERR_UNSUPPORTED, decided before a device is queried): width 1 or 2; block a power of two in [16, 4096];
 * 1 <= target <= 32767; 1 <= gain_max <= 262144 (256 x in Q10); hang <= 65535; 1 <= decay <= 256; n_rows = dev->n_channels >= 1.
 * Stream lifetime and completion points: as fmd_channelizer_* (fmd_agc_check). */
typedef struct fmd_agc fmd_agc;
typedef struct fmd_agc_config {
    uint32_t block;     /* P: samples per block                                        */
    uint32_t target;    /* the largest |out|                                           */
    uint32_t gain_max;  /* Q10: the gain of a quiet row                                */
    uint32_t hang;      /* blocks the gain is held after an attack                     */
    uint32_t decay;     /* release: the fraction decay / 256 of the gap, per block     */
} fmd_agc_config;
int fmd_agc_new(const fmd_agc_config *cfg, uint32_t width, const fmd_device_config *dev, fmd_agc **out);
void fmd_agc_free(fmd_agc *a);
int fmd_agc_reset(fmd_agc *a);
/* block ceil(n_in / block): outputs per row one call of n_in samples can complete at most, whatever the history; 0 for block 0. */
size_t fmd_agc_out_cap(uint32_t block, size_t n_in);
/* HOST buffers: in [n_rows][in_cap][width], the first n_in samples of each row valid; out [n_rows][out_cap][width]; *n_out =
 * outputs per row (the same for all). */
int fmd_agc_run_batch(fmd_agc *a, const int16_t *in, size_t n_in, size_t in_cap, int16_t *out, size_t out_cap, size_t *n_out);
/* DEVICE buffers, enqueued on `stream` without synchronising: d_in is a bank's d_out as it stands, with the bank's out_cap as
 * in_cap; pointers 4-byte aligned at width 2 and 2-byte aligned at width 1, any in_cap and out_cap. */
int fmd_agc_run_device(fmd_agc *a, const void *d_in, size_t n_in, size_t in_cap, void *d_out, size_t out_cap, size_t *n_out,
                       void *stream);
int fmd_agc_check(fmd_agc *a);
/* Samples taken and outputs produced per row since creation or the last reset. */
int fmd_agc_outputs(const fmd_agc *a, uint64_t *inputs, uint64_t *outputs);
/* (G, h) of `row` after the last emitted block; gain_max, 0 before any block.  Synchronises first. */
int fmd_agc_gain(fmd_agc *a, uint32_t row, uint32_t *gain, uint32_t *hang);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_agc_kernel_name(const fmd_agc *a, char *name, size_t cap);

/* ---- tone squelch: any bank's NFM rows gated by a sub-audible tone (CTCSS) --------------------------------------- */
/* NEW SURFACE (the reference has no tone decoder).  Every int16 row a bank leaves on the device is correlated, block by block,
 * against a table of up to 64 windowed reference tones, and gated by the tone that the blocks before decided on -- the first link of
 * the output chain bank -> tone squelch -> AGC -> resampler; a row is one (stream, channel), `width` int16 per sample: 1 for mono
 * audio, 2 for interleaved (L, R), whose mean is correlated and whose components share the gate.  Definition (integers only, exact;
 * tests/tonesq_ref.py), per row, with P = block and i the sample index since creation or reset:
 *   x[i][c]     int16 input, c < width
 *   m[i]        = x[i][0]                         (width 1)
 *               = (x[i][0] + x[i][1]) >> 1        (width 2; arithmetic shift)
 *   tab[f][r]   = (c_f[r], s_f[r])   int16 pairs, f < F tones, r < P, every |entry| <= 1023
 *   block j     = samples with floor(i / P) = j,  r = i mod P
 *   Re_f(j)     = sum_r c_f[r] m[jP + r]          Im_f(j) = sum_r s_f[r] m[jP + r]      (exact; |.| <= 2^38)
 *   A_f = Re_f >> 14,  B_f = Im_f >> 14           (arithmetic shift: floor)
 *   W_f         = A_f^2 + B_f^2                   (u64, < 2^50)
 *   f*          = the smallest f with W_f maximal
 *   rest        = max W_f over |f - f*| > guard   (0 if there is none)
 *   hit_j       = f*  if W_f* >= min_power and (W_f* >> dom_shift) >= rest,  else NONE
 * State per row (t, cand, cnt, h, s_prev, s_cur), starting at (NONE, NONE, 0, 0, 0, 0), stepped once per completed block j:
 *   hit != NONE:  if hit == cand: cnt = min(cnt + 1, 65535)   else: cand = hit, cnt = 1
 *   hit == NONE:  cand = NONE, cnt = 0
 *   then:         cnt >= confirm:  t = cand, h = hang
 *                 else if h > 0:   h = h - 1
 *                 else:            t = NONE
 *   s_j  = 256 if t != NONE and bit t of accept is set, else 0
 * With s_{-1} = s_{-2} = 0 the gate on block j uses the decisions up to block j - 1: causal, no look-ahead, no added latency:
 *   Q = ramp (a power of two <= P)
 *   g[i]      = s_{j-2} + (((s_{j-1} - s_{j-2}) (min(r, Q - 1) + 1)) >> log2 Q)
 *   out[i][c] = (x[i][c] g[i]) >> 8
 * An open gate passes x bit for bit, a closed gate writes zeros.
 * Why |entry| <= 1023: a run of 64 samples gives at most 64 * 32768 * 1023 = 2 145 386 496 < 2^31, so any grouping of at most 64
 * products sums exactly in i32 (v_dot2_i32_i16) before it goes to an i64 sum; the definition does not depend on the grouping.
 * Counts and state: every call returns n_out = n_in and fmd_tonesq_out_cap(n_in) = n_in; the handle carries no samples, only the
 * 2 F partial sums (i64) and the small state per row.  core.pos is the one counter; the rows layer's history is unused.
 * Cut independence: partial sums of exact integers are associative, so the output and every report are independent of how the
 * stream is cut into calls, calls of one sample and calls that span several block ends included.
 * Reset: all-zero state is "closed, nothing carried" (t and cand are stored as t + 1, cand + 1).
 * n_in == 0 is FMD_OK, launches nothing and changes nothing.  n_in > in_cap or out_cap < n_in -> FMD_ERR_CAPACITY (nothing is
 * written or taken).  d_out == d_in is allowed when out_cap == in_cap (the gate in place); any other overlap is the caller's error.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried): width 1 or 2; block a power of two in
 * [64, 8192]; 1 <= n_tones <= 64; n_tones * block <= 262144; every table entry in [-1023, 1023]; guard <= 63; dom_shift <= 32;
 * min_power >= 1 (a silent block is never a hit); 1 <= confirm <= 255; hang <= 65535; ramp a power of two in [1, block];
 * n_rows = dev->n_channels >= 1.  Stream lifetime and completion points: as fmd_channelizer_* (fmd_tonesq_check). */
typedef struct fmd_tonesq fmd_tonesq;
typedef struct fmd_tonesq_config {
    uint32_t block;      /* P: samples per decision block                                      */
    uint32_t guard;      /* tones next to f* that do not count as `rest`                       */
    uint32_t dom_shift;  /* f* must exceed the rest by 2^dom_shift                             */
    uint32_t confirm;    /* equal hits in a row that open                                      */
    uint32_t hang;       /* blocks the tone is held after the last confirmed one               */
    uint32_t ramp;       /* Q: samples over which the gate moves at the start of a block       */
    uint64_t min_power;  /* the least W_f* of a hit                                            */
    uint64_t accept;     /* bit f: tone f opens the gate                                       */
} fmd_tonesq_config;
/* table: [n_tones][block][2] int16, (c_f[r], s_f[r]). */
int fmd_tonesq_new(const fmd_tonesq_config *cfg, const int16_t *table, uint32_t n_tones, uint32_t width,
                   const fmd_device_config *dev, fmd_tonesq **out);
void fmd_tonesq_free(fmd_tonesq *t);
int fmd_tonesq_reset(fmd_tonesq *t);
/* n_in. */
size_t fmd_tonesq_out_cap(size_t n_in);
/* HOST buffers: in [n_rows][in_cap][width], the first n_in samples of each row valid; out [n_rows][out_cap][width]; *n_out = n_in. */
int fmd_tonesq_run_batch(fmd_tonesq *t, const int16_t *in, size_t n_in, size_t in_cap, int16_t *out, size_t out_cap, size_t *n_out);
/* DEVICE buffers, enqueued on `stream` without synchronising: d_in is a bank's d_out as it stands, with the bank's out_cap as
 * in_cap; pointers 4-byte aligned at width 2 and 2-byte aligned at width 1, any in_cap and out_cap. */
int fmd_tonesq_run_device(fmd_tonesq *t, const void *d_in, size_t n_in, size_t in_cap, void *d_out, size_t out_cap, size_t *n_out,
                          void *stream);
int fmd_tonesq_check(fmd_tonesq *t);
/* Samples taken and produced per row since creation or the last reset (the same number). */
int fmd_tonesq_outputs(const fmd_tonesq *t, uint64_t *inputs, uint64_t *outputs);
/* Host arrays [n_rows], after the last completed block: tone = t (-1: NONE), power = W_f* of that block, open = s_j != 0; -1 / 0 /
 * 0 before the first block.  Synchronises first. */
int fmd_tonesq_status(fmd_tonesq *t, int32_t *tone, uint64_t *power, uint8_t *open);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_tonesq_kernel_name(const fmd_tonesq *t, char *name, size_t cap);

/* ---- code squelch: any bank's NFM rows gated by a digital code (DCS) ------------------------------------------------ */
/* NEW SURFACE (the reference has no code decoder).  DCS, the digital-coded squelch, sends a 23-bit Golay word at 134.4 bit/s NRZ
 * under the voice band, continuously.  Every int16 row a bank leaves on the device is searched for one of up to 128 such words and
 * gated by the code that the blocks before decided on -- beside the tone squelch at the head of the output chain bank -> squelch ->
 * AGC -> resampler; a row is one (stream, channel), `width` int16 per sample: 1 for mono audio, 2 for interleaved (L, R), whose
 * mean is searched and whose components share the gate.  There is no clock recovery: every decimated sample k forms a word from
 * samples one bit apart back in time and compares it un-rotated; the code repeats, so every alignment comes by once per word
 * period (171 ms), and all k are independent.  Definition (integers only, exact; tests/dcs_ref.py), per row, with i the sample
 * index since creation or reset; everything at a negative index is 0:
 *   x[i][c]     int16 input, c < width
 *   m[i]        = x[i][0]                         (width 1)
 *               = (x[i][0] + x[i][1]) >> 1        (width 2; arithmetic shift)
 *   box         b[k]    = (sum_{r<B} m[k B + r]) >> log2 B                     B = box, a power of two; b is int16 by construction
 *   low-pass    soft[k] = sat16((sum_{t<T} lp[t] b[k - (T-1) + t]) >> lshift)  T = n_taps, |lp[t]| <= 1023; the sum is exact in
 *                                                                              i32: 64 * 32768 * 1023 < 2^31 (as the tone squelch)
 *   word        bit j of w[k] = 1 iff 23 soft[k - tap[j]] > sum_{j'<23} soft[k - tap[j']]
 *               (tap[0] = 0, non-decreasing, tap[22] <= 511.  The threshold is the mean of the 23 samples: a mistuned channel's
 *               DC does not move the slicer, and no high-pass is needed.)
 *   match       d_f = popcount(w[k] ^ u_f) over the table u_f, f < F <= 128;  f(k) = the smallest f with d_f minimal;
 *               k is a hit on f(k) if that d_f <= tol
 *   block j     = samples [j P, (j+1) P), P = block; its k are j P / B <= k < (j+1) P / B
 *               hits_f = the block's hits on f;  f* = the smallest f with hits_f maximal
 *               hit_j  = f*  if hits_f* >= min_hits,  else NONE
 * State per row and gate: exactly the tone squelch's.  (t, cand, cnt, h, s_prev, s_cur) from (NONE, NONE, 0, 0, 0, 0), stepped once
 * per completed block j:
 *   hit != NONE:  if hit == cand: cnt = min(cnt + 1, 65535)   else: cand = hit, cnt = 1
 *   hit == NONE:  cand = NONE, cnt = 0
 *   then:         cnt >= confirm:  t = cand, h = hang
 *                 else if h > 0:   h = h - 1
 *                 else:            t = NONE
 *   s_j  = 256 if t != NONE and bit (t & 63) of accept[t >> 6] is set, else 0
 * With s_{-1} = s_{-2} = 0, r = i mod P and Q = ramp (a power of two <= P):
 *   g[i]      = s_{j-2} + (((s_{j-1} - s_{j-2}) (min(r, Q - 1) + 1)) >> log2 Q)
 *   out[i][c] = (x[i][c] g[i]) >> 8
 * An open gate passes x bit for bit, a closed gate writes zeros.
 * Table bit order: bit j of u_f is compared with the sample tap[j] back, so bit 0 is the newest bit.  A DCS word c (bit 0 sent
 * first) is therefore stored reversed: table bit j = bit 22 - j of c (fm::dcs_word, dcs_word of the Python package).
 * Polarity: a discriminator of the other sign complements every word.  The complement of each of the 104 standard words is a
 * rotation of another of the 104, so a table of all 104 still reports such a station, under its partner's index.
 * Counts and state: every call returns n_out = n_in and fmd_dcs_out_cap(n_in) = n_in.  Per row the handle carries the open box's
 * partial sum, the last T - 1 b, the last tap[22] soft, the F hit counters of the open block and eight int32 of state.  core.pos
 * is the one counter; the rows layer's history is unused.
 * Cut independence: everything carried is an exact integer, so the output and every report are independent of how the stream is
 * cut into calls, calls of one sample and calls that span several block ends included.
 * Reset: all-zero state is "closed, nothing carried" (t and cand are stored as t + 1, cand + 1).
 * n_in == 0 is FMD_OK, launches nothing and changes nothing.  n_in > in_cap or out_cap < n_in -> FMD_ERR_CAPACITY (nothing is
 * written or taken).  d_out == d_in is allowed when out_cap == in_cap (the gate in place); any other overlap is the caller's error.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried): width 1 or 2; block a multiple of 64 in
 * [64, 32768]; box a power of two in [1, 64]; 1 <= n_taps <= 64; every lp entry in [-1023, 1023]; lshift <= 31; tap[0] = 0, tap
 * non-decreasing, tap[22] <= 511; 1 <= n_words <= 128; every word below 2^23; tol <= 23; min_hits >= 1; 1 <= confirm <= 255;
 * hang <= 65535; ramp a power of two in [1, block]; n_rows = dev->n_channels >= 1.  Stream lifetime and completion points: as
 * fmd_channelizer_* (fmd_dcs_check). */
typedef struct fmd_dcs fmd_dcs;
typedef struct fmd_dcs_config {
    uint32_t block;      /* P: samples per decision block                                      */
    uint32_t box;        /* B: samples per decimated sample                                    */
    uint32_t n_taps;     /* T: taps of the low-pass                                            */
    int16_t lp[64];      /* the low-pass, lp[T - 1] on the newest b; entries behind T unused   */
    uint32_t lshift;     /* the low-pass sum's shift                                           */
    uint32_t tap[23];    /* decimated samples from the newest bit back to bit j                */
    uint32_t tol;        /* bit errors a matching word may have                                */
    uint32_t min_hits;   /* the least hits_f* of a block that is a hit                         */
    uint32_t confirm;    /* equal hits in a row that open                                      */
    uint32_t hang;       /* blocks the code is held after the last confirmed one               */
    uint32_t ramp;       /* Q: samples over which the gate moves at the start of a block       */
    uint64_t accept[2];  /* bit f & 63 of accept[f >> 6]: word f opens the gate                */
} fmd_dcs_config;
/* words: [n_words] table words u_f, 23 bits each. */
int fmd_dcs_new(const fmd_dcs_config *cfg, const uint32_t *words, uint32_t n_words, uint32_t width,
                const fmd_device_config *dev, fmd_dcs **out);
void fmd_dcs_free(fmd_dcs *d);
int fmd_dcs_reset(fmd_dcs *d);
/* n_in. */
size_t fmd_dcs_out_cap(size_t n_in);
/* HOST buffers: in [n_rows][in_cap][width], the first n_in samples of each row valid; out [n_rows][out_cap][width]; *n_out = n_in. */
int fmd_dcs_run_batch(fmd_dcs *d, const int16_t *in, size_t n_in, size_t in_cap, int16_t *out, size_t out_cap, size_t *n_out);
/* DEVICE buffers, enqueued on `stream` without synchronising: d_in is a bank's d_out as it stands, with the bank's out_cap as
 * in_cap; pointers 4-byte aligned at width 2 and 2-byte aligned at width 1, any in_cap and out_cap. */
int fmd_dcs_run_device(fmd_dcs *d, const void *d_in, size_t n_in, size_t in_cap, void *d_out, size_t out_cap, size_t *n_out,
                       void *stream);
int fmd_dcs_check(fmd_dcs *d);
/* Samples taken and produced per row since creation or the last reset (the same number). */
int fmd_dcs_outputs(const fmd_dcs *d, uint64_t *inputs, uint64_t *outputs);
/* Host arrays [n_rows], after the last completed block: code = t (-1: NONE), hits = hits_f* of that block, open = s_j != 0; -1 / 0 /
 * 0 before the first block.  Synchronises first. */
int fmd_dcs_status(fmd_dcs *d, int32_t *code, uint32_t *hits, uint8_t *open);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_dcs_kernel_name(const fmd_dcs *d, char *name, size_t cap);

/* ---- packet demodulator: AX.25 frames (APRS) out of any bank's NFM rows --------------------------------------------- */
/* NEW SURFACE (the reference has no data decoder).  1200 baud AFSK packet in two halves, as fmd_rds_* and fmd_rds_decoder_* are for
 * RDS: fmd_afsk_* on the GPU turns every mono int16 row a bank leaves on the device into signed soft decisions, a few per bit;
 * fmd_ax25_decoder_* on the host, one per row, turns them into frames.
 *
 * fmd_afsk_*: the tone-pair demodulator, a row processor like the resampler; a row is one (stream, channel), width 1 only (the NFM
 * rows are mono; width 2 is FMD_ERR_UNSUPPORTED).  Definition (integers only, exact; tests/afsk_ref.py), per row:
 *   x[i]        int16 input, i counted from creation or reset
 *   tab[q][t]   int16, q < 4: mark-cos, mark-sin, space-cos, space-sin; t < T; every |entry| <= 1023
 *   i_n         = n D
 *   S_q[n]      = sum_{t < T} tab[q][t] x[i_n + t]     (exact in i32: 64 * 32768 * 1023 = 2 145 386 496 < 2^31, hence T <= 64)
 *   A_q         = S_q >> pre_shift                     (arithmetic shift: floor)
 *   E_m = A_0^2 + A_1^2,  E_s = A_2^2 + A_3^2          (i64; each below 2^63 even at pre_shift 0)
 *   out[n]      = sat16((E_m - E_s) >> out_shift)      (arithmetic shift; positive: mark)
 * Counting (the resampler's rule at L = 1, M = D): after N inputs, N >= T ? ceil((N - T + 1) / D) : 0 outputs exist; output n comes
 * with the call in which x[i_n + T - 1] arrives; the handle carries at most T - 1 samples.  fmd_afsk_out_cap(D, n_in) = ceil(n_in / D)
 * + 1 bounds a call's outputs.  A call that completes no output returns FMD_ERR_TOO_SHORT and takes nothing (hand the same samples
 * over again, with more behind them).  n_in > in_cap, or out_cap below the call's outputs -> FMD_ERR_CAPACITY, nothing is written or
 * taken.  The output does not depend on how the stream is cut into calls.  core.pos is the only counter: reset forgets the carried
 * samples, output 0 follows.
 * Levels: the designers (afsk_table in Python, fm::afsk_table in csrc/demod.hpp) give rectangular windows one bit long, pre_shift 8
 * and the smallest out_shift at which a full window of either tone at amplitude 1024 stays inside int16.  Louder input saturates at
 * +-32767 / -32768; that is harmless, because the decoder reads only signs and where they change.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried): width 1; 2 <= T <= 64; 1 <= D <= min(T, 32);
 * pre_shift <= 16; out_shift <= 48; every table entry in [-1023, 1023]; n_rows = dev->n_channels >= 1.  Stream lifetime and
 * completion points: as fmd_channelizer_* (fmd_afsk_check). */
typedef struct fmd_afsk fmd_afsk;
/* table: [4][T] int16. */
int fmd_afsk_new(const int16_t *table, uint32_t T, uint32_t D, uint32_t pre_shift, uint32_t out_shift, uint32_t width,
                 const fmd_device_config *dev, fmd_afsk **out);
void fmd_afsk_free(fmd_afsk *a);
int fmd_afsk_reset(fmd_afsk *a);
/* ceil(n_in / D) + 1; 0 when D is 0. */
size_t fmd_afsk_out_cap(uint32_t D, size_t n_in);
/* HOST buffers: in [n_rows][in_cap], the first n_in samples of each row valid; out [n_rows][out_cap]; *n_out outputs per row. */
int fmd_afsk_run_batch(fmd_afsk *a, const int16_t *in, size_t n_in, size_t in_cap, int16_t *out, size_t out_cap, size_t *n_out);
/* DEVICE buffers, enqueued on `stream` without synchronising: d_in is a bank's d_out as it stands, with the bank's out_cap as
 * in_cap; pointers 2-byte aligned, any in_cap and out_cap. */
int fmd_afsk_run_device(fmd_afsk *a, const void *d_in, size_t n_in, size_t in_cap, void *d_out, size_t out_cap, size_t *n_out,
                        void *stream);
int fmd_afsk_check(fmd_afsk *a);
/* Samples taken and soft decisions produced per row since creation or the last reset. */
int fmd_afsk_outputs(const fmd_afsk *a, uint64_t *inputs, uint64_t *outputs);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_afsk_kernel_name(const fmd_afsk *a, char *name, size_t cap);

/* fmd_ax25_decoder_*: the frame decoder of one row, on the host, no GPU.  Definition (integers only; tests/ax25_ref.py; the result
 * does not depend on how the samples are cut into pushes), with mod = rate_num and step = baud * rate_den (u64), the soft decisions
 * arriving at rate_num / rate_den per second (the audio rate over D):
 *   clock   ph = 0 at the start.  Per soft sample v: cur = (v >= 0); if cur differs from the sample before (1 at the start):
 *           ph -= (ph - mod / 2) >> 2 (arithmetic shift of the signed difference); then ph += step; when ph >= mod: ph -= mod and a
 *           bit is taken.
 *   NRZI    bit = (cur == the level at the previous take) (1 at the start).
 *   HDLC    per bit, in this order: the bit enters an 8-bit shift register from the top; the register equal to 0x7E is a flag, which
 *           closes the open frame and opens the next; else a 1 counts, and seven 1s in a row abort the open frame and close the
 *           receiver until the next flag; a 0 after exactly five 1s is dropped; every other bit goes to the open frame, LSB first.
 *   closing the flag's first seven bits, which went in, are removed.  No bits left: nothing (flags back to back).  A frame has whole
 *           bytes, 17 <= bytes <= 514 with its FCS, and the CRC-16/X.25 (reflected 0x1021, init and final xor 0xFFFF; "123456789"
 *           -> 0x906E) of all but the last two bytes equal to those two, low byte first.  What fails any of it is counted in
 *           bad_fcs and not delivered.
 * Every buffer is fixed and every write bounded: a frame's bits behind 514 bytes are counted, not stored; frames that do not fit
 * `frames` wait in a ring of 64, whose oldest gives way when a caller lets it fill.
 * Domain: 4 <= (rate_num / rate_den) / baud <= 64, else FMD_ERR_UNSUPPORTED ("need 4 <= rate / baud <= 64").
 * The same decoder for every row of a bank at once, on the device: fmd_hdlc_* below. */
typedef struct fmd_ax25_decoder fmd_ax25_decoder;
typedef struct fmd_ax25_frame {
    uint8_t data[512];       /* address, control, PID and information fields; the FCS is checked and left out */
    uint32_t len;
    uint64_t end_sample;     /* index, since creation or reset, of the soft sample that took the closing flag's last bit */
} fmd_ax25_frame;
typedef struct fmd_ax25_info {
    uint64_t frames_ok;      /* frames that passed, delivered or waiting                               */
    uint64_t bad_fcs;        /* bits between two flags that were not a frame (length, whole bytes, FCS) */
    uint64_t aborts;         /* open frames ended by seven 1s                                           */
    int in_frame;            /* a flag was seen and no abort since                                      */
} fmd_ax25_info;
int fmd_ax25_decoder_new(uint32_t rate_num, uint32_t rate_den, uint32_t baud, fmd_ax25_decoder **out);
void fmd_ax25_decoder_free(fmd_ax25_decoder *d);
int fmd_ax25_decoder_reset(fmd_ax25_decoder *d);
/* n soft decisions in; up to `cap` frames out, oldest first.  Frames that do not fit stay queued and come with the next push
 * (n may be 0, soft then NULL). */
int fmd_ax25_decoder_push(fmd_ax25_decoder *d, const int16_t *soft, size_t n, fmd_ax25_frame *frames, size_t cap, size_t *n_frames);
int fmd_ax25_decoder_info(const fmd_ax25_decoder *d, fmd_ax25_info *info);

/* fmd_hdlc_*: the frame bank, the same decoder for every row ON THE DEVICE: a seventh row processor, which takes fmd_afsk's d_out as
 * it stands and returns only the frames.  There is no new arithmetic.  For any number of rows and any cutting of the stream into
 * calls, row r behaves as an fmd_ax25_decoder(rate_num, rate_den, baud) of its own would that is pushed exactly row r's n_in samples
 * of each call, with room for every frame (tests/hdlc_ref.py).  A call leaves, per row:
 *   count   the frames that passed in this call, all of them;
 *   frames  the first min(count, frame_cap) of them as fmd_ax25_frame, in the order they closed: data is zero behind len, end_sample
 *           is counted from creation or reset as the host decoder counts it;
 *   info    the row's fmd_ax25_info after the call, cumulative since creation or reset.
 * A row with count > frame_cap has lost count - frame_cap frames for delivery; frames_ok counts them all the same.  How many a call
 * can complete: every sample takes at most one bit, and the clock's phase gains at most step + (mod / 2 + 3) / 4 per sample (the
 * step and the largest pull, from phase 0), so a call of n soft decisions takes at most
 *   B(n) = min(n, (mod - 1 + n (step + (mod / 2 + 3) / 4)) / mod)   bits (integer divisions)
 * and, the shortest frame being 144 line bits with one flag (17 bytes, no stuffed bit), completes at most (B(n) + 143) / 144 frames
 * per row -- the first may have all but its last bit in front of the call.  At rate / baud = 5 (mod = 5 step) that is about 0.325 n bits:
 * frame_cap 1 holds every frame of calls up to about 440 soft decisions, frame_cap 4 of calls up to about 1770.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried): the host decoder's rate test with its text
 * ("need 4 <= rate / baud <= 64"); 1 <= frame_cap <= 16 ("need 1 <= frame_cap <= 16"); n_rows = dev->n_channels >= 1 ("need n_rows >=
 * 1").  Calls: every call with 1 <= n_in <= 2^28 is taken (there is no FMD_ERR_TOO_SHORT); n_in == 0 launches nothing and leaves the
 * last call's counts and frames; n_in > in_cap is FMD_ERR_CAPACITY, with nothing taken.  Stream lifetime and completion points: as
 * fmd_channelizer_* (fmd_hdlc_check).  Reset: position 0, every row as new. */
typedef struct fmd_hdlc fmd_hdlc;
int fmd_hdlc_new(uint32_t rate_num, uint32_t rate_den, uint32_t baud, uint32_t frame_cap, const fmd_device_config *dev, fmd_hdlc **out);
void fmd_hdlc_free(fmd_hdlc *f);
int fmd_hdlc_reset(fmd_hdlc *f);
/* HOST rows: in [n_rows][in_cap], the first n_in samples of each row valid.  Returns when the call has completed. */
int fmd_hdlc_run_batch(fmd_hdlc *f, const int16_t *in, size_t n_in, size_t in_cap);
/* DEVICE rows, enqueued on `stream` without synchronising: d_in is fmd_afsk's d_out as it stands, with its out_cap as in_cap;
 * 2-byte aligned, any in_cap. */
int fmd_hdlc_run_device(fmd_hdlc *f, const void *d_in, size_t n_in, size_t in_cap, void *stream);
int fmd_hdlc_check(fmd_hdlc *f);
/* Samples taken per row since creation or the last reset. */
int fmd_hdlc_inputs(const fmd_hdlc *f, uint64_t *inputs);
/* The last call's results, behind a synchronisation.  counts: host array [n_rows] (all 0 before the first call and after reset).
 * frames: host array [n_sel][frame_cap] for the rows listed in `rows` only, zero behind each row's min(count, frame_cap); a row
 * index at or beyond n_rows is FMD_ERR_INVALID_ARG, with nothing written.  info: host array [n_rows]. */
int fmd_hdlc_counts(fmd_hdlc *f, uint32_t *counts);
int fmd_hdlc_frames(fmd_hdlc *f, const uint32_t *rows, size_t n_sel, fmd_ax25_frame *frames);
int fmd_hdlc_info(fmd_hdlc *f, fmd_ax25_info *info);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_hdlc_kernel_name(const fmd_hdlc *f, char *name, size_t cap);

/* ---- pager decoder: POCSAG messages out of any bank's NFM rows --------------------------------------------------------- */
/* NEW SURFACE (the reference has no data decoder).  POCSAG paging (direct 2-FSK at 512, 1200 or 2400 bit/s) in two halves:
 * fmd_fsk_* on the GPU turns every mono int16 row a bank leaves on the device into soft decisions, a few per bit, and reports
 * where a 32-bit sync word ends; fmd_pocsag_decoder_* on the host, one per row, reads the batches behind those reports.  There is no
 * clock recovery: every batch starts with the sync codeword 0x7CD215D8, the kernel tests every soft sample for it, and what it
 * finds gives the host the bit timing, the slicer level (which holds the DC a mistuned channel leaves on the discriminator) and
 * the polarity.
 *
 * fmd_fsk_*: a row processor; a row is one (stream, channel), width 1 only (width 2 is FMD_ERR_UNSUPPORTED).  Definition (integers
 * only, exact; tests/fsk_ref.py), per row; everything at a negative index is 0:
 *   x[i]      int16 input, i counted from creation or reset
 *   box       b[k]    = sum_{r < D} x[k D + r]                         (i32)
 *   soft      soft[k] = (sum_{t < W} b[k - t]) >> shift                (arithmetic shift; D W <= 2^shift, so soft is an int16 by
 *                                                                      construction and nothing saturates)
 *   out[k]    = soft[k]; output k comes with the call that brings x[k D + D - 1]
 *   word      thr[k]  = sum_{j < 32} soft[k - tap[j]]                  (tap[0] = 0, non-decreasing, tap[31] <= 255)
 *             bit j of w[k] = 1 iff 32 soft[k - tap[j]] > thr[k]       (equality: 0)
 *   match     d[k]    = popcount(w[k] ^ sync)
 *             C[k]    = sum_j (bit j of sync ? +1 : -1) soft[k - tap[j]]        (|C| <= 2^20)
 *   hit       normal   if d <= tol       and  C >= min_corr
 *             inverted if d >= 32 - tol  and -C >= min_corr            (tol <= 15, so never both)
 *   record    fmd_fsk_hit of every hit; k_rel = index of out[k] in THIS call
 * Bit order: POCSAG sends bit 31 first, so the newest bit is bit 0; table bit j is bit j of the codeword and sync is 0x7CD215D8
 * as written.
 * Counting: a call gives floor((pos + n_in) / D) - floor(pos / D) outputs; fmd_fsk_out_cap(D, n_in) = ceil(n_in / D) + 1 bounds
 * them.  A call that completes no box is taken (FMD_OK, 0 outputs, the partial sum carried).  n_in == 0 launches nothing and leaves
 * the last call's hits as they are.  n_in > in_cap, or out_cap below the call's outputs -> FMD_ERR_CAPACITY, nothing is written or
 * taken.
 * Per call and row: count, the number of hits, all of them; and the first min(count, hit_cap) records, in increasing k.  Both live
 * in device memory of the handle, are replaced by the next call that launches, and are read with fmd_fsk_hits.
 * Carried per row: the open box's partial sum, the last W - 1 b, the last tap[31] soft.  All zeros is "nothing carried", which is
 * what reset leaves.  Everything carried is an exact integer, so outputs and records are independent of how the stream is cut
 * into calls, calls of one sample and calls that complete no box included.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried): width 1; 1 <= D <= 64; 1 <= W <= 16;
 * shift <= 10 and D W <= 2^shift; tap[0] = 0, tap non-decreasing, tap[31] <= 255; tol <= 15; 0 <= min_corr <= 2^20;
 * 1 <= hit_cap <= 64; n_rows = dev->n_channels >= 1.  Stream lifetime and completion points: as fmd_channelizer_*
 * (fmd_fsk_check).  The designers (fsk_design in Python, fm::fsk_design in csrc/demod.hpp): D = max(1, floor(rate / (5 baud) +
 * 0.5)), W = floor(rate / (baud D) + 0.5), shift = ceil(log2(D W)), tap[j] = floor(j rate / (baud D) + 0.5), sync 0x7CD215D8,
 * tol 2, min_corr 1024, hit_cap 16. */
typedef struct fmd_fsk fmd_fsk;
typedef struct fmd_fsk_config {
    uint32_t D;          /* samples per box: the decimation                        */
    uint32_t W;          /* boxes per soft decision: D W samples are about one bit */
    uint32_t shift;      /* the soft decision's shift                              */
    uint32_t tap[32];    /* soft samples from the newest bit back to bit j         */
    uint32_t sync;       /* the word searched for                                  */
    uint32_t tol;        /* bit errors a hit may have                              */
    int32_t min_corr;    /* the least |C| of a hit                                 */
    uint32_t hit_cap;    /* records kept per row and call                          */
} fmd_fsk_config;
typedef struct fmd_fsk_hit {
    uint32_t k_rel;      /* index of out[k] in the call that reported it           */
    uint32_t d;          /* bits that differ, | 1 << 31 for an inverted hit        */
    int32_t corr;        /* C                                                      */
    int32_t thr;         /* the sum of the 32 soft samples: slice 32 soft > thr    */
} fmd_fsk_hit;
int fmd_fsk_new(const fmd_fsk_config *cfg, uint32_t width, const fmd_device_config *dev, fmd_fsk **out);
void fmd_fsk_free(fmd_fsk *f);
int fmd_fsk_reset(fmd_fsk *f);
/* ceil(n_in / D) + 1; 0 when D is 0. */
size_t fmd_fsk_out_cap(uint32_t D, size_t n_in);
/* HOST buffers: in [n_rows][in_cap], the first n_in samples of each row valid; out [n_rows][out_cap]; *n_out outputs per row. */
int fmd_fsk_run_batch(fmd_fsk *f, const int16_t *in, size_t n_in, size_t in_cap, int16_t *out, size_t out_cap, size_t *n_out);
/* DEVICE buffers, enqueued on `stream` without synchronising: d_in is a bank's d_out as it stands, with the bank's out_cap as
 * in_cap; pointers 2-byte aligned, any in_cap and out_cap. */
int fmd_fsk_run_device(fmd_fsk *f, const void *d_in, size_t n_in, size_t in_cap, void *d_out, size_t out_cap, size_t *n_out,
                       void *stream);
int fmd_fsk_check(fmd_fsk *f);
/* Samples taken and soft decisions produced per row since creation or the last reset. */
int fmd_fsk_outputs(const fmd_fsk *f, uint64_t *inputs, uint64_t *outputs);
/* Host arrays of the last call that launched: counts [n_rows], hits [n_rows][hit_cap] (zeros behind a row's records).  Either may
 * be NULL.  Synchronises first. */
int fmd_fsk_hits(fmd_fsk *f, uint32_t *counts, fmd_fsk_hit *hits);
/* The same results where they lie, so that a later kernel (fmd_pager_run_device) takes them without a visit to the host: DEVICE
 * pointers to what the last call that launched wrote, *d_counts [n_rows] uint32 and *d_hits [n_rows][hit_cap] fmd_fsk_hit (16-byte
 * aligned; behind a row's min(count, hit_cap) records lies whatever an earlier call left).  Does not synchronise: the contents are
 * complete once the call that wrote them is.  Valid until the handle's next call that launches, its reset, or its free. */
int fmd_pager_fsk_hits(fmd_fsk *f, const void **d_counts, const void **d_hits);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_fsk_kernel_name(const fmd_fsk *f, char *name, size_t cap);

/* fmd_pocsag_decoder_*: the batch decoder of one row, on the host, no GPU.  Definition (integers only; tests/pocsag_ref.py; the
 * result does not depend on how the samples and records are cut into pushes), with mod = rate_num and step = baud * rate_den (u64),
 * the soft decisions arriving at rate_num / rate_den per second (the audio rate over D), r = (2 mod + step) / (2 step) soft samples
 * per bit, and a ring of the last 64 soft samples.  Sample and record indices count from creation or reset; a record belongs to the
 * sample k_rel of its push, records whose k_rel is not below n or not in increasing order are ignored.  Per sample, in this order:
 * the sample enters the ring; its records are taken; a search window that is due closes; the bits and the slot that are due are read.
 *   search  the first record opens a window anchored at its index k1; a later record with k <= k1 + r and strictly larger |corr|
 *           replaces the candidate; when sample k1 + r has arrived the decoder locks on the candidate: k0, thr, inverted.
 *   locked  bit n >= 1 is (32 soft[p(n)] > thr) xor inverted, p(n) = k0 + (2 n mod + step) / (2 step); word i = 0 ... 15 is bits
 *           32 i + 1 ... 32 i + 32, first bit highest.  Slot 16 is the next sync, and the records alone decide it: when sample
 *           p(544) + r / 2 has arrived, of the records with |k - p(544)| <= r / 2 and the lock's polarity the one with the largest
 *           |corr|, the first such, becomes the new (k0, thr) and the next batch follows; with none the lock is lost, the open
 *           message closes and the decoder searches again.  Other records are ignored while locked.
 *   word    the corrected word is the unique valid codeword within Hamming distance max_errors over all 32 bits; valid: bits 31..1
 *           divisible by x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1 (0x769) and even parity over all 32.  The minimum distance is 6,
 *           so it is unique for max_errors <= 2.  With none, bad_codewords counts and the open message closes.
 *           0x7A89C197 (idle) closes the open message.  Bit 31 = 0: an address word, closes the open message and opens one with
 *           address = ((cw >> 13) & 0x3FFFF) << 3 | (i >> 1), function = (cw >> 11) & 3.  Bit 31 = 1: a message word, appends
 *           (cw >> 11) & 0xFFFFF, highest bit first, to the open message (bits behind 2560 are counted, not stored); with no
 *           message open it counts in orphans.
 * A closed message is delivered.  Messages that do not fit `msgs` wait in a ring of 64, whose oldest gives way when it fills.
 * Domain: 2 <= (rate_num / rate_den) / baud <= 32 ("need 2 <= rate / baud <= 32") and max_errors <= 2 ("need max_errors <= 2"),
 * else FMD_ERR_UNSUPPORTED. */
typedef struct fmd_pocsag_decoder fmd_pocsag_decoder;
typedef struct fmd_pocsag_msg {
    uint32_t address;        /* 21 bits: 18 of the address word, 3 of its frame                          */
    uint32_t function;       /* 0 ... 3                                                                  */
    uint32_t n_bits;         /* message bits, 20 per message word; 0: a tone-only page                   */
    uint8_t bits[320];       /* the first 2560 of them, the first in bit 7 of bits[0]                    */
    uint32_t corrected;      /* bits corrected in the message's codewords                                */
    uint32_t inverted;       /* the lock's polarity                                                      */
    uint64_t end_sample;     /* index of the soft sample that gave the last bit of its last codeword     */
} fmd_pocsag_msg;
typedef struct fmd_pocsag_info {
    uint64_t messages;       /* messages closed, delivered or waiting                  */
    uint64_t batches;        /* sync words the decoder locked on or followed           */
    uint64_t bad_codewords;  /* words with no valid codeword within max_errors         */
    uint64_t orphans;        /* message words with no message open                     */
    int locked;              /* inside a batch or waiting for the next sync word       */
    int searching;           /* a record opened a search window that is not due yet    */
} fmd_pocsag_info;
int fmd_pocsag_decoder_new(uint32_t rate_num, uint32_t rate_den, uint32_t baud, uint32_t max_errors, fmd_pocsag_decoder **out);
void fmd_pocsag_decoder_free(fmd_pocsag_decoder *d);
int fmd_pocsag_decoder_reset(fmd_pocsag_decoder *d);
/* n soft decisions and this call's n_hits records of the row in (k_rel counted into soft); up to `cap` messages out, oldest first.
 * Messages that do not fit stay queued and come with the next push (n may be 0, soft then NULL: it drains). */
int fmd_pocsag_decoder_push(fmd_pocsag_decoder *d, const int16_t *soft, size_t n, const fmd_fsk_hit *hits, size_t n_hits,
                            fmd_pocsag_msg *msgs, size_t cap, size_t *n_msgs);
int fmd_pocsag_decoder_info(const fmd_pocsag_decoder *d, fmd_pocsag_info *info);
/* The corrected codeword of `word` within `max_errors` (<= 2) bit errors in *cw and the bits flipped in *n_fixed (either may be
 * NULL): FMD_OK, or FMD_ERR_BAD_STATE when there is none. */
int fmd_pocsag_correct(uint32_t word, uint32_t max_errors, uint32_t *cw, uint32_t *n_fixed);

/* fmd_pager_*: the page bank, the same decoder for every row ON THE DEVICE: an eighth row processor, which takes fmd_fsk's d_out and
 * its records as they stand and returns only the messages.  There is no new arithmetic.  For any number of rows and any cutting of
 * the stream into calls, row r behaves as an fmd_pocsag_decoder(rate_num, rate_den, baud, max_errors) of its own would that is pushed
 * exactly row r's n_in soft decisions of each call and the first min(count_r, hit_cap) records of that call, with room for every
 * message (tests/pager_ref.py); the host decoder's ring of 64 waiting messages has no counterpart here.  A call leaves, per row:
 *   count   the messages that closed in this call, all of them;
 *   msgs    the first min(count, msg_cap) of them as fmd_pocsag_msg, in the order they closed: bits is zero behind (min(n_bits,
 *           2560) + 7) / 8 bytes, end_sample is counted from creation or reset as the host decoder counts it;
 *   info    the row's fmd_pocsag_info after the call, cumulative since creation or reset, with locked and searching.
 * A row with count > msg_cap has lost count - msg_cap messages for delivery; `messages` counts them all the same.
 * How many a call can complete.  A bit read in a call lies at a sample of that call: p(n) <= the sample that makes it due.  Inside a
 * batch two bit positions are at least q = mod / step (integer division) apart, since p(n + 1) - p(n) >= floor(mod / step); an anchor
 * made at sample s, after a search or at slot 16, puts p(1) = k + r >= s, behind every bit read before it.  So the bits a call of n
 * samples reads lie at distinct samples at least q apart within each batch and in increasing order across batches: at most B =
 * ceil(n / q) of them.  A codeword completes at its 32nd bit and all but that bit may lie in front of the call: at most (B + 31) / 32
 * codewords, each of which closes at most one message.  The only other close is a lost lock, which takes a whole batch of 512 bits
 * since the anchor: one whose bits all lie in front of the call, and one more per 512 bits read in it.  Hence at most
 *   M(n) = (B + 31) / 32 + 1 + B / 512   messages per row and call (fmd_pager_max_messages; 0 outside the rate domain).
 * At rate / baud = 5 a call of 256 soft decisions gives 3, and msg_cap 16 holds every message of calls up to 2400.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried): the host decoder's tests in its order with its
 * texts ("need 2 <= rate / baud <= 32", "need max_errors <= 2"); 1 <= msg_cap <= 16 ("need 1 <= msg_cap <= 16"); n_rows =
 * dev->n_channels >= 1 ("need n_rows >= 1"); per call 1 <= hit_cap <= 64 ("need 1 <= hit_cap <= 64").  Calls: every call with 1 <=
 * n_in <= 2^28 is taken; n_in == 0 launches nothing and leaves the last call's counts and messages; n_in > in_cap is
 * FMD_ERR_CAPACITY, with nothing taken.  Records follow the host decoder's rule: one with k_rel >= n_in, or one that is not in
 * increasing order, is passed over and never used as an index; a count above hit_cap reads hit_cap records.  Stream lifetime and
 * completion points: as fmd_channelizer_* (fmd_pager_check).  Reset: position 0, every row as new. */
typedef struct fmd_pager fmd_pager;
int fmd_pager_new(uint32_t rate_num, uint32_t rate_den, uint32_t baud, uint32_t max_errors, uint32_t msg_cap,
                  const fmd_device_config *dev, fmd_pager **out);
void fmd_pager_free(fmd_pager *p);
int fmd_pager_reset(fmd_pager *p);
/* HOST arrays: soft [n_rows][in_cap], the first n_in of each row valid; counts [n_rows]; hits [n_rows][hit_cap].  Returns when the
 * call has completed. */
int fmd_pager_run_batch(fmd_pager *p, const int16_t *soft, size_t n_in, size_t in_cap, const uint32_t *counts, const fmd_fsk_hit *hits,
                        uint32_t hit_cap);
/* DEVICE arrays, enqueued on `stream` without synchronising: d_soft is fmd_fsk's d_out as it stands, with its out_cap as in_cap
 * (2-byte aligned, any in_cap); d_counts and d_hits are what the same fsk call wrote (fmd_pager_fsk_hits; 4- and 16-byte aligned). */
int fmd_pager_run_device(fmd_pager *p, const void *d_soft, size_t n_in, size_t in_cap, const void *d_counts, const void *d_hits,
                         uint32_t hit_cap, void *stream);
int fmd_pager_check(fmd_pager *p);
/* Samples taken per row since creation or the last reset. */
int fmd_pager_inputs(const fmd_pager *p, uint64_t *inputs);
/* The last call's results, behind a synchronisation.  counts: host array [n_rows] (all 0 before the first call and after reset).
 * msgs: host array [n_sel][msg_cap] for the rows listed in `rows` only, zero behind each row's min(count, msg_cap); a row index at
 * or beyond n_rows is FMD_ERR_INVALID_ARG, with nothing written.  info: host array [n_rows]. */
int fmd_pager_counts(fmd_pager *p, uint32_t *counts);
int fmd_pager_msgs(fmd_pager *p, const uint32_t *rows, size_t n_sel, fmd_pocsag_msg *msgs);
int fmd_pager_info(fmd_pager *p, fmd_pocsag_info *info);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_pager_kernel_name(const fmd_pager *p, char *name, size_t cap);
/* The kernel's correction table for `max_errors` (<= 2), 2048 flip masks: entry (s << 1 | parity) is the bits to flip in a word
 * whose bits 31 ... 1 leave the remainder s by 0x769 and whose 32 bits have that parity, 0xFFFFFFFF where no codeword lies within
 * max_errors bits.  Host only. */
int fmd_pager_table(uint32_t max_errors, uint32_t *table);
/* M(n) above; 0 where rate / baud < 2. */
size_t fmd_pager_max_messages(uint32_t rate_num, uint32_t rate_den, uint32_t baud, size_t n);

/* ---- Mode S bank: ADS-B messages (1090 MHz extended squitter) decoded on the device per stream ------------------------- */
/* NEW SURFACE: rtl_adsb's job at bank size.  Mode S is pulse-position modulation on the raw magnitude, so this handle sits behind
 * no discriminator: it takes the u8 IQ of many 2 Msample/s streams as read_sync delivers it and leaves each stream's messages.
 * Integers only; the results do not depend on how a stream is cut into calls.  Definition (tests/modes_ref.py), per stream, i
 * counting samples from creation or reset, everything at a negative index 0:
 *   m[i]   = ((2 b[2i] - 255)^2 + (2 b[2i+1] - 255)^2) >> 1        (the sum of two odd squares is 2 mod 8: the shift loses nothing;
 *                                                                    0 <= m <= 65025, a u16)
 *   a_j    = m[p + j], j < 240, for a position p >= 0
 *   S(p)   = a0 + a2 + a7 + a9                                      (the four 0.5 us preamble pulses at 0, 1.0, 3.5 and 4.5 us)
 *   pre(p) = a0 > a1 and a1 < a2 and a2 > a3 and a3 < a0 and a4 < a0 and a5 < a0 and a6 < a0 and a7 > a8 and a8 < a9 and a9 > a6
 *            and 6 a_j < S for j in {4, 5, 11, 12, 13, 14} and S >= min_power
 *   bit t  = 1 iff m[p + 16 + 2t] > m[p + 17 + 2t]                  (equality: 0; t = 0 is sent first and is the MSB of byte 0)
 *   DF     = bits 0 ... 4;  n = 112 if bit 0 is 1 (DF >= 16), else 56
 *   syn    = the remainder of bits 0 ... n-25 under the generator 0xFFF409, XOR bits n-24 ... n-1 (24 bits, MSB-first shift register,
 *            initial value 0) = XOR over the set bits t of T_n[t]; T_112[t] = x^(111 - t) mod the generator: T_112[0] = 0x3935EA,
 *            T_112[87] = 0xFFF409, T_112[88] = 0x800000, T_112[111] = 1; T_56[t] = T_112[t + 56]; all 112 entries are distinct
 *   accept   DF in {17, 18} and syn == 0
 *       or   DF == 11 and df11 and (syn & 0xFFFF80) == 0
 *       or   DF in {17, 18} and fix_errors and syn == T_112[t] for one t in 5 ... 111: bit t is flipped in the record and
 *            fixed_bit = t (the DF field is never touched).
 * Each accepted p gives one record, in increasing p; overlapping acceptances are not suppressed on the device.  Position p is
 * decided by the call that brings sample p + 239, for both message lengths: a call over the samples [pos, pos + n) decides
 * max(0, pos - 239) <= p < pos + n - 239, and k_rel = p - pos runs from -239 upward.  Carried per stream: the m of its last 240
 * samples and the cumulative counters; all zeros is what reset leaves.  A call shorter than 240 samples is taken and may decide
 * nothing; nbytes == 0 launches nothing and leaves the last call's results.  Per call and stream `count` is every acceptance and the
 * first min(count, msg_cap) records are kept, whatever the scheduling.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried): min_power <= 262144, fix_errors and df11 0 or 1,
 * 1 <= msg_cap <= 256, n_streams = dev->n_channels >= 1 (0: FMD_ERR_INVALID_ARG).  Calls: nbytes % 8 != 0 is FMD_ERR_BAD_LENGTH,
 * nbytes > cap_bytes FMD_ERR_CAPACITY, cap_bytes % 4 != 0 or a d_iq that is not 4-byte aligned FMD_ERR_INVALID_ARG.  Stream lifetime
 * and completion points: as fmd_channelizer_* (fmd_modes_check).  Out of scope: the address/parity-overlaid formats (DF 0, 4, 5, 16,
 * 20, 21), 2.4 Msample/s input, two-bit correction, suppression of overlapping acceptances and a flush of the last 239 samples. */
typedef struct fmd_modes fmd_modes;
typedef struct fmd_modes_config {
    uint32_t min_power;   /* 0 .. 262144 */
    uint32_t fix_errors;  /* 0 | 1 */
    uint32_t df11;        /* 0 | 1 */
    uint32_t msg_cap;     /* 1 .. 256 */
} fmd_modes_config;
typedef struct fmd_modes_msg {                                                  /* 32 bytes */
    int32_t  k_rel;
    uint32_t power;       /* S */
    uint8_t  n_bytes;     /* 7 | 14 */
    uint8_t  fixed_bit;   /* 0xFF: none */
    uint8_t  df;
    uint8_t  rsv;
    uint8_t  bytes[14];   /* after the fix; zeros behind 7 */
    uint8_t  pad[6];
} fmd_modes_msg;
/* per stream, cumulative since creation or reset: samples taken, positions that passed pre(p), acceptances, acceptances with a fix.
 * (Read by fmd_modes_info; C keeps functions and typedefs in one name space, so the struct goes by another name.) */
typedef struct fmd_modes_totals {
    uint64_t samples, candidates, messages, fixed;
} fmd_modes_totals;

int fmd_modes_new(const fmd_modes_config *cfg, const fmd_device_config *dev, fmd_modes **out);   /* n_streams = dev->n_channels */
void fmd_modes_free(fmd_modes *h);
int fmd_modes_reset(fmd_modes *h);
/* HOST array iq [n_streams][cap_bytes], the first nbytes of each stream valid.  Returns when the call has completed. */
int fmd_modes_run_batch(fmd_modes *h, const uint8_t *iq, size_t nbytes, size_t cap_bytes);
/* DEVICE array of the same form, enqueued on `stream` without synchronising. */
int fmd_modes_run_device(fmd_modes *h, const void *d_iq, size_t nbytes, size_t cap_bytes, void *stream);
int fmd_modes_check(fmd_modes *h);
/* The last call's results, behind a synchronisation.  counts: host array [n_streams] (all 0 before the first call and after reset).
 * msgs: host array [n_sel][msg_cap] for the streams listed in `streams` only, in the order listed, zero behind each one's
 * min(count, msg_cap); an index at or beyond n_streams is FMD_ERR_INVALID_ARG, with nothing written.  info: host array [n_streams]. */
int fmd_modes_counts(fmd_modes *h, uint32_t *counts);
int fmd_modes_msgs(fmd_modes *h, const uint32_t *streams, size_t n_sel, fmd_modes_msg *msgs);
int fmd_modes_info(fmd_modes *h, fmd_modes_totals *info);
/* Name of the kernel of pass 0 (the tiles: preamble test, decode, syndrome) or 1 (per stream: the records in tile order, the carried
 * samples, the counters), as `rocprofv3 --kernel-trace` prints it. */
int fmd_modes_kernel_name(const fmd_modes *h, uint32_t pass, char *name, size_t cap);
/* Positions per workgroup of pass 0.  Host only. */
uint32_t fmd_modes_tile(void);
/* T_56 or T_112 above into table[n_bits] (n_bits 56 or 112, else FMD_ERR_UNSUPPORTED).  Host only. */
int fmd_modes_table(uint32_t n_bits, uint32_t *table);
/* syn above of a message of 7 or 14 bytes (else FMD_ERR_BAD_LENGTH).  Host only. */
int fmd_modes_syndrome(const uint8_t *bytes, size_t n_bytes, uint32_t *syn);
/* The fields of an extended squitter (DF 17, 18; host only).  has: bit 0 callsign (type codes 1-4: eight characters, trailing
 * blanks dropped), bit 1 altitude_ft (type codes 9-18 with the Q bit: 25 N - 1000), bit 2 the 17-bit CPR latitude and longitude with
 * the odd flag (type codes 9-18), bit 3 speed_kt, track_deg (clockwise from north) and vrate_fpm (type code 19, subtypes 1 and 2;
 * a component or a rate that is "not available" clears the bit).  Another DF or length: FMD_ERR_UNSUPPORTED. */
typedef struct fmd_modes_fields {
    uint32_t df, icao, type_code, subtype, has;
    int32_t  altitude_ft;
    uint32_t cpr_odd, cpr_lat, cpr_lon;
    int32_t  vrate_fpm;
    double   speed_kt, track_deg;
    char     callsign[16];
} fmd_modes_fields;
int fmd_modes_decode(const uint8_t *bytes, size_t n_bytes, fmd_modes_fields *out);
/* The globally unambiguous position of one even and one odd CPR pair of the same aircraft; latest_odd says which of the two is the
 * newer, whose position is returned in degrees.  FMD_ERR_BAD_STATE when the two lie in different longitude zones
 * or give no latitude within +-90 degrees (they are not a pair). */
int fmd_modes_cpr_global(uint32_t lat_even, uint32_t lon_even, uint32_t lat_odd, uint32_t lon_odd, int latest_odd, double *lat,
                         double *lon);

/* ---- Pulse bank: the on-off-keyed pulses of every stream as width / gap / level records, with a host slicer ------------- */
/* NEW SURFACE: the front half of rtl_433 at bank size.  The remotes, weather stations, tyre sensors and doorbells of the 315 / 433 /
 * 868 MHz bands key their carrier on and off; this handle takes the u8 IQ of many streams as read_sync delivers it and leaves every
 * pulse of every stream: its width, the gap in front of it and its level.  Integers only; the results do not depend on how a stream
 * is cut into calls.  Definition (tests/pulses_ref.py), per stream, i counting samples from creation or reset, everything at a
 * negative index 0:
 *   m[i]  = ((2 b[2i] - 255)^2 + (2 b[2i+1] - 255)^2) >> 1          (exactly the Mode S bank's m; a u16)
 *   e[i]  = m[i] + m[i-1] + ... + m[i-W+1]                            (a box of W samples; e <= 64 * 65025)
 *   s[i]  = 1 if e[i] >= hi;  0 if e[i] < lo;  else s[i-1];   s[-1] = 0     (a comparator with hysteresis)
 *   rise at i: s[i] = 1, s[i-1] = 0.     fall at i: s[i] = 0, s[i-1] = 1.
 * Every fall at f gives one record, in increasing f: k_rel = f - pos (0 <= k_rel < n: a fall is decided by the call that brings
 * sample f, there is no look-ahead); width = f - r, r the rise before f; gap = r - f_prev, f_prev the fall before r, and 0 if there
 * has been no fall since creation or reset; level = e[f - 1], the box over the pulse's last W samples.  width and gap saturate at
 * 2^32 - 1.  Per call and stream `count` is every fall of the call and the first min(count, pulse_cap) records are kept, whatever
 * the scheduling: overflow is decided by position alone.  Cumulative per stream (fmd_pulses_totals): samples, pulses (falls), rises,
 * the current s and `run`, the samples since the last edge or since reset -- `state == 0 && run >= reset` lets the host close a
 * package without waiting for the next pulse.  Carried per stream: the m of its last 64 samples, s, the run, the open pulse's gap and
 * the counters; all zeros is what reset leaves.  nbytes == 0 launches nothing and leaves the last call's results.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried): 1 <= W <= 64, 1 <= lo <= hi <= 64 * 65025,
 * 1 <= pulse_cap <= 1024, n_streams = dev->n_channels >= 1.  Calls: as fmd_modes_run_*: nbytes % 8 != 0 is FMD_ERR_BAD_LENGTH,
 * nbytes > cap_bytes FMD_ERR_CAPACITY, cap_bytes % 4 != 0 or a d_iq that is not 4-byte aligned FMD_ERR_INVALID_ARG.  Stream lifetime
 * and completion points: as fmd_channelizer_* (fmd_pulses_check).  Out of scope: adaptive thresholds on the device, FSK pulse
 * detection, a peak or mean over the whole pulse, glitch merging below a minimum width.  (Slicing on the device: the package bank,
 * fmd_packages_*, below.) */
typedef struct fmd_pulses fmd_pulses;
typedef struct fmd_pulses_config {
    uint32_t W;           /* 1 .. 64 */
    uint32_t lo, hi;      /* 1 <= lo <= hi <= 64 * 65025 */
    uint32_t pulse_cap;   /* 1 .. 1024 */
} fmd_pulses_config;
typedef struct fmd_pulses_rec {                                                 /* 16 bytes */
    int32_t  k_rel;
    uint32_t width, gap, level;
} fmd_pulses_rec;
/* (Read by fmd_pulses_info; the struct goes by another name as fmd_modes_totals does.) */
typedef struct fmd_pulses_totals {                                              /* 40 bytes */
    uint64_t samples, pulses, rises;
    uint32_t state;       /* the current s */
    uint32_t rsv;
    uint64_t run;
} fmd_pulses_totals;

int fmd_pulses_new(const fmd_pulses_config *cfg, const fmd_device_config *dev, fmd_pulses **out);   /* n_streams = dev->n_channels */
void fmd_pulses_free(fmd_pulses *h);
int fmd_pulses_reset(fmd_pulses *h);
/* HOST array iq [n_streams][cap_bytes], the first nbytes of each stream valid.  Returns when the call has completed. */
int fmd_pulses_run_batch(fmd_pulses *h, const uint8_t *iq, size_t nbytes, size_t cap_bytes);
/* DEVICE array of the same form, enqueued on `stream` without synchronising. */
int fmd_pulses_run_device(fmd_pulses *h, const void *d_iq, size_t nbytes, size_t cap_bytes, void *stream);
int fmd_pulses_check(fmd_pulses *h);
/* The last call's results, behind a synchronisation.  counts: host array [n_streams] (all 0 before the first call and after reset).
 * recs: host array [n_sel][pulse_cap] for the streams listed in `streams` only, in the order listed, zero behind each one's
 * min(count, pulse_cap); an index at or beyond n_streams is FMD_ERR_INVALID_ARG, with nothing written.  info: host array [n_streams]. */
int fmd_pulses_counts(fmd_pulses *h, uint32_t *counts);
int fmd_pulses_recs(fmd_pulses *h, const uint32_t *streams, size_t n_sel, fmd_pulses_rec *recs);
int fmd_pulses_info(fmd_pulses *h, fmd_pulses_totals *info);
/* Name of the kernel of pass 0 (the tiles: box, comparator, edges) or 1 (per stream: the records in tile order, the runs across
 * tiles and calls, the carried state), as `rocprofv3 --kernel-trace` prints it. */
int fmd_pulses_kernel_name(const fmd_pulses *h, uint32_t pass, char *name, size_t cap);
/* Positions per workgroup of pass 0.  Host only. */
uint32_t fmd_pulses_tile(void);

/* The host slicer behind the pulse bank (host only, fixed buffers; definition tests/pulse_slice_ref.py): pulse records of one stream
 * in, bit packages out.  A package is a maximal run of pulses in which every pulse but the first has gap < reset; it closes on the
 * next record with gap >= reset, or on fmd_pulse_slicer_idle with state == 0 && run >= reset.  Bits, as rtl_433 slices them -- PWM:
 * a pulse gives a 1 if |width - short_w| <= tol, else a 0 if |width - long_w| <= tol; PPM: every pulse but the package's first gives
 * a bit from its gap, 0 if |gap - short_w| <= tol, else 1 if |gap - long_w| <= tol.  A pulse that fits neither sets FMD_PULSE_BAD,
 * and the rest of the package gives no bits.  Up to 256 bits are kept, MSB first; a bit beyond sets FMD_PULSE_TRUNCATED.  n_pulses
 * counts every pulse of the package.  start is the absolute sample of the first pulse's rise.  Up to 64 closed packages wait for
 * fmd_pulse_slicer_take; one that closes while 64 wait is dropped.  The state lives in the object: a package may span calls.
 * Domain (else FMD_ERR_UNSUPPORTED): modulation 0 or 1, short_w, long_w and reset >= 1. */
#define FMD_PULSE_PWM 0u
#define FMD_PULSE_PPM 1u
#define FMD_PULSE_BAD 1u
#define FMD_PULSE_TRUNCATED 2u
typedef struct fmd_pulse_slicer fmd_pulse_slicer;
typedef struct fmd_pulse_slicer_config {
    uint32_t modulation;  /* FMD_PULSE_PWM | FMD_PULSE_PPM */
    uint32_t short_w, long_w, tol, reset;
} fmd_pulse_slicer_config;
typedef struct fmd_pulse_package {                                              /* 56 bytes */
    uint64_t start;
    uint32_t n_pulses, n_bits;
    uint8_t  bits[32];
    uint32_t flags;       /* FMD_PULSE_BAD | FMD_PULSE_TRUNCATED */
    uint32_t rsv;
} fmd_pulse_package;
int fmd_pulse_slicer_new(const fmd_pulse_slicer_config *cfg, fmd_pulse_slicer **out);
void fmd_pulse_slicer_free(fmd_pulse_slicer *p);
/* n records of one call, whose first sample is the absolute sample `pos` (a record's fall is at pos + k_rel). */
int fmd_pulse_slicer_push(fmd_pulse_slicer *p, const fmd_pulses_rec *recs, size_t n, uint64_t pos);
/* The stream's state and run behind a call (fmd_pulses_totals): closes the open package when the stream has been low for `reset`. */
int fmd_pulse_slicer_idle(fmd_pulse_slicer *p, uint32_t state, uint64_t run);
/* Moves the oldest min(waiting, cap) closed packages into packages[cap]; *n is how many. */
int fmd_pulse_slicer_take(fmd_pulse_slicer *p, fmd_pulse_package *packages, size_t cap, size_t *n);

/* ---- Package bank: the pulse records of every stream sliced into PWM / PPM bit packages on the device -------------------- */
/* NEW SURFACE: the host slicer above, one per stream of a pulse bank, on the device.  Definition (tests/packages_ref.py): for any
 * number of streams and any cutting into calls, stream s behaves as an fmd_pulse_slicer(modulation, short_w, long_w, tol, reset) of
 * its own that, per call, is pushed the first min(count_s, rec_cap) records with pos_s = samples_s - n_samples (u64; samples_s the
 * stream's fmd_pulses_totals.samples after the call), is then given idle(state_s, run_s), and has room for every package: the host
 * ring of 64 has no counterpart.  A call leaves per stream
 *   count  the delivered packages that closed in this call, all of them: the closes by a record with gap >= reset in record order,
 *          the close by idle last;
 *   pkgs   the first min(count, pkg_cap) of them as fmd_pulse_package: bits zero behind (n_bits + 7) / 8 bytes, rsv 0, start as
 *          the host slicer computes it (fall = pos + (int64) k_rel; start = fall >= width ? fall - width : 0);
 *   info   fmd_packages_totals, cumulative since creation or reset.
 * min_bits (0 ... 256) is the one addition over the host slicer: a closed package with n_bits < min_bits counts in `packages` and
 * `skipped`, takes no slot and is not in `count` (noise gives many one-pulse packages); min_bits = 0 is the host slicer exactly.
 * A call of R records read closes at most R + 1 packages (the carried one at record 0, each record's own at the next record, the
 * last by idle), so pkg_cap = rec_cap + 1 holds every package of a call: fmd_packages_max.  n_pulses saturates at 2^32 - 1.
 * Domain (else FMD_ERR_UNSUPPORTED with a text, decided before a device is queried), in this order: the host slicer's tests with
 * its texts; min_bits <= 256; 1 <= pkg_cap <= 1025; n_streams = dev->n_channels >= 1; per call 1 <= rec_cap <= 1024.
 * n_samples == 0 launches nothing and leaves the last call's results.  A count above rec_cap reads rec_cap records; whatever lies
 * behind a stream's min(count, rec_cap) records is never read.  Stream lifetime and completion points: as fmd_channelizer_*
 * (fmd_packages_check).  Reset: every stream as new. */
typedef struct fmd_packages fmd_packages;
struct fmd_packages_config {                                                    /* 28 bytes */
    fmd_pulse_slicer_config slicer;
    uint32_t min_bits;    /* 0 .. 256 */
    uint32_t pkg_cap;     /* 1 .. 1025 */
};
typedef struct fmd_packages_config fmd_packages_config;
/* (Read by fmd_packages_info; the struct goes by another name as fmd_pulses_totals does.) */
typedef struct fmd_packages_totals {                                            /* 40 bytes */
    uint64_t records;     /* records taken */
    uint64_t packages;    /* packages closed, delivered or not */
    uint64_t skipped;     /* of them, closed with n_bits < min_bits */
    uint64_t bad;         /* of them, closed with FMD_PULSE_BAD */
    uint32_t open;        /* 1 if a package is open */
    uint32_t open_pulses; /* the open package's n_pulses */
} fmd_packages_totals;

int fmd_packages_new(const fmd_packages_config *cfg, const fmd_device_config *dev, fmd_packages **out);   /* n_streams = dev->n_channels */
void fmd_packages_free(fmd_packages *h);
int fmd_packages_reset(fmd_packages *h);
/* HOST arrays counts [n_streams], recs [n_streams][rec_cap] and totals [n_streams], as the pulse bank's accessors give them after a
 * call of n_samples samples per stream.  Returns when the call has completed. */
int fmd_packages_run_batch(fmd_packages *h, const uint32_t *counts, const fmd_pulses_rec *recs, size_t rec_cap,
                           const fmd_pulses_totals *totals, size_t n_samples);
/* What `bank`'s last call that launched left, where it lies on the device: counts, records, state and that call's sample count.
 * Enqueued on `stream` without synchronising; nothing visits the host.  A bank on another device or with another n_streams is
 * FMD_ERR_INVALID_ARG, one that has not launched since creation or reset FMD_ERR_BAD_STATE.  The bank's results must still be
 * those of that call when the kernel runs: enqueue the bank's next call but one behind this one. */
int fmd_packages_run_bank(fmd_packages *h, fmd_pulses *bank, void *stream);
/* A call of no records whose idle test passes for every stream: the end of an input.  Its results are a call's results. */
int fmd_packages_flush(fmd_packages *h, void *stream);
int fmd_packages_check(fmd_packages *h);
/* The last call's results, behind a synchronisation.  counts: host array [n_streams] (all 0 before the first call and after reset).
 * pkgs: host array [n_sel][pkg_cap] for the streams listed in `streams` only, in the order listed, zero behind each one's
 * min(count, pkg_cap); an index at or beyond n_streams is FMD_ERR_INVALID_ARG, with nothing written.  info: host array [n_streams]. */
int fmd_packages_counts(fmd_packages *h, uint32_t *counts);
int fmd_packages_pkgs(fmd_packages *h, const uint32_t *streams, size_t n_sel, fmd_pulse_package *pkgs);
int fmd_packages_info(fmd_packages *h, fmd_packages_totals *info);
/* Name of the kernel, as `rocprofv3 --kernel-trace` prints it. */
int fmd_packages_kernel_name(const fmd_packages *h, char *name, size_t cap);
/* The packages a call of n_records records read can close at most: n_records + 1.  Host only. */
size_t fmd_packages_max(size_t n_records);

/* ---- pipelined, multi-GPU sink for read_sync buffers ------------------------------------------------------- */
/* NEW SURFACE (the reference has no asynchronous reader).  It mirrors the hand-off the example
 * does have: receive() fills a buffer with RtlSdr::read_sync (src/lib.rs:153) and sends it down an mpsc channel,
 * process() demodulates it and calls output() (examples/simple_fm.rs:55-60,114-127,150-156).  Here the channel
 * is a ring of `depth` page-locked slots and the consumer is one Demod bank per GPU: channels are split into
 * contiguous ranges over `device_ids` (one Demod per stream, :137 -- no communication between devices); host ->
 * device copy of buffer n+1, the kernel of buffer n and the device -> host copy of buffer n-1 overlap.
 *   fmd_sink_acquire: the next slot to fill, [n_channels][nbytes] channel-major (blocks only when all `depth`
 *                     slots are in flight: then the oldest is completed first);
 *   fmd_sink_submit : enqueue it on every device and return without waiting;
 *   fmd_sink_release: give the acquired slot back unsubmitted (a short read_sync ends the run, simple_fm.rs:122-125);
 *   completion, in submission order, from inside acquire / poll / drain on the caller's thread:
 *       callback(user, seq, audio [n_channels][out_cap], out_len [n_channels], out_cap, status)
 *     -- `audio` is valid during the callback only; status FMD_OK or the first error of that buffer.
 * Results are exactly those of feeding the same buffers to fmd_demod_demodulate_batch one by one, with ONE stated
 * exception: a buffer so short that it yields no audio sample at all carries its f64 sample (simple_fm.rs:359) in the
 * partial sum handed to the next buffer; with depth > 1 the next launch may already be enqueued when that sample turns
 * out to need the host-libm correction (probability ~2^-36 per buffer, see fmd_demod_check) -- that buffer is then
 * delivered with status FMD_ERR_HIP instead of silently different audio.  read_sync-sized buffers never get there.
 * A submit that fails after it has touched a device cannot be rolled back (the Demod state of the parts before the
 * failing one has advanced): it is terminal for the sink -- this and every later acquire / submit return the same
 * error, poll / drain still deliver what was submitted before and then return it too. */
typedef struct fmd_sink fmd_sink;
typedef void (*fmd_sink_callback)(void *user, uint64_t seq, const int16_t *audio, const size_t *out_len,
                                  size_t out_cap, int status);
int fmd_sink_new(const fmd_demod_config *config, uint32_t n_channels, const int32_t *device_ids, uint32_t n_devices,
                 size_t nbytes, uint32_t depth, fmd_sink_callback callback, void *user, fmd_sink **out);
void fmd_sink_free(fmd_sink *s);
int fmd_sink_acquire(fmd_sink *s, uint8_t **iq);
int fmd_sink_submit(fmd_sink *s);
int fmd_sink_release(fmd_sink *s);
int fmd_sink_poll(fmd_sink *s);     /* deliver what has finished; returns the number of buffers delivered or < 0 */
int fmd_sink_drain(fmd_sink *s);    /* wait for and deliver everything in flight */
int fmd_sink_info(const fmd_sink *s, size_t *out_cap, uint32_t *n_devices, uint32_t *in_flight);
/* f64 samples that fell into the guard band / that the host libm corrected, summed over the device parts (fmd_demod_f64_stats). */
int fmd_sink_f64_stats(const fmd_sink *s, uint64_t *guarded, uint64_t *patched);

/* ---- rtl_tcp client-side IQ source ---------------------------------------------------- */
/* The reference ships the rtl_tcp SERVER (examples/rtl_tcp.rs); this is the matching client, so that a dongle on another
 * host feeds the sinks above without USB code here.  Wire format: a 12-byte handshake "RTL0" + tuner type + tuner gain
 * count, both u32 big-endian (send_handshake, examples/rtl_tcp.rs:691-697); then raw interleaved u8 IQ exactly as
 * RtlSdr::read_sync delivered it (sender_loop, :609-631); commands are 5 bytes, opcode + big-endian 32-bit parameter
 * (command_loop, :639-678).  Host code only (no GPU needed).
 *   fmd_rtltcp_open     : connect (timeout_ms, 0 = 10 s) and read the handshake; FMD_ERR_IO when it is not "RTL0";
 *   fmd_rtltcp_read_sync: RtlSdr::read_sync (src/lib.rs:153) -- fill buf, *n_read = bytes written; FEWER than nbytes
 *                         means the stream ended, which the reference's callers treat as "samples lost"
 *                         (examples/simple_fm.rs:122); a socket error or a timeout returns FMD_ERR_IO with
 *                         *n_read = the bytes that did arrive (the stream keeps its I/Q byte alignment);
 *   fmd_rtltcp_command  : one command; a negative (i32) parameter travels as its two's complement. */
typedef struct fmd_rtltcp fmd_rtltcp;
#define FMD_RTLTCP_SET_FREQUENCY       0x01   /* opcodes of command_loop, examples/rtl_tcp.rs:659-675 */
#define FMD_RTLTCP_SET_SAMPLE_RATE     0x02
#define FMD_RTLTCP_SET_GAIN_MODE       0x03
#define FMD_RTLTCP_SET_GAIN            0x04
#define FMD_RTLTCP_SET_FREQ_CORRECTION 0x05
#define FMD_RTLTCP_SET_IF_GAIN         0x06
#define FMD_RTLTCP_SET_TEST_MODE       0x07
#define FMD_RTLTCP_SET_AGC_MODE        0x08
#define FMD_RTLTCP_SET_DIRECT_SAMPLING 0x09
#define FMD_RTLTCP_SET_OFFSET_TUNING   0x0a
#define FMD_RTLTCP_SET_RTL_XTAL        0x0b
#define FMD_RTLTCP_SET_TUNER_XTAL      0x0c
#define FMD_RTLTCP_SET_GAIN_BY_INDEX   0x0d
#define FMD_RTLTCP_SET_BIAS_TEE        0x0e
int fmd_rtltcp_open(const char *host, uint16_t port, uint32_t timeout_ms, fmd_rtltcp **out);
void fmd_rtltcp_close(fmd_rtltcp *s);
int fmd_rtltcp_info(const fmd_rtltcp *s, uint32_t *tuner_type, uint32_t *gain_count);
int fmd_rtltcp_read_sync(fmd_rtltcp *s, uint8_t *buf, size_t nbytes, size_t *n_read);
/* read_sync for MANY sources behind one poll(): row c (row_stride bytes apart, the first nbytes of it) is filled from
 * sources[c], n_read[c] = bytes written to it.  FMD_OK with n_read[c] < nbytes: that stream ended early; FMD_ERR_IO: a
 * socket error, or no byte on any unfinished stream within the smallest timeout of the sources (n_read as far as it
 * got).  The receive() loop of simple_fm.rs:100-132 for a bank of streams. */
int fmd_rtltcp_read_many(fmd_rtltcp *const *sources, uint32_t n, uint8_t *base, size_t row_stride, size_t nbytes,
                         size_t *n_read);
int fmd_rtltcp_command(fmd_rtltcp *s, uint8_t opcode, uint32_t param);
/* receive() (simple_fm.rs:89-132) for a bank of rtl_tcp streams, below the binding: acquire the next slot, fill row c from
 * sources[c] (n_sources must equal the sink's n_channels; fmd_rtltcp_read_many: ONE poll() loop over all sockets) and
 * submit it.  *n_short = sources that ended before their row was full: when > 0 the slot has been released unsubmitted
 * and the run is over ("samples lost", :122-125) -- the sink stays usable, drain it to get what was submitted before.
 * fmd_sink_pump_rtltcp repeats that until a short read or max_buffers (0 = no limit) and then drains;
 * *n_submitted = buffers that went to the GPUs. */
int fmd_sink_fill_from_rtltcp(fmd_sink *s, fmd_rtltcp *const *sources, uint32_t n_sources, uint32_t *n_short);
int fmd_sink_pump_rtltcp(fmd_sink *s, fmd_rtltcp *const *sources, uint32_t n_sources, uint64_t max_buffers,
                         uint64_t *n_submitted);

/* ---- diagnostics ---------------------------------------------------------------------- */
const char *fmd_strerror(int status);
const char *fmd_last_error(void);          /* thread-local detail of the last failure          */
int fmd_device_count(int *count);          /* gfx950 devices visible to HIP                    */
int fmd_version(void);                     /* FMD_VERSION_MAJOR * 1000 + FMD_VERSION_MINOR     */
/* Kernel tiling (for benchmarks / DESIGN.md bookkeeping): of the handle's most recent launch,
 * or, before the first one, what a bank fed whole read_sync buffers will run. */
int fmd_demod_tiling(const fmd_demod *d, uint32_t *audio_per_tile, uint32_t *lds_bytes,
                     uint32_t *block_threads);
/* Which plan chose the LDS kernels' tile (diagnostics for measured rows): 0 = the caller (fmd_demod_set_tiling), 1 = the largest
 * tile that keeps 8 blocks per CU resident (20 KB), 2 = the 15.5 ... 17.3 KB window of the rows on the memory side; negative on
 * a null handle.  (The register-streaming kernel of downsample 2 / 4 has a tiling of its own: fmd_demod_tiling reports it.) */
int fmd_demod_tiling_plan(const fmd_demod *d);
/* Name of the kernel the handle's most recent launch ran, as `rocprofv3 --kernel-trace` prints
 * it (e.g. "fmd_tk::fmd_demod_tile_kernel<5, 2>"); "" before the first launch.  bench.py
 * quotes it in `roofline.kernel` instead of a constant. */
int fmd_demod_last_kernel(const fmd_demod *d, char *name, size_t cap);
/* Override the tiling (audio samples per workgroup tile; 0 = automatic).  Results never
 * depend on it; it exists for tuning sweeps. */
int fmd_demod_set_tiling(fmd_demod *d, uint32_t audio_per_tile);

#ifdef __cplusplus
}
#endif
#endif /* FMD_H */
