"""Host-side wrapper of the power-spectrum scanner (include/fmd.h, fmd_spectrum_*): the integrated power of N DFT bins of each IQ
stream, and `find_stations`, which picks the FM stations out of such a spectrum so that a StationBank can be tuned to them."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, CheckedHandle, check, lib


def hann_window(n_bins, amplitude=2047):
    """The library's exact integer Hann window (int16, n_bins entries); amplitude <= 127 gives the one-digit tap form."""
    w = np.zeros(int(n_bins), dtype=np.int16)
    check(lib().fmd_spectrum_hann(int(n_bins), int(amplitude), w.ctypes.data_as(C.POINTER(C.c_int16))))
    return w


class Spectrum(CheckedHandle):
    """N-bin power spectrum of `n_streams` streams: frames of N samples every `hop` samples, |DFT|^2 >> shift summed over the
    frames of a call (u64, natural DFT order).  `window` defaults to hann_window(n_bins)."""
    _prefix = "spectrum"

    def __init__(self, n_bins, hop=None, window=None, shift=0, n_streams=1, device_id=-1):
        self.n_bins, self.n_streams = int(n_bins), int(n_streams)
        self.hop = self.n_bins if hop is None else int(hop)
        self.shift = int(shift)
        self.window = np.ascontiguousarray(hann_window(self.n_bins) if window is None else window, dtype=np.int16)
        self._h = C.c_void_p()
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(lib().fmd_spectrum_new(self.window.ctypes.data_as(C.POINTER(C.c_int16)), self.window.size, self.hop, self.shift,
                                     C.byref(dev), C.byref(self._h)))

    def frames(self, nbytes):
        return int(lib().fmd_spectrum_frames(self.n_bins, self.hop, int(nbytes)))

    def power_batch(self, iq):
        """iq uint8 [n_streams, nbytes] -> uint64 [n_streams, n_bins]."""
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim != 2 or iq.shape[0] != self.n_streams:
            raise ValueError("iq must be [n_streams, nbytes]")
        out = np.zeros((self.n_streams, self.n_bins), dtype=np.uint64)
        check(lib().fmd_spectrum_power_batch(self._h, iq.ctypes.data, iq.shape[1], out.ctypes.data))
        return out

    def power_device(self, d_iq, nbytes, d_power, accumulate=False, stream=None):
        """Enqueue on device pointers (d_power [n_streams][n_bins] u64).  `stream` must stay alive until the handle's next
        `power_device` call or `check` has returned (stream lifetime rule of include/fmd.h)."""
        check(lib().fmd_spectrum_power_device(self._h, d_iq, int(nbytes), d_power, 1 if accumulate else 0, stream))

    def tap_digits(self):
        return int(lib().fmd_spectrum_tap_digits(self._h))

    def bin_offsets_hz(self, rate):
        """Offset of every bin (natural DFT order) from the capture's centre, in Hz."""
        k = np.arange(self.n_bins)
        return np.where(k < self.n_bins // 2, k, k - self.n_bins) * (float(rate) / self.n_bins)

    def bin_inc(self, k):
        """The StationBank phase_inc that tunes to the centre of bin k."""
        inc = C.c_uint32(0)
        check(lib().fmd_spectrum_bin_inc(int(k) % self.n_bins, self.n_bins, C.byref(inc)))
        return inc.value


def find_stations(power, rate, count, channel_hz=200e3, min_snr_db=10.0):
    """Up to `count` stations in one spectrum (`power` in natural DFT order, as Spectrum returns it for one stream).

    A wideband FM station is spread over +-75 kHz, and a tone-modulated one peaks at its band edges, so the spectrum is first
    smoothed with a boxcar one channel wide.  The local maxima of the smoothed spectrum, strongest first, are taken at least one
    channel apart and at least `min_snr_db` above the median bin.  Each is reported as the power-weighted centroid of the raw
    bins within half a channel of it.  Returns (offsets_hz, bins) in increasing frequency; `bins` are the natural-order bins
    nearest to the offsets (Spectrum.bin_inc of them tunes a StationBank)."""
    p = np.asarray(power, dtype=np.float64).ravel()
    N = p.size
    df = float(rate) / N
    order = np.fft.fftshift(np.arange(N))                   # natural bins in frequency order
    pf = p[order]
    f = (np.arange(N) - N // 2) * df
    half = max(0, int(round(channel_hz / df)) // 2)
    ones = np.ones(2 * half + 1)
    smooth = np.convolve(pf, ones, mode="same") / np.convolve(np.ones(N), ones, mode="same")
    noise = max(float(np.median(p)), 1e-300)
    peaks = [i for i in range(N) if (i == 0 or smooth[i] >= smooth[i - 1]) and (i == N - 1 or smooth[i] >= smooth[i + 1])]
    peaks.sort(key=lambda i: -smooth[i])
    picked = []
    for i in peaks:
        if len(picked) >= count:
            break
        if 10.0 * np.log10(max(smooth[i], 1e-300) / noise) < min_snr_db:
            break
        if any(abs(f[i] - f[j]) < channel_hz for j in picked):
            continue
        picked.append(i)
    offs = []
    for i in sorted(picked):
        lo, hi = max(0, i - half), min(N, i + half + 1)
        w = pf[lo:hi]
        offs.append(float((w * f[lo:hi]).sum() / w.sum()) if w.sum() > 0 else float(f[i]))
    offs = np.array(offs, dtype=np.float64)
    bins = (np.round(offs / df).astype(np.int64) % N) if offs.size else np.zeros(0, np.int64)
    return offs, bins
