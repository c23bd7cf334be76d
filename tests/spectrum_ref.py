"""Test-side definition of the power-spectrum scanner (include/fmd.h, "power spectrum") in numpy integers.  Independent of the
library."""
import numpy as np

import stations_ref as sr

BINS = (16, 32, 64, 128, 256)


def hann(N, A):
    """w[n] = (A (16384 - TAB[(n 1024 / N) & 1023]) + 16384) >> 15."""
    n = np.arange(N)
    return ((A * (16384 - sr.TAB[(n * (1024 // N)) & 1023]) + 16384) >> 15).astype(np.int16)


def bin_inc(k, N):
    return (k * (1 << 32) // N) % (1 << 32)


def taps(window):
    """[N, N] Wr, Wi: the station bank's complex taps at inc_k = k 2^32 / N."""
    N = len(window)
    w = [sr.complex_taps(window, bin_inc(k, N)) for k in range(N)]
    return np.stack([a for a, _ in w]), np.stack([b for _, b in w])


def digits(window):
    wr, wi = taps(window)
    return 1 if max(np.abs(wr).max(), np.abs(wi).max()) <= 127 else 2


def frames(N, hop, nbytes):
    ns = nbytes // 2
    return 0 if ns < N else (ns - N) // hop + 1


def power(window, hop, shift, iq):
    """iq uint8 [S, nbytes] -> uint64 [S, N]: P[s][k] = sum_f ((zr^2 + zi^2) >> shift) mod 2^64."""
    iq = np.atleast_2d(np.asarray(iq, dtype=np.uint8))
    N = len(window)
    F = frames(N, hop, iq.shape[1])
    assert F >= 1
    wr, wi = taps(window)
    out = np.zeros((iq.shape[0], N), dtype=np.uint64)
    idx = np.arange(F)[:, None] * hop + np.arange(N)[None, :]     # [F, N] sample indices
    for s in range(iq.shape[0]):
        cr = iq[s, 0::2].astype(np.int64) - 127
        ci = iq[s, 1::2].astype(np.int64) - 127
        xr, xi = cr[idx], ci[idx]                                   # [F, N]
        zr = xr @ wr.T - xi @ wi.T                                  # [F, K]; |z| < 2^31, exact in int64
        zi = xr @ wi.T + xi @ wr.T
        p = ((zr * zr + zi * zi).astype(np.uint64)) >> np.uint64(shift)
        out[s] = p.sum(axis=0, dtype=np.uint64)                    # wraps modulo 2^64
    return out


def power_chunked(window, hop, shift, iq, chunk=1 << 14):
    """power() for long calls: frames in chunks of `chunk`, z from float64 products.  Every product c W and every partial sum is
    an integer below 2^27 in magnitude (|c| <= 128, |W| <= 2047, N <= 256), so float64 holds each exactly whatever order the
    matrix product sums in; the squares and the mod-2^64 sum are done in 64-bit integers as in power()."""
    iq = np.atleast_2d(np.asarray(iq, dtype=np.uint8))
    N = len(window)
    F = frames(N, hop, iq.shape[1])
    assert F >= 1
    wr, wi = (a.astype(np.float64) for a in taps(window))
    out = np.zeros((iq.shape[0], N), dtype=np.uint64)
    for s in range(iq.shape[0]):
        cr = iq[s, 0::2].astype(np.float64) - 127
        ci = iq[s, 1::2].astype(np.float64) - 127
        for f0 in range(0, F, chunk):
            idx = np.arange(f0, min(F, f0 + chunk))[:, None] * hop + np.arange(N)[None, :]
            xr, xi = cr[idx], ci[idx]
            zr = (xr @ wr.T - xi @ wi.T).astype(np.int64)
            zi = (xr @ wi.T + xi @ wr.T).astype(np.int64)
            p = ((zr * zr + zi * zi).astype(np.uint64)) >> np.uint64(shift)
            out[s] += p.sum(axis=0, dtype=np.uint64)
    return out
