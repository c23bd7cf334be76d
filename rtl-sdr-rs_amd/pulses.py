"""Host-side wrapper of the pulse bank (include/fmd.h, fmd_pulses_*) and of the host slicer behind it (fmd_pulse_slicer_*): the front
half of rtl_433 at bank size.  The bank takes the u8 IQ of many streams and leaves every on-off-keyed pulse of every stream as a record
of its width, the gap in front of it and its level -- a box envelope of W samples, a comparator with hysteresis and run lengths, exact
in integers and independent of how a stream is cut into calls.  The slicer turns one stream's records into PWM or PPM bit packages.
With them: the sender of one package (ook_encode) and thresholds from a quiet capture (pulse_thresholds)."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, RecordBank, check, lib

PWM, PPM = 0, 1
PULSE_BAD, PULSE_TRUNCATED = 1, 2
E_MAX = 64 * 65025                                           # the largest box sum


class PulsesConfig(C.Structure):
    """struct fmd_pulses_config"""
    _fields_ = [("W", C.c_uint32), ("lo", C.c_uint32), ("hi", C.c_uint32), ("pulse_cap", C.c_uint32)]


class PulseRec(C.Structure):
    """struct fmd_pulses_rec"""
    _fields_ = [("k_rel", C.c_int32), ("width", C.c_uint32), ("gap", C.c_uint32), ("level", C.c_uint32)]


class PulsesTotals(C.Structure):
    """struct fmd_pulses_totals"""
    _fields_ = [("samples", C.c_uint64), ("pulses", C.c_uint64), ("rises", C.c_uint64), ("state", C.c_uint32), ("rsv", C.c_uint32),
                ("run", C.c_uint64)]


class PulseSlicerConfig(C.Structure):
    """struct fmd_pulse_slicer_config"""
    _fields_ = [("modulation", C.c_uint32), ("short_w", C.c_uint32), ("long_w", C.c_uint32), ("tol", C.c_uint32), ("reset", C.c_uint32)]


class PulsePackage(C.Structure):
    """struct fmd_pulse_package"""
    _fields_ = [("start", C.c_uint64), ("n_pulses", C.c_uint32), ("n_bits", C.c_uint32), ("bits", C.c_uint8 * 32), ("flags", C.c_uint32),
                ("rsv", C.c_uint32)]


def pulses_tile():
    """Positions per workgroup of the bank's first pass."""
    return int(lib().fmd_pulses_tile())


def _modulation(m):
    if m in ("pwm", "PWM", PWM):
        return PWM
    if m in ("ppm", "PPM", PPM):
        return PPM
    raise ValueError("modulation must be pwm or ppm")


def ook_encode(bits, modulation, short, long, gap, amplitude=60, lead=0, trail=0):
    """The sender: the u8 IQ (uint8 [2 n]) of one package of `bits` (0 / 1, first sent first).  PWM: a pulse per bit, `short` samples
    wide for a 1 and `long` for a 0, with `gap` quiet samples behind each.  PPM: len(bits) + 1 pulses of `gap` samples each, and
    between two of them `short` quiet samples for a 0 and `long` for a 1.  `lead` quiet samples in front and `trail` behind.  A pulse
    is I = 128 + amplitude, Q = 128; quiet is 128, 128."""
    mod, bits = _modulation(modulation), [int(b) & 1 for b in bits]
    short, long, gap = int(short), int(long), int(gap)
    if min(short, long, gap) < 1 or not 0 < int(amplitude) <= 127:
        raise ValueError("need short, long, gap >= 1 and 0 < amplitude <= 127")
    runs = [(0, int(lead))]                                  # (on, samples)
    if mod == PWM:
        for b in bits:
            runs += [(1, short if b else long), (0, gap)]
    else:
        runs.append((1, gap))
        for b in bits:
            runs += [(0, long if b else short), (1, gap)]
    runs.append((0, int(trail)))
    on = np.concatenate([np.full(n, v, bool) for v, n in runs]) if runs else np.zeros(0, bool)
    iq = np.full((on.size, 2), 128, np.uint8)
    iq[on, 0] = 128 + int(amplitude)
    return iq.reshape(-1)


def pulse_thresholds(iq, W=8, factor=4.0):
    """(lo, hi) for the bank from a quiet capture (u8 IQ, uint8 [2 n], n >= W): hi is `factor` times the median of the box sum e over
    the capture and lo half of hi, both inside the bank's domain.  Plain numpy: the host's stand-in for adaptive thresholds."""
    b = np.asarray(iq, np.uint8).reshape(-1).astype(np.int64)
    W = int(W)
    if not 1 <= W <= 64 or b.size < 2 * W or b.size % 2:
        raise ValueError("need 1 <= W <= 64 and at least W samples")
    m = ((2 * b[0::2] - 255) ** 2 + (2 * b[1::2] - 255) ** 2) >> 1
    c = np.concatenate([[0], np.cumsum(m)])
    e = c[W:] - c[:-W]
    hi = int(min(E_MAX, max(2, round(float(factor) * float(np.median(e))))))
    return max(1, hi // 2), hi


def _rec_dict(r):
    return {"k_rel": r.k_rel, "width": r.width, "gap": r.gap, "level": r.level}


class PulseBank(RecordBank):
    """The pulse bank (fmd_pulses_*): `n_streams` streams of u8 IQ.  run takes uint8 [n_streams, nbytes] on the host, run_device the
    same on the device; both return nothing.  Behind a call: counts() uint32 [n_streams], every fall of the call; pulses(streams) the
    first min(count, pulse_cap) records of each listed stream in increasing position, as dicts {"k_rel", "width", "gap", "level"}
    (k_rel: the fall, counted from the call's first sample); info() the streams' cumulative counters {"samples", "pulses", "rises",
    "state", "run"}."""
    _prefix, _cap, _reader, _record, _info, _as_dict = "pulses", "pulse_cap", "recs", PulseRec, PulsesTotals, staticmethod(_rec_dict)
    _passes = 2
    pulses = RecordBank.delivered

    def __init__(self, n_streams=1, W=8, lo=30000, hi=60000, pulse_cap=64, device_id=-1):
        self.n_streams = self.n_rows = int(n_streams)
        self.W, self.lo, self.hi, self.pulse_cap = int(W), int(lo), int(hi), int(pulse_cap)
        for name in ("n_streams", "W", "lo", "hi", "pulse_cap"):
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        self._h = C.c_void_p()
        cfg = PulsesConfig(self.W, self.lo, self.hi, self.pulse_cap)
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(lib().fmd_pulses_new(C.byref(cfg), C.byref(dev), C.byref(self._h)))

    def info(self):
        return [{k: v for k, v in i.items() if k != "rsv"} for i in super().info()]

    def kernel_name(self, which=0):
        """The kernel of pass `which` (0: the tiles, 1: per stream), as rocprofv3 --kernel-trace prints it."""
        buf = C.create_string_buffer(128)
        check(lib().fmd_pulses_kernel_name(self._h, int(which), buf, len(buf)))
        return buf.value.decode()

    def run(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim != 2 or iq.shape[0] != self.n_streams:
            raise ValueError("iq must be [n_streams, nbytes]")
        check(lib().fmd_pulses_run_batch(self._h, iq.ctypes.data, iq.shape[1], iq.shape[1]))

    def run_device(self, d_iq, nbytes, cap_bytes, stream=None):
        """Enqueue on a device pointer (d_iq [n_streams][cap_bytes], the first nbytes of each stream valid).  `stream` must stay alive
        until the handle's next `run_device` call or `check` has returned (include/fmd.h)."""
        check(lib().fmd_pulses_run_device(self._h, d_iq, nbytes, cap_bytes, stream))


class PulseSlicer:
    """The host slicer (fmd_pulse_slicer_*) of one stream: push(records, pos) takes the records of a call whose first sample is the
    absolute sample `pos` (dicts as PulseBank.pulses gives them), idle(state, run) the stream's state behind the call, take() returns
    the closed packages as dicts {"start", "n_pulses", "n_bits", "bits" (32 bytes, MSB first), "flags"}."""

    def __init__(self, modulation, short, long, tol, reset):
        self._h = C.c_void_p()
        cfg = PulseSlicerConfig(_modulation(modulation), int(short), int(long), int(tol), int(reset))
        check(lib().fmd_pulse_slicer_new(C.byref(cfg), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib().fmd_pulse_slicer_free(self._h)
            self._h = None

    def push(self, records, pos):
        buf = (PulseRec * max(1, len(records)))(*[PulseRec(r["k_rel"], r["width"], r["gap"], r.get("level", 0)) for r in records])
        check(lib().fmd_pulse_slicer_push(self._h, buf, len(records), int(pos)))

    def idle(self, state, run):
        check(lib().fmd_pulse_slicer_idle(self._h, int(state), int(run)))

    def take(self, cap=64):
        buf, n = (PulsePackage * max(1, int(cap)))(), C.c_size_t(0)
        check(lib().fmd_pulse_slicer_take(self._h, buf, int(cap), C.byref(n)))
        return [{"start": int(k.start), "n_pulses": k.n_pulses, "n_bits": k.n_bits, "bits": bytes(k.bits), "flags": k.flags} for k in buf[:n.value]]


def package_bits(package):
    """The bits of a package as a list of 0 / 1."""
    return np.unpackbits(np.frombuffer(package["bits"], np.uint8))[:package["n_bits"]].tolist()
