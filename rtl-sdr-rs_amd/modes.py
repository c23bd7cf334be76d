"""Host-side wrapper of the Mode S bank (include/fmd.h, fmd_modes_*): the ADS-B messages -- 1090 MHz extended squitter, rtl_adsb's job
-- of many 2 Msample/s u8 IQ streams, decoded on the device: every sample position of every stream is tried as a preamble, a passing
one gives 112 bit decisions and a 24-bit syndrome, and only the accepted messages come back.  Exact in integers and independent of
how a stream is cut into calls.  With it: the sender of one message (modes_encode), the syndrome and parity of a message, the field
decoder of extended squitters (modes_fields), the global CPR solve (cpr_global) and the host's policy for overlapping acceptances
(modes_dedupe)."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, RecordBank, check, lib

MODES_GENERATOR = 0xFFF409
MODES_TAIL = 239                                             # a position is decided by the call that brings the sample p + 239


class ModesConfig(C.Structure):
    """struct fmd_modes_config"""
    _fields_ = [("min_power", C.c_uint32), ("fix_errors", C.c_uint32), ("df11", C.c_uint32), ("msg_cap", C.c_uint32)]


class ModesMsg(C.Structure):
    """struct fmd_modes_msg"""
    _fields_ = [("k_rel", C.c_int32), ("power", C.c_uint32), ("n_bytes", C.c_uint8), ("fixed_bit", C.c_uint8), ("df", C.c_uint8),
                ("rsv", C.c_uint8), ("bytes", C.c_uint8 * 14), ("pad", C.c_uint8 * 6)]


class ModesTotals(C.Structure):
    """struct fmd_modes_totals"""
    _fields_ = [("samples", C.c_uint64), ("candidates", C.c_uint64), ("messages", C.c_uint64), ("fixed", C.c_uint64)]


class ModesFields(C.Structure):
    """struct fmd_modes_fields"""
    _fields_ = [("df", C.c_uint32), ("icao", C.c_uint32), ("type_code", C.c_uint32), ("subtype", C.c_uint32), ("has", C.c_uint32),
                ("altitude_ft", C.c_int32), ("cpr_odd", C.c_uint32), ("cpr_lat", C.c_uint32), ("cpr_lon", C.c_uint32),
                ("vrate_fpm", C.c_int32), ("speed_kt", C.c_double), ("track_deg", C.c_double), ("callsign", C.c_char * 16)]


def modes_tile():
    """Positions per workgroup of the bank's first pass."""
    return int(lib().fmd_modes_tile())


def modes_table(n_bits=112):
    """T_56 or T_112 of include/fmd.h as uint32 [n_bits]: the syndrome of a message is the XOR of the entries at its set bits."""
    t = np.zeros(int(n_bits), np.uint32)
    check(lib().fmd_modes_table(int(n_bits), t.ctypes.data))
    return t


def _as_bytes(msg):
    if isinstance(msg, dict):
        msg = msg["bytes"]
    if isinstance(msg, str):
        msg = bytes.fromhex(msg)
    return bytes(msg)


def modes_syndrome(msg):
    """The 24-bit syndrome of a message of 7 or 14 bytes (bytes, a hex string or a record): 0 for a valid extended squitter."""
    b = _as_bytes(msg)
    buf, syn = (C.c_uint8 * len(b)).from_buffer_copy(b) if b else None, C.c_uint32(0)
    check(lib().fmd_modes_syndrome(buf, len(b), C.byref(syn)))
    return syn.value


def modes_frame(data, overlay=0):
    """`data` (4 or 11 bytes) with its 24 parity bits behind it, XOR `overlay` (DF 11: the interrogator's 7-bit IID)."""
    data = _as_bytes(data)
    p = modes_syndrome(data + b"\0\0\0") ^ int(overlay)
    return data + bytes([(p >> 16) & 255, (p >> 8) & 255, p & 255])


def modes_df11(address, iid=0, capability=5):
    """The 7 bytes of an all-call reply (DF 11) of the 24-bit `address` to the interrogator `iid` (0 ... 127; 0: a squitter)."""
    address = int(address)
    if not 0 <= address < 1 << 24 or not 0 <= int(iid) < 128 or not 0 <= int(capability) < 8:
        raise ValueError("need address < 2^24, iid < 128 and capability < 8")
    return modes_frame(bytes([11 << 3 | int(capability), address >> 16, (address >> 8) & 255, address & 255]), iid)


def modes_encode(msg, amplitude=60, lead=0, trail=0):
    """The sender: the u8 IQ (uint8 [2 (lead + 16 + 2 n_bits + trail)]) of one message of 7 or 14 bytes at 2 Msample/s: `lead` quiet
    samples, the four preamble pulses at the samples 0, 2, 7 and 9, from sample 16 two samples per bit -- pulse then gap for a 1, gap
    then pulse for a 0 -- and `trail` quiet samples.  A pulse is I = 128 + amplitude, Q = 128; quiet is 128, 128."""
    b = _as_bytes(msg)
    if len(b) not in (7, 14) or not 0 < int(amplitude) <= 127:
        raise ValueError("need 7 or 14 bytes and 0 < amplitude <= 127")
    bits = np.unpackbits(np.frombuffer(b, np.uint8))
    on = np.zeros(int(lead) + 16 + 2 * bits.size + int(trail), bool)
    on[int(lead) + np.array([0, 2, 7, 9])] = True
    on[int(lead) + 16 + 2 * np.arange(bits.size) + (1 - bits)] = True
    iq = np.full((on.size, 2), 128, np.uint8)
    iq[on, 0] = 128 + int(amplitude)
    return iq.reshape(-1)


def modes_dedupe(records):
    """Host policy, not part of the device result (the device suppresses nothing): `records` -- dicts in increasing position "p"
    (absolute; "k_rel" where there is none) -- without every record that begins inside an earlier kept one, which spans 16 + 16
    n_bytes samples."""
    out, busy = [], None
    for r in records:
        p = r["p"] if "p" in r else r["k_rel"]
        if busy is not None and p < busy:
            continue
        out.append(r)
        busy = p + 16 + 16 * r["n_bytes"]
    return out


def modes_fields(msg):
    """What an extended squitter (DF 17, 18; bytes, a hex string or a record) says, as a dict: df, icao, type_code, subtype and,
    where the type code carries them, callsign; altitude_ft; cpr_odd, cpr_lat, cpr_lon; speed_kt, track_deg, vrate_fpm."""
    b = _as_bytes(msg)
    f = ModesFields()
    check(lib().fmd_modes_decode((C.c_uint8 * len(b)).from_buffer_copy(b) if b else None, len(b), C.byref(f)))
    out = {"df": f.df, "icao": f.icao, "type_code": f.type_code, "subtype": f.subtype}
    if f.has & 1:
        out["callsign"] = f.callsign.decode()
    if f.has & 2:
        out["altitude_ft"] = f.altitude_ft
    if f.has & 4:
        out.update(cpr_odd=f.cpr_odd, cpr_lat=f.cpr_lat, cpr_lon=f.cpr_lon)
    if f.has & 8:
        out.update(speed_kt=f.speed_kt, track_deg=f.track_deg, vrate_fpm=f.vrate_fpm)
    return out


def cpr_global(even, odd, latest="even"):
    """(latitude, longitude) in degrees from one even and one odd airborne position of the same aircraft (messages, or their
    modes_fields dicts); `latest` names the newer of the two, whose position it is.  None when the pair straddles a longitude zone."""
    e = even if isinstance(even, dict) and "cpr_lat" in even else modes_fields(even)
    o = odd if isinstance(odd, dict) and "cpr_lat" in odd else modes_fields(odd)
    if e.get("cpr_odd") != 0 or o.get("cpr_odd") != 1 or latest not in ("even", "odd"):
        raise ValueError("need an even and an odd position, and latest even or odd")
    lat, lon = C.c_double(0), C.c_double(0)
    rc = lib().fmd_modes_cpr_global(e["cpr_lat"], e["cpr_lon"], o["cpr_lat"], o["cpr_lon"], int(latest == "odd"), C.byref(lat), C.byref(lon))
    if rc == -7:                                             # FMD_ERR_BAD_STATE
        return None
    check(rc)
    return lat.value, lon.value


def _msg_dict(m):
    return {"k_rel": m.k_rel, "power": m.power, "n_bytes": m.n_bytes, "fixed_bit": m.fixed_bit, "df": m.df, "bytes": bytes(m.bytes)}


class ModeSBank(RecordBank):
    """The Mode S bank (fmd_modes_*): `n_streams` streams of 2 Msample/s u8 IQ.  run takes uint8 [n_streams, nbytes] on the host,
    run_device the same on the device; both return nothing.  Behind a call: counts() uint32 [n_streams], every acceptance of the
    call; messages(streams) the first min(count, msg_cap) records of each listed stream in increasing position, as dicts {"k_rel",
    "power", "n_bytes", "fixed_bit", "df", "bytes"} (k_rel counts from the call's first sample, from -239 upward; bytes is 14 long,
    zero behind n_bytes); info() the streams' cumulative counters."""
    _prefix, _cap, _reader, _record, _info, _as_dict = "modes", "msg_cap", "msgs", ModesMsg, ModesTotals, staticmethod(_msg_dict)
    _passes = 2
    messages = RecordBank.delivered

    def __init__(self, n_streams=1, min_power=0, fix_errors=False, df11=False, msg_cap=32, device_id=-1):
        self.n_streams = self.n_rows = int(n_streams)
        self.min_power, self.fix_errors, self.df11, self.msg_cap = int(min_power), int(fix_errors), int(df11), int(msg_cap)
        for name in ("n_streams", "min_power", "fix_errors", "df11", "msg_cap"):
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        self._h = C.c_void_p()
        cfg = ModesConfig(self.min_power, self.fix_errors, self.df11, self.msg_cap)
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(lib().fmd_modes_new(C.byref(cfg), C.byref(dev), C.byref(self._h)))

    def kernel_name(self, which=0):
        """The kernel of pass `which` (0: the tiles, 1: per stream), as rocprofv3 --kernel-trace prints it."""
        buf = C.create_string_buffer(128)
        check(lib().fmd_modes_kernel_name(self._h, int(which), buf, len(buf)))
        return buf.value.decode()

    def run(self, iq):
        iq = np.ascontiguousarray(iq, dtype=np.uint8)
        if iq.ndim != 2 or iq.shape[0] != self.n_streams:
            raise ValueError("iq must be [n_streams, nbytes]")
        check(lib().fmd_modes_run_batch(self._h, iq.ctypes.data, iq.shape[1], iq.shape[1]))

    def run_device(self, d_iq, nbytes, cap_bytes, stream=None):
        """Enqueue on a device pointer (d_iq [n_streams][cap_bytes], the first nbytes of each stream valid).  `stream` must stay alive
        until the handle's next `run_device` call or `check` has returned (include/fmd.h)."""
        check(lib().fmd_modes_run_device(self._h, d_iq, nbytes, cap_bytes, stream))
