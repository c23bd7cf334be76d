"""Host-side wrapper of the package bank (include/fmd.h, fmd_packages_*): the slicer of pulses.py for every stream of a pulse bank, on
the device.  It takes the pulse records of a call -- from the host, or where a PulseBank left them on the device -- and leaves the PWM
or PPM bit packages that closed in the call, per stream, as PulseSlicer.take gives them."""
import ctypes as C

import numpy as np

from ._ffi import DeviceConfig, RecordBank, check, lib
from .pulses import PulsePackage, PulseRec, PulseSlicerConfig, PulsesTotals, _modulation


class PackagesConfig(C.Structure):
    """struct fmd_packages_config"""
    _fields_ = [("slicer", PulseSlicerConfig), ("min_bits", C.c_uint32), ("pkg_cap", C.c_uint32)]


class PackagesTotals(C.Structure):
    """struct fmd_packages_totals"""
    _fields_ = [("records", C.c_uint64), ("packages", C.c_uint64), ("skipped", C.c_uint64), ("bad", C.c_uint64), ("open", C.c_uint32),
                ("open_pulses", C.c_uint32)]


def packages_max(n_records):
    """The packages a call of n_records records read can close at most."""
    return int(lib().fmd_packages_max(int(n_records)))


def _package_dict(k):
    return {"start": int(k.start), "n_pulses": k.n_pulses, "n_bits": k.n_bits, "bits": bytes(k.bits), "flags": k.flags}


class PackageBank(RecordBank):
    """The package bank (fmd_packages_*): a slicer per stream.  run_batch takes a call's records from the host, run_bank what a
    PulseBank's last call left on the device, flush ends the input; all return nothing.  Behind a call: counts() uint32 [n_streams],
    every delivered package that closed in the call; packages(streams) the first min(count, pkg_cap) of each listed stream as dicts
    {"start", "n_pulses", "n_bits", "bits" (32 bytes, MSB first), "flags"}; info() the streams' cumulative counters {"records",
    "packages", "skipped", "bad", "open", "open_pulses"}."""
    _prefix, _cap, _reader, _record, _info, _as_dict = "packages", "pkg_cap", "pkgs", PulsePackage, PackagesTotals, staticmethod(_package_dict)
    packages = RecordBank.delivered

    def __init__(self, n_streams, modulation, short, long, tol, reset, min_bits=0, pkg_cap=1025, device_id=-1):
        self.n_streams = self.n_rows = int(n_streams)
        self.modulation = _modulation(modulation)
        self.short, self.long, self.tol, self.reset_gap = int(short), int(long), int(tol), int(reset)
        self.min_bits, self.pkg_cap = int(min_bits), int(pkg_cap)
        for name in ("n_streams", "short", "long", "tol", "reset_gap", "min_bits", "pkg_cap"):
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        self._h = C.c_void_p()
        cfg = PackagesConfig(PulseSlicerConfig(self.modulation, self.short, self.long, self.tol, self.reset_gap), self.min_bits, self.pkg_cap)
        dev = DeviceConfig(self.n_streams, device_id, 0)
        check(lib().fmd_packages_new(C.byref(cfg), C.byref(dev), C.byref(self._h)))

    def run_batch(self, counts, recs, totals, n_samples):
        """counts: uint32 [n_streams]; recs: per stream a list of record dicts as PulseBank.pulses gives them (rec_cap is the longest
        list, at least 1), or a numpy array [n_streams, rec_cap, 4] of int32 / uint32 dwords; totals: per stream a dict with "samples",
        "state" and "run" as PulseBank.info gives them; n_samples: the samples per stream of the call that left them."""
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        if isinstance(recs, np.ndarray):
            raw = np.ascontiguousarray(recs).view(np.uint32)
            if raw.ndim != 3 or raw.shape[0] != self.n_streams or raw.shape[2] != 4:
                raise ValueError("recs must be [n_streams, rec_cap, 4]")
        else:
            cap = max([1] + [len(r) for r in recs])
            raw = np.zeros((self.n_streams, cap, 4), np.uint32)
            for s, row in enumerate(recs):
                for k, r in enumerate(row):
                    raw[s, k] = (r["k_rel"] & 0xFFFFFFFF, r["width"], r["gap"], r.get("level", 0))
        if counts.shape[0] != self.n_streams or len(totals) != self.n_streams:
            raise ValueError("counts, recs and totals must have n_streams entries")
        tot = (PulsesTotals * self.n_streams)(*[PulsesTotals(t["samples"], t.get("pulses", 0), t.get("rises", 0), t["state"], 0, t["run"]) for t in totals])
        check(lib().fmd_packages_run_batch(self._h, counts.ctypes.data, raw.ctypes.data, raw.shape[1], tot, int(n_samples)))

    def run_bank(self, bank, stream=None):
        """Enqueue on what `bank` (a PulseBank with the same n_streams on the same device) left on the device in its last call that
        launched; nothing visits the host.  `stream` must stay alive until the handle's next call or `check` has returned."""
        check(lib().fmd_packages_run_bank(self._h, bank._h, stream))

    def flush(self, stream=None):
        """The end of the input: a call of no records that closes every open package."""
        check(lib().fmd_packages_flush(self._h, stream))


def sliced(bank, modulation, short, long, tol, reset, min_bits=0, pkg_cap=None, device_id=-1):
    """A PackageBank matched to the PulseBank `bank`: its n_streams, and room for every package a call of it can close (pkg_cap
    defaults to min(1025, pulse_cap + 1))."""
    if pkg_cap is None:
        pkg_cap = min(1025, bank.pulse_cap + 1)
    return PackageBank(bank.n_streams, modulation, short, long, tol, reset, min_bits, pkg_cap, device_id)
