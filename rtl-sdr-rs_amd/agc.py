"""Host-side wrapper of the automatic gain control (include/fmd.h, fmd_agc_*): a block-peak AGC with one block of look-ahead over the
int16 rows a bank leaves on the device -- mono audio at width 1, interleaved (L, R) or (I, Q) under one common gain at width 2 -- so
that strong and weak channels of one bank come out at the same level and none of them clips.  Exact in integers; the output does not
depend on how the stream is cut."""
import ctypes as C

from ._ffi import DeviceConfig, RowProcessor, bank_rows, check, lib


class AgcConfig(C.Structure):
    """struct fmd_agc_config"""
    _fields_ = [("block", C.c_uint32), ("target", C.c_uint32), ("gain_max", C.c_uint32), ("hang", C.c_uint32), ("decay", C.c_uint32)]


class Agc(RowProcessor):
    """`n_rows` is the rows of the bank whose output it takes (n_streams x stations or channels), `width` 1 or 2 int16 per sample.
    |out| <= target; `gain_max` is Q10 (1024: unity), `hang` blocks of `block` samples are held after an attack, then the gain
    closes decay / 256 of its gap per block.  Block j comes out with the call that completes block j + 1: the last block .. 2 block
    - 1 samples of a stream come out only behind 2 block further (zero) samples.  run_batch takes [n_rows, n_in, width] (or
    [n_rows, n_in] at width 1) on the host; run_device takes a bank's d_out as it stands, with the bank's out_cap as in_cap."""
    _prefix = "agc"

    def __init__(self, n_rows=1, width=1, target=12000, block=256, hang=4, decay=32, gain_max=65536, device_id=-1):
        self.n_rows, self.width = int(n_rows), int(width)
        self.target, self.block, self.hang, self.decay, self.gain_max = int(target), int(block), int(hang), int(decay), int(gain_max)
        for name in ("target", "block", "hang", "decay", "gain_max", "n_rows", "width"):
            if not 0 <= getattr(self, name) < 1 << 32:
                raise ValueError("%s out of range" % name)
        self._h = C.c_void_p()
        cfg = AgcConfig(self.block, self.target, self.gain_max, self.hang, self.decay)
        dev = DeviceConfig(self.n_rows, device_id, 0)
        check(lib().fmd_agc_new(C.byref(cfg), self.width, C.byref(dev), C.byref(self._h)))

    def out_cap(self, n_in):
        return int(lib().fmd_agc_out_cap(self.block, n_in))

    def gain(self, row=0):
        """(G, h) of `row` after the last emitted block: the Q10 gain and the hang blocks left.  Synchronises."""
        g, h = C.c_uint32(0), C.c_uint32(0)
        check(self._fn("gain")(self._h, int(row), C.byref(g), C.byref(h)))
        return g.value, h.value


def leveled(bank, target=12000, block=256, hang=4, decay=32, gain_max=65536, device_id=-1):
    """An Agc matched to `bank`: its rows (n_streams x stations or selected channels) and its width."""
    rows, width = bank_rows(bank)
    return Agc(n_rows=rows, width=width, target=target, block=block, hang=hang, decay=decay, gain_max=gain_max, device_id=device_id)
