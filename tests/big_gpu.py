"""What the GPU tests beyond the 2 GiB and 4 GiB lines share (tests/test_gpu_big_rows.py, tests/test_gpu_big_banks.py, tests/test_gpu_big_demod.py): one pitched
device buffer per case (tests/big_cases.py: Geo) that is allocated but never filled as a whole, with the pointer handed to the
library a front margin inside it; its windows filled with decoy input or sentinel; the live rows put into them; and the windows
read back after the call.  A host mirror of the windows is kept, so one comparison per call shows that the outputs are the
reference's, that every sentinel around them is intact (the 64 elements on each side of every live output and everything behind
n_out included), or that an input buffer is unchanged.  And for the inputs that have no pitch, and so are really 2^32 bytes and
more: the check of the free memory, the random fill on the device, the rows that are compared, the sentinel behind the outputs."""
import numpy as np
import pytest

import big_cases as bc


class Pitched:
    def __init__(self, geo, peak, kind, seed):
        """`kind`: "decoy" (valid random int16 that differ from any live row's) or "sentinel"."""
        import torch
        need(torch, peak)
        self.geo, self.torch = geo, torch
        self.buf = torch.empty(geo.size, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0 and geo.margin % 256 == 0
        self.ptr = self.buf.data_ptr() + geo.margin
        rng = np.random.default_rng([seed, 77])
        self.mirror = {}
        for lo, hi in geo.windows():
            assert lo % 2 == 0 and hi % 2 == 0
            n = (hi - lo) // 2
            w = rng.integers(-32768, 32768, n).astype(np.int16) if kind == "decoy" else np.full(n, bc.SENT, np.int16)
            self.mirror[(lo, hi)] = w
            self._write(lo, w)
        torch.cuda.synchronize()

    def _view(self, lo, hi):
        return self.buf[self.geo.margin + lo:self.geo.margin + hi]

    def _write(self, lo, w):
        self._view(lo, lo + 2 * w.size).copy_(self.torch.from_numpy(w.view(np.uint8)).cuda())

    def _window(self, off, nbytes):
        for (lo, hi), w in self.mirror.items():
            if lo <= off and off + nbytes <= hi:
                return lo, w
        raise AssertionError("bytes %d ... %d are in no window" % (off, off + nbytes))

    def put(self, r, x, device=True):
        """Row r's first elements := x (int16 [n] or [n, width], or int32, whose bytes are taken as they are); `device` False: into
        the mirror only (what a call must have written)."""
        x = np.ascontiguousarray(x)
        assert x.dtype in (np.int16, np.int32)
        x = x.view(np.int16).reshape(-1)
        off = self.geo.base(r)
        lo, w = self._window(off, 2 * x.size)
        w[(off - lo) // 2:(off - lo) // 2 + x.size] = x
        if device:
            self._write(off, x)

    def clear(self, value=bc.SENT):
        """Every window back to the sentinel, on the device and in the mirror."""
        for (lo, hi), w in self.mirror.items():
            w[:] = value
            self._write(lo, w)

    def row(self, r, n, width=1):
        """The first n elements of row r as the device holds them."""
        off = self.geo.base(r)
        got = self._view(off, off + 2 * n * width).cpu().numpy().view(np.int16)
        return got.reshape(n, width) if width > 1 else got

    def check(self, what):
        """Every window on the device is what the mirror says."""
        self.torch.cuda.synchronize()
        for (lo, hi), w in self.mirror.items():
            got = self._view(lo, hi).cpu().numpy().view(np.int16)
            if not np.array_equal(got, w):
                bad = np.nonzero(got != w)[0]
                raise AssertionError("%s: %d of %d int16 of the window at bytes %d ... %d differ, first at byte %d (row pitch %d): device %d, expected %d" % (
                    what, bad.size, w.size, lo, hi, lo + 2 * bad[0], self.geo.pitch, got[bad[0]], w[bad[0]]))

    def release(self):
        self.buf = None
        self.mirror = {}
        self.torch.cuda.empty_cache()


# ---- inputs without a pitch: the data is really there ----------------------------------------------------------------------------

def need(torch, peak):
    """Skips the test where it needs more device memory than is free."""
    free, _ = torch.cuda.mem_get_info()
    if peak > free:
        pytest.skip("needs %.1f GiB of device memory, %.1f GiB are free" % (peak / bc.GiB, free / bc.GiB))


def random_bytes(torch, d_iq, seed):
    """Fills the whole device buffer with random bytes, on the device, a GiB at a time."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    flat = d_iq.view(-1)
    step = 1 << 30
    for lo in range(0, flat.numel(), step):
        n = min(step, flat.numel() - lo)
        flat[lo:lo + n] = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)


def rows_of(torch, d, picks):
    """The rows `picks` of a device array on the host, row by row (plain slices, whatever the array's size)."""
    return torch.stack([d[c] for c in picks]).cpu().numpy()


def rest_is_sentinel(torch, d_out, lens):
    """Behind every row's length the output still holds the sentinel (d_out [rows, cap, ...], lens one length per row)."""
    rows, cap = d_out.shape[0], d_out.shape[1]
    lens = torch.as_tensor(lens, device="cuda").to(torch.int64)
    live = torch.arange(cap, device="cuda")[None, :] < lens[:, None]
    return bool(((d_out.reshape(rows, cap, -1) == bc.SENT) | live[:, :, None]).all())
