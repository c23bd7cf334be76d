"""What the GPU tests of the row processors (tests/test_gpu_resample.py, tests/test_gpu_agc.py, tests/test_gpu_tonesq.py and their
*_domain files) share: one run_device call over sentinel-filled device buffers, the same with rows that start at chosen offsets, and
the raw IQ bytes of the banks in front of them."""
import numpy as np

SENT = -12345
TOO_SHORT = -3                                               # FMD_ERR_TOO_SHORT


def call(h, x, in_cap=None, out_pad=2, stream=None):
    """One run_device call over x [rows, n_in, width] in a device buffer of `in_cap` samples per row, into an odd out_cap; the
    outputs [rows, n_out, width].  Nothing beyond them is written.  FmdError when the call is refused."""
    import torch
    rows, n_in, W = x.shape
    in_cap = n_in if in_cap is None else in_cap
    buf = np.full((rows, max(1, in_cap), W), 12321, np.int16)
    buf[:, :n_in] = x
    d_in = torch.from_numpy(buf).cuda()
    cap = (h.out_cap(n_in) + out_pad) | 1
    d_out = torch.full((rows, cap, W), SENT, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    n = h.run_device(d_in.data_ptr(), n_in, in_cap, d_out.data_ptr(), cap, stream)
    h.check()
    got = d_out.cpu().numpy()
    assert (got[:, n:] == SENT).all()
    return got[:, :n]


FILL = 12321


def call_at(h, x, off_in=0, off_out=0, in_place=False, out_pad=2):
    """One run_device call over x [rows, n_in, width] whose input rows start `off_in` samples and whose output rows `off_out` samples
    behind a 16-byte boundary: the device pointers are advanced by that many samples inside larger buffers, and the capacities are
    multiples of 8 samples, so every row has its pointer's offset.  `in_place`: d_out is d_in and out_cap is in_cap (`off_out` is
    not used).  Returns the outputs [rows, n_out, width]; nothing else in either buffer is written."""
    import torch
    rows, n_in, W = x.shape
    in_cap = (n_in + 15) // 8 * 8
    host = np.full((rows * in_cap + 16) * W, FILL, np.int16)
    host[off_in * W:(off_in + rows * in_cap) * W].reshape(rows, in_cap, W)[:, :n_in] = x
    d_in = torch.from_numpy(host).cuda()
    cap = in_cap if in_place else (h.out_cap(n_in) + out_pad + 15) // 8 * 8
    d_out = d_in if in_place else torch.full(((rows * cap + 16) * W,), SENT, dtype=torch.int16, device="cuda")
    off_out = off_in if in_place else off_out
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    n = h.run_device(d_in.data_ptr() + 2 * W * off_in, n_in, in_cap, d_out.data_ptr() + 2 * W * off_out, cap)
    h.check()
    got = d_out.cpu().numpy()
    lo, hi = off_out * W, (off_out + rows * cap) * W
    body = got[lo:hi].reshape(rows, cap, W)
    if in_place:
        assert n == n_in and (body[:, n:] == FILL).all() and (got[:lo] == FILL).all() and (got[hi:] == FILL).all()
    else:
        assert (body[:, n:] == SENT).all() and (got[:lo] == SENT).all() and (got[hi:] == SENT).all()
        assert np.array_equal(d_in.cpu().numpy(), host)
    return body[:, :n].copy()


def iq_bytes(rng, S, n, quiet=False):
    """S streams of n raw IQ bytes: a third of them at the rails; with `quiet`, a quarter of them next to the centre."""
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    b[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)
    if quiet:
        q = slice(n // 2, n // 2 + n // 4)
        b[:, q] = rng.integers(120, 136, (S, b[:, q].shape[1]), dtype=np.uint8)
    return b
