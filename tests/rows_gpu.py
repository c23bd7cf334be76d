"""What the GPU tests of the row processors (tests/test_gpu_resample.py, tests/test_gpu_agc.py) share: one run_device call over
sentinel-filled device buffers, and the raw IQ bytes of the banks in front of them."""
import numpy as np

SENT = -12345


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


def iq_bytes(rng, S, n, quiet=False):
    """S streams of n raw IQ bytes: a third of them at the rails; with `quiet`, a quarter of them next to the centre."""
    b = rng.integers(0, 256, (S, n), dtype=np.uint8)
    b[:, : n // 3] = np.where(rng.random((S, n // 3)) < 0.5, 0, 255)
    if quiet:
        q = slice(n // 2, n // 2 + n // 4)
        b[:, q] = rng.integers(120, 136, (S, b[:, q].shape[1]), dtype=np.uint8)
    return b
