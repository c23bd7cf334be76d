"""The FIR bank and the fused FIR-demod bank on the handle core that every later handle uses (csrc/fmd_ddc.h), on the MI355X: three
FIR banks -- one tap (no history), the matrix-core form with two tap digits, the vector-pipe kernel with its separate history
kernel --, two fused banks (the LDS-array kernel and a register form) and a station bank, which shares the core, alive at once.  Each
is checked bit for bit against the oracle of tests/test_fir.py and tests/test_firdemod.py while the others run, are reset, refuse a
call and are freed around it; then the `_device` entries on alternating streams, the growth of the batch staging buffers, the fused
bank's completion point, state and checkpoints, and which of two wrong arguments answers."""
import ctypes as C

import numpy as np
import pytest

import stations_ref as sr

pytestmark = pytest.mark.gpu

INVALID_ARG, BAD_LENGTH, TOO_SHORT, BAD_RATES, CAPACITY, UNSUPPORTED, BAD_STATE = -1, -2, -3, -4, -5, -6, -7
NCH = 3
CUTS = (8 * 601, 8 * 513, 8 * 389)                            # 2404 + 2052 + 1556 samples per channel


def _taps(rng, n, lim):
    h = rng.integers(-lim, lim + 1, n).astype(np.int16)
    h[0] = lim                                                # (the extreme itself: |tap| > 127 asks for two digits)
    return h


def _cuts(rng, sizes=CUTS):
    data = rng.integers(0, 256, (NCH, sum(sizes)), dtype=np.uint8)
    return data, [np.ascontiguousarray(c) for c in np.split(data, np.cumsum(sizes)[:-1], axis=1)]


def _state(s):
    return (s["now_lpr"], s["prev_lpr_index"], s["demod_pre"])


class Under:
    """A FirBank, or with `rates` a FirDemodBank, and the oracle's instance of each of its channels."""

    def __init__(self, fmd, oracle, taps, decim, rates=None):
        self.o, self.taps, self.decim, self.rates = oracle, taps, decim, rates
        self.bank = fmd.FirDemodBank(taps, decim, rates[0], rates[1], NCH, device_id=0) if rates else fmd.FirBank(taps, decim, NCH, device_id=0)
        self.refs = []
        self.fresh_refs()

    def fresh_refs(self):
        self.drop_refs()
        if self.rates:
            self.refs = [self.o.firdemod_new(self.taps, self.decim, self.bank.shift, *self.rates) for _ in range(NCH)]
        else:
            self.refs = [self.o.fir_new(self.taps, self.decim) for _ in range(NCH)]

    def drop_refs(self):
        for h in self.refs:
            (self.o.lib.fmo_firdemod_free if self.rates else self.o.lib.fmo_fir_free)(h)
        self.refs = []

    def expect(self, cut):
        return [(self.o.firdemod if self.rates else self.o.fir_filter)(h, cut[c]) for c, h in enumerate(self.refs)]

    def agrees(self, got, exp):
        ok = all(got[c].shape == exp[c].shape and np.array_equal(got[c], exp[c]) for c in range(NCH))
        if self.rates:                                        # the fused bank's completion point and carried state, after every call
            self.bank.check()
            ok = ok and all(_state(self.bank.get_state(c).as_dict()) == _state(self.o.firdemod_state(self.refs[c])) for c in range(NCH))
        return ok

    def step(self, cut, at_least=1):
        """one host call against the oracle"""
        exp = self.expect(cut)
        got = self.bank.demodulate_batch(cut) if self.rates else self.bank.filter_batch(cut)
        assert len(exp[0]) >= at_least and self.agrees(got, exp), (self.taps.size, self.decim, self.rates)
        return got

    def device(self, d_iq, nbytes, d_out, cap, stream=None):
        run = self.bank.demodulate_device if self.rates else self.bank.filter_device
        return run(d_iq.data_ptr(), nbytes, d_out.data_ptr(), cap, stream)

    def d_out(self, nbytes):
        import torch
        cap = self.bank.out_cap(nbytes)
        shape, dt = ((NCH, cap), torch.int16) if self.rates else ((NCH, cap, 2), torch.int32)
        return torch.zeros(shape, dtype=dt, device="cuda"), cap

    def close(self):
        self.bank.close()
        self.drop_refs()


SHAPES = {"one": (1, 2, None),                                # one tap: no history
          "mfma": (33, 4, None),                              # matrix-core form, two digits
          "valu": (5, 130, None),                             # vector-pipe kernel + history kernel
          "fd": (33, 4, (250000, 48000)),                     # LDS-array kernel
          "reg": (127, 8, (2500000, 48000))}                  # register form


def _make(fmd, oracle, kind):
    """a fresh handle of one of this file's shapes (the same taps every time)"""
    T, M, rates = SHAPES[kind]
    return Under(fmd, oracle, _taps(np.random.default_rng(100 * T + M), T, 900), M, rates)


def _fir_count(T, M, samples):
    return (samples - T) // M + 1 if samples >= T else 0


def test_fir_fused_and_station_handles_interleaved_reset_refusal_and_free(fmd, oracle):
    import torch
    rng = np.random.default_rng(2024)
    data, cuts = _cuts(rng)
    u = {k: _make(fmd, oracle, k) for k in SHAPES}
    assert u["one"].bank.kernel_name().endswith(", false, 2>") and u["one"].bank.tap_digits() == 2
    assert u["mfma"].bank.kernel_name().endswith(", false, 2>") and u["mfma"].bank.tap_digits() == 2
    assert u["valu"].bank.kernel_name().endswith("fmd_fir_kernel") and u["valu"].bank.tap_digits() == 0
    assert u["fd"].bank.kernel_name().endswith("fmd_firdemod_kernel<2, 0>")
    assert "fmd_firdemod_reg" in u["reg"].bank.kernel_name()
    # the station bank: 2 stations out of each of the 3 streams, 4 filter outputs per audio sample
    h = _taps(rng, 33, 900)
    incs = np.array([[int(x) for x in rng.integers(0, 1 << 32, 2)] for _ in range(NCH)], np.uint32)
    sb = fmd.StationBank(h, 4, incs, 120000, 30000, n_streams=NCH, device_id=0)
    sref = [sr.StationsRef(oracle, h, 4, incs[s], 120000, 30000, sb.shift, z=sr.z_corr) for s in range(NCH)]

    def stations(cut):
        exp = [sref[s].feed(cut[s]) for s in range(NCH)]
        got = sb.demodulate_batch(cut)
        assert got.shape[2] == len(exp[0][0]) >= 1 and all(np.array_equal(got[s, k], exp[s][k]) for s in range(NCH) for k in range(2))

    # cut 1, the handles interleaved call by call
    first = {k: u[k].step(cuts[0]) for k in ("one", "mfma", "fd", "valu", "reg")}
    stations(cuts[0])

    # one of each kind back to the start: they reproduce their first outputs, the others continue unbroken
    u["mfma"].bank.reset()
    u["reg"].bank.reset()
    u["mfma"].fresh_refs()
    u["reg"].fresh_refs()
    u["one"].step(cuts[1])
    again = u["mfma"].step(cuts[0])
    assert all(np.array_equal(again[c], first["mfma"][c]) for c in range(NCH))
    u["fd"].step(cuts[1])
    again = u["reg"].step(cuts[0])
    assert all(np.array_equal(again[c], first["reg"][c]) for c in range(NCH))
    u["valu"].step(cuts[1])
    stations(cuts[1])

    # refused calls of each kind between good ones: 12 bytes; 8 bytes, which are 4 samples and at most one filter output; room for
    # one output per channel where the call completes more, through the `_device` entries
    d_iq = torch.from_numpy(cuts[1]).cuda()
    for k in SHAPES:
        with pytest.raises(fmd.FmdError) as e:
            (u[k].bank.demodulate_batch if u[k].rates else u[k].bank.filter_batch)(data[:, :12])
        assert e.value.status == BAD_LENGTH, k
        if u[k].rates:
            with pytest.raises(fmd.FmdError) as e:
                u[k].bank.demodulate_batch(data[:, :8])
            assert e.value.status == TOO_SHORT, k
        d_out, _ = u[k].d_out(CUTS[1])
        with pytest.raises(fmd.FmdError) as e:
            u[k].device(d_iq, CUTS[1], d_out, 1)
        assert e.value.status == CAPACITY, k
        torch.cuda.synchronize()
        assert not d_out.any()
    u["mfma"].step(cuts[1], at_least=2)
    u["reg"].step(cuts[1], at_least=2)

    for k in ("reg", "one", "fd", "valu", "mfma"):
        u[k].step(cuts[2], at_least=2)
    stations(cuts[2])

    # freed in another order than created; handles created afterwards start clean
    sb.close()
    for k in ("fd", "one", "reg", "valu", "mfma"):
        u[k].close()
    for k in ("mfma", "reg"):
        v = _make(fmd, oracle, k)
        again = v.step(cuts[0])
        assert all(np.array_equal(again[c], first[k][c]) for c in range(NCH))
        v.close()


@pytest.mark.parametrize("kind", list(SHAPES))
def test_device_entries_on_alternating_streams_equal_the_single_stream_run(fmd, oracle, kind):
    """Three calls on two streams in turn: every launch reads the history (and the channel state) its predecessor wrote on the
    other stream.  The twin handle takes the same calls on one stream."""
    import torch
    _, cuts = _cuts(np.random.default_rng(31))
    a, b = _make(fmd, oracle, kind), _make(fmd, oracle, kind)
    d_iqs = [torch.from_numpy(c).cuda() for c in cuts]
    outs = {h: [h.d_out(n) for n in CUTS] for h in (a, b)}
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    ns = {h: [] for h in (a, b)}
    for i, n in enumerate(CUTS):
        ns[a].append(a.device(d_iqs[i], n, outs[a][i][0], outs[a][i][1], streams[i % 2].cuda_stream))
        ns[b].append(b.device(d_iqs[i], n, outs[b][i][0], outs[b][i][1], streams[0].cuda_stream))
    if a.rates:
        a.bank.check()
        b.bank.check()
    torch.cuda.synchronize()
    for i, cut in enumerate(cuts):
        exp = a.expect(cut)
        ga, gb = outs[a][i][0].cpu().numpy(), outs[b][i][0].cpu().numpy()
        assert ns[a][i] == ns[b][i] == len(exp[0]) >= 1 and np.array_equal(ga, gb)
        assert all(np.array_equal(ga[c, :ns[a][i]], exp[c]) for c in range(NCH)), (kind, i)
    a.close()
    b.close()


def test_batch_staging_grows_and_is_kept(fmd, oracle):
    """A small call, a larger one, the small size again: the staging buffers grow once and then serve the smaller call.  80 bytes are
    40 samples: two outputs of the 33-tap filter at decimation 4 in rows of out_cap 12 (the strided copy back), then ten (the
    linear one); the fused bank's first call completes no audio sample and copies nothing back."""
    sizes = (80, 8 * 2000, 80)
    _, cuts = _cuts(np.random.default_rng(77), sizes)
    for k in ("mfma", "fd", "valu"):
        u = _make(fmd, oracle, k)
        seen, lens = 0, []
        for n, cut in zip(sizes, cuts):
            lens.append(u.step(cut, at_least=0)[0].shape[0])
            if k == "mfma":
                assert lens[-1] == _fir_count(33, 4, seen + n // 2) - _fir_count(33, 4, seen) and (n > 80 or u.bank.out_cap(n) == 12)
            seen += n // 2
        assert lens == [2, 2000, 10] if k == "mfma" else lens[0] == 0 < lens[2] if k == "fd" else min(lens) >= 1
        u.close()


@pytest.mark.parametrize("kind", ["fd", "reg"])
def test_fused_checkpoint_resume_and_a_damaged_blob(fmd, oracle, kind):
    _, cuts = _cuts(np.random.default_rng(55))
    a = _make(fmd, oracle, kind)
    a.step(cuts[0])
    blob = a.bank.checkpoint()
    later = [a.step(cuts[1]), a.step(cuts[2])]
    assert a.bank.f64_stats()["patched"] <= a.bank.f64_stats()["guarded"]
    b = _make(fmd, oracle, kind)                              # a fresh one: never called
    for h in (a, b):
        h.bank.resume(blob)
        h.bank.check()
        for i in (1, 2):
            got = h.bank.demodulate_batch(cuts[i])
            h.bank.check()
            assert all(np.array_equal(got[c], later[i - 1][c]) for c in range(NCH)), (kind, i)
        assert all(_state(h.bank.get_state(c).as_dict()) == _state(oracle.firdemod_state(a.refs[c])) for c in range(NCH))
    # one flipped byte, in the header, in a channel's state, in the history: refused, and the handle carries on
    for at in (20, 64 + 21, len(blob) - 1):
        bad = bytearray(blob)
        bad[at] ^= 0x10
        with pytest.raises(fmd.FmdError) as e:
            a.bank.resume(bytes(bad))
        assert e.value.status == BAD_STATE, at
    a.step(cuts[0])                                           # (the oracle's instances have seen cuts 1 - 3)
    a.close()
    b.close()


def _fir_new(fmd, taps, decim, n_channels):
    h, dev = C.c_void_p(), fmd.DeviceConfig(n_channels, 0, 0)
    taps = np.ascontiguousarray(taps, np.int16)
    rc = fmd.lib().fmd_fir_new(taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, decim, C.byref(dev), C.byref(h))
    if rc == 0:
        fmd.lib().fmd_fir_free(h)
    return rc, fmd.lib().fmd_last_error().decode()


def _firdemod_new(fmd, taps, decim, shift, fast, slow, n_channels):
    h, dev = C.c_void_p(), fmd.DeviceConfig(n_channels, 0, 0)
    taps = np.ascontiguousarray(taps, np.int16)
    rc = fmd.lib().fmd_firdemod_new(taps.ctypes.data_as(C.POINTER(C.c_int16)), taps.size, decim, shift, fast, slow, C.byref(dev), C.byref(h))
    if rc == 0:
        fmd.lib().fmd_firdemod_free(h)
    return rc, fmd.lib().fmd_last_error().decode()


ONES, WIDE, LOUD = np.ones(8, np.int16), np.full(8, 2048, np.int16), np.full(1024, 2047, np.int16)
# (constructor, arguments, status, text): two wrong arguments each, and the one that answers
NEW_REFUSALS = [
    ("fir", (ONES, 3, 0), INVALID_ARG, "null / empty argument"),                    # no channels, odd decimation
    ("fir", (WIDE, 3, 1), UNSUPPORTED, "need 1 <= n_taps <= 1024"),                 # odd decimation, |tap| > 2047
    ("fir", (WIDE, 4098, 1), UNSUPPORTED, "need 1 <= n_taps <= 1024"),              # decimation > 4096, |tap| > 2047
    ("fir", (WIDE, 2, 1), UNSUPPORTED, "|tap| > 2047"),
    ("firdemod", (ONES, 3, 0, 48000, 48000, 0), INVALID_ARG, "null / empty argument"),      # no channels, odd decimation
    ("firdemod", (ONES, 66, 0, 32000, 48000, 1), UNSUPPORTED, "need 1 <= n_taps <= 1024"),  # decimation > 64, rate_out < rate_resample
    ("firdemod", (ONES, 4, 25, 48000, 0, 1), UNSUPPORTED, "need 1 <= n_taps <= 1024"),      # shift > 24, rate_resample 0
    ("firdemod", (WIDE, 4, 0, 32000, 48000, 1), BAD_RATES, "rate_out >= rate_resample"),    # rate_out < rate_resample, |tap| > 2047
    ("firdemod", (np.concatenate([LOUD[:7], WIDE[:1]]), 4, 0, 48000, 48000, 1), UNSUPPORTED, "|tap| > 2047"),   # |tap| > 2047 behind a gain too large
    ("firdemod", (LOUD, 64, 0, 48000 * 600, 48000, 1), UNSUPPORTED, "filter gain too large"),   # gain too large, rate ratio out of range
    ("firdemod", (ONES, 64, 0, 48000 * 600, 48000, 1), UNSUPPORTED, "rate ratio outside"),      # rate ratio out of range, no audio sample per tile
    ("firdemod", (ONES, 64, 0, 48000 * 500, 48000, 1), UNSUPPORTED, "one audio sample does not fit a tile"),
]


@pytest.mark.parametrize("kind,args,status,text", NEW_REFUSALS, ids=["%s-%d" % (c[0], i) for i, c in enumerate(NEW_REFUSALS)])
def test_the_order_of_constructor_refusals(fmd, kind, args, status, text):
    rc, err = (_fir_new if kind == "fir" else _firdemod_new)(fmd, *args)
    assert rc == status and text in err, (rc, err)


BIG = (1 << 31) + 8
# (handle, null d_out, byte offset of d_iq, nbytes, out_cap, status, text) over a buffer of 3 x 4808 bytes on a fresh handle: two wrong
# arguments each, and the one that answers.  (None: the host entry.)
CALL_REFUSALS = [(k,) + c for k in ("mfma", "fd") for c in [
    (True, 0, 12, 0, INVALID_ARG, "null argument"),
    (False, 1, 12, 0, BAD_LENGTH, "nbytes % 8 != 0"),
    (False, 1, 0, 0, UNSUPPORTED, "nbytes out of range"),
    (False, 1, BIG, 0, UNSUPPORTED, "nbytes out of range"),
    (False, 1, 4808, 0, INVALID_ARG, "misaligned device buffer"),
    (False, 0, 4808, 0, CAPACITY, "out_cap too small"),
    (False, None, 12, 0, BAD_LENGTH, "nbytes % 8 != 0"),
]] + [
    ("fd", False, 2, 8, 0, INVALID_ARG, "misaligned device buffer"),                # misaligned, too short
    ("fd", False, 0, 8, 0, TOO_SHORT, "fewer than 2 filter outputs"),               # too short, no room
    ("fd", False, None, 8, 0, TOO_SHORT, "fewer than 2 filter outputs"),
]


@pytest.mark.parametrize("kind,null_out,off,nbytes,out_cap,status,text", CALL_REFUSALS,
                         ids=["%s-%d" % (c[0], i) for i, c in enumerate(CALL_REFUSALS)])
def test_the_order_of_call_refusals_and_what_they_leave(fmd, oracle, kind, null_out, off, nbytes, out_cap, status, text):
    """Where two checks refuse a call the first one answers -- the pointers, the length, its range, the alignment, what the call
    completes, out_cap -- and a refused call writes nothing and takes nothing: the next call is the stream's first."""
    import torch
    _, cuts = _cuts(np.random.default_rng(99))
    u = _make(fmd, oracle, kind)
    d_iq = torch.from_numpy(cuts[0]).cuda()
    d_out, _ = u.d_out(CUTS[0])
    torch.cuda.synchronize()
    with pytest.raises(fmd.FmdError) as e:
        if off is None:
            lens = (C.c_size_t * NCH)()
            host = np.zeros(d_out.shape, np.int16 if u.rates else np.int32)
            run = fmd.lib().fmd_firdemod_demodulate_batch if u.rates else fmd.lib().fmd_fir_filter_batch
            fmd.check(run(u.bank._h, cuts[0].ctypes.data, nbytes, host.ctypes.data, out_cap, lens))
        else:
            run = u.bank.demodulate_device if u.rates else u.bank.filter_device
            run(d_iq.data_ptr() + off, nbytes, None if null_out else d_out.data_ptr(), out_cap)
    assert e.value.status == status and text in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert not d_out.any()
    u.step(cuts[0])
    u.close()
