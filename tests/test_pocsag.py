"""POCSAG batch decoder (include/fmd.h, fmd_pocsag_decoder_*) without a GPU: the C++ decoder against tests/pocsag_ref.py message for
message and counter for counter, the code, the text functions in C++ and Python, the behaviour of the two definitions (tests/fsk_ref.py
in front of tests/pocsag_ref.py) over twelve (rate, baud) pairs, the fuzz program under the sanitizers, and pocsag_gpu's arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fsk_ref as fr
import pocsag_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rtl-sdr-rs_amd")
CLI = os.path.join(PKG, "pocsag_gpu")
INVALID_ARG, UNSUPPORTED, NO_DEVICE = -1, -6, -8
SYMBOLS = ["new", "free", "reset", "push", "info"]
PAIRS = [(9600, 1200), (11025, 1200), (12000, 512), (12000, 1200), (12000, 2400), (16000, 1200), (22050, 2400), (24000, 512),
         (24000, 1200), (25600, 2400), (48000, 512), (48000, 2400)]


def test_every_symbol_is_declared_exported_and_bound(fmd):
    from rtl_sdr_rs_amd import _ffi, pocsag
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmd.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(fmd_pocsag_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(["fmd_pocsag_decoder_" + s for s in SYMBOLS] + ["fmd_pocsag_correct"])
    for name in declared:
        assert name in _ffi.PROTOTYPES and hasattr(fmd.lib(), name), name
    for name in ("PocsagDecoder", "pocsag_text", "pocsag_numeric", "pocsag_alpha", "pocsag_encode", "decode_pages", "pages"):
        assert callable(getattr(fmd, name)), name
    assert fmd.lib().fmd_version() == 3
    assert C.sizeof(pocsag.PocsagMsg) == 352 and pocsag.PocsagMsg.end_sample.offset == 344 and pocsag.PocsagMsg.bits.offset == 12
    assert C.sizeof(pocsag.PocsagInfo) == 40 and C.sizeof(pocsag.FskHit) == 16 == pocsag.HIT_DTYPE.itemsize


def test_null_arguments_and_the_domain(fmd):
    lib, h, n = fmd.lib(), C.c_void_p(), C.c_size_t(0)
    assert lib.fmd_pocsag_decoder_new(2400, 1, 1200, 1, None) == INVALID_ARG
    assert lib.fmd_pocsag_decoder_reset(None) == INVALID_ARG and lib.fmd_pocsag_decoder_info(None, None) == INVALID_ARG
    assert lib.fmd_pocsag_decoder_push(None, None, 0, None, 0, None, 0, C.byref(n)) == INVALID_ARG
    lib.fmd_pocsag_decoder_free(None)
    rate = "need 2 <= rate / baud <= 32"
    for args, text in (((2399, 1, 1200, 1), rate), ((38401, 1, 1200, 1), rate), ((4800, 0, 1200, 1), rate), ((4800, 1, 0, 1), rate),
                       ((0, 1 << 31, 1 << 31, 1), rate), ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 1), rate),
                       ((6000, 1, 1200, 3), "need max_errors <= 2")):
        assert lib.fmd_pocsag_decoder_new(*args, C.byref(h)) == UNSUPPORTED and not h.value, args
        assert lib.fmd_last_error().decode() == text
    for args in ((2400, 1, 1200, 0), (38400, 1, 1200, 2), (0xFFFFFFFF, 0xFFFFFFFF // 2400, 1200, 1), (11025, 2, 1200, 1)):
        assert lib.fmd_pocsag_decoder_new(*args, C.byref(h)) == 0 and h.value, args
        one = np.zeros(1, np.int16)
        assert lib.fmd_pocsag_decoder_push(h, None, 1, None, 0, None, 0, C.byref(n)) == INVALID_ARG
        assert lib.fmd_pocsag_decoder_push(h, one.ctypes.data, 1, None, 1, None, 0, C.byref(n)) == INVALID_ARG
        assert lib.fmd_pocsag_decoder_push(h, one.ctypes.data, 1, None, 0, None, 1, C.byref(n)) == INVALID_ARG
        assert lib.fmd_pocsag_decoder_push(h, one.ctypes.data, 1, None, 0, None, 0, None) == INVALID_ARG
        lib.fmd_pocsag_decoder_free(h)
        h = C.c_void_p()


# ---- the code --------------------------------------------------------------------------------------------------------------------
def test_sync_and_idle_are_valid_codewords_and_the_encoder_makes_them(fmd):
    from rtl_sdr_rs_amd import pocsag
    assert pr.valid(0x7CD215D8) and pr.valid(0x7A89C197) and pocsag.pocsag_valid(0x7CD215D8) and pocsag.pocsag_valid(0x7A89C197)
    assert pocsag.pocsag_codeword(0x7CD215D8 >> 11) == 0x7CD215D8 and pocsag.pocsag_codeword(0x7A89C197 >> 11) == 0x7A89C197
    assert pocsag.pocsag_correct(0x7CD215D8, 0) == (0x7CD215D8, 0) and pocsag.pocsag_correct(0x7A89C197 ^ 1, 0) is None
    rng = np.random.default_rng(1)
    words = [pocsag.pocsag_codeword(int(v)) for v in rng.integers(0, 1 << 21, 200)]
    assert all(pr.valid(w) for w in words)
    dist = min(bin(a ^ b).count("1") for i, a in enumerate(words) for b in words[:i] if a != b)
    assert dist >= 6                                         # (the code's minimum distance)


def test_correction_of_every_single_and_double_flip_and_no_triple_flip_back_to_what_was_sent(fmd):
    from rtl_sdr_rs_amd import pocsag
    rng = np.random.default_rng(2)
    cw = pocsag.pocsag_codeword(int(rng.integers(0, 1 << 21)))
    for a in range(32):
        w = cw ^ (1 << a)
        assert pocsag.pocsag_correct(w, 0) is None and pr.correct(w, 0) is None
        assert pocsag.pocsag_correct(w, 1) == (cw, 1) == pr.correct(w, 1) and pocsag.pocsag_correct(w, 2) == (cw, 1)
        for b in range(a + 1, 32):
            w2 = w ^ (1 << b)
            assert pocsag.pocsag_correct(w2, 0) is None and pocsag.pocsag_correct(w2, 1) is None
            assert pocsag.pocsag_correct(w2, 2) == (cw, 2)
    assert pr.correct(cw ^ 0x81, 1) is None and pr.correct(cw ^ 0x81, 2) == (cw, 2)
    for _ in range(600):                                     # three flips: some other codeword or none, never the one that was sent
        a, b, c = rng.choice(32, 3, replace=False)
        w3 = cw ^ (1 << int(a)) ^ (1 << int(b)) ^ (1 << int(c))
        for e in (0, 1, 2):
            got = pocsag.pocsag_correct(w3, e)
            assert got is None or got[0] != cw
            assert got == pr.correct(w3, e)
    with pytest.raises(fmd.FmdError):
        pocsag.pocsag_correct(cw, 3)


# ---- decoder against the definition ------------------------------------------------------------------------------------------------
SPB = 5


def _soft(bits, amp=3000, dc=0, invert=False, spb=SPB, lead=40, tail=None):
    """soft decisions at `spb` per bit and the records of the sync words in them (the middle sample of a sync word's last bit)"""
    from rtl_sdr_rs_amd import pocsag
    bits = np.asarray(bits, np.int64)
    tail = 40 * spb if tail is None else tail
    lvl = np.where(bits == 1, amp, -amp) * (-1 if invert else 1) + dc
    soft = np.concatenate([np.full(lead, dc), np.repeat(lvl, spb), np.full(tail, dc)]).astype(np.int16)
    sync = [(pocsag.POCSAG_SYNC >> b) & 1 for b in range(31, -1, -1)]
    hits = []
    for i in range(len(bits) - 31):
        if bits[i:i + 32].tolist() == sync:
            hits.append((lead + (i + 31) * spb + spb // 2, 32 | 1 << 31 if invert else 0, (-32 if invert else 32) * amp, 32 * dc))
    return soft, hits


def _both(fmd, soft, hits, cuts=None, max_errors=1, spb=SPB, cap=None):
    """C++ and definition over the same pushes; returns (messages, info) after asserting they agree"""
    from rtl_sdr_rs_amd import pocsag
    dec, ref = fmd.PocsagDecoder(1200 * spb, 1, 1200, max_errors), pr.Decoder(1200 * spb, 1, 1200, max_errors)
    cuts = [len(soft)] if cuts is None else cuts
    got, want, lo = [], [], 0
    for n in cuts:
        n = min(n, len(soft) - lo)
        h = [(k - lo, d, c, t) for k, d, c, t in hits if lo <= k < lo + n]
        got += dec.push(soft[lo:lo + n], np.array(h, pocsag.HIT_DTYPE))
        want += ref.push(soft[lo:lo + n], h)
        lo += n
    assert lo == len(soft)
    assert got == want and dec.info() == ref.info()
    return got, dec.info()


def test_address_and_frame_arithmetic_for_all_eight_frames(fmd):
    for frame in range(8):
        address = (0x2A5A5 << 3 | frame) & 0x1FFFFF
        for function in range(4):
            soft, hits = _soft(fmd.pocsag_encode([(address, function, "", "tone")], preamble=64))
            msgs, info = _both(fmd, soft, hits)
            assert [(m["address"], m["function"], m["n_bits"], m["inverted"], m["corrected"]) for m in msgs] == [(address, function, 0, 0, 0)]
            assert info["messages"] == 1 and info["batches"] == 1 and info["orphans"] == 0 and info["bad_codewords"] == 0
            assert "Tone: " in fmd.pocsag_text(msgs[0]) and "Address: %07d  Function: %d" % (address, function) in fmd.pocsag_text(msgs[0])
    assert (fmd.pocsag_text(msgs[0], 512) == "POCSAG512: Address: %07d  Function: 3  Tone: " % address)


def test_numeric_and_alpha_round_trips_the_alpha_over_a_batch_boundary(fmd):
    number = "0123456789*U -)(42"
    text = "The quick brown fox jumps over the lazy dog 0123456789 times, ~{|}!"     # 67 characters: 24 words from frame 5 on
    bits = fmd.pocsag_encode([(1234560, 0, number, "numeric"), (765437, 3, text, "alpha")], preamble=576)
    assert len(bits) == 576 + 3 * 544
    soft, hits = _soft(bits)
    assert len(hits) == 3
    msgs, info = _both(fmd, soft, hits, cuts=[1, 7, 1000, 333, 10 ** 6])
    assert [(m["address"], m["function"]) for m in msgs] == [(1234560, 0), (765437, 3)] and info["batches"] == 3
    assert fmd.pocsag_numeric(msgs[0]).rstrip(" ") == number and fmd.pocsag_alpha(msgs[1]) == text
    assert fmd.pocsag_text(msgs[0], 1200) == "POCSAG1200: Address: 1234560  Function: 0  Numeric: " + fmd.pocsag_numeric(msgs[0])
    assert fmd.pocsag_text(msgs[1], 2400) == "POCSAG2400: Address: 0765437  Function: 3  Alpha: " + text
    assert fmd.pocsag_text(msgs[1], 1200, "numeric").startswith("POCSAG1200: Address: 0765437  Function: 3  Numeric: ")
    assert fmd.pocsag_text(msgs[0], 1200, "alpha").startswith("POCSAG1200: Address: 1234560  Function: 0  Alpha: ")
    assert msgs[0]["end_sample"] < msgs[1]["end_sample"] < len(soft)
    with pytest.raises(ValueError):
        fmd.pocsag_text(msgs[0], 1200, "hex")


@pytest.fixture(scope="module")
def probe_exe(fmd, tmp_path_factory):
    fmd.lib()
    exe = str(tmp_path_factory.mktemp("probe") / "pocsag_probe")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pocsag_probe.cpp"), "-o", exe, "-L", PKG, "-lfmd_hip", "-Wl,-rpath," + PKG],
                   check=True, timeout=300)
    return exe


def test_text_in_cpp_and_python_character_for_character(fmd, probe_exe):
    rng = np.random.default_rng(3)
    cases = [(5, 0, 0, b"")]
    for n_bits in (20, 40, 140, 2560, 2580, 19):
        data = rng.integers(0, 256, (min(n_bits, 2560) + 7) // 8, dtype=np.uint8).tobytes()
        cases += [(int(rng.integers(0, 1 << 21)), f, n_bits, data) for f in range(4)]
    etx = fmd.pocsag_encode([(8, 1, "AB\x03\x04", "alpha")], preamble=0)
    cases.append((8, 1, 40, np.packbits(np.concatenate([etx[65:85], etx[97:117]])).tobytes()))
    for address, function, n_bits, data in cases:
        msg = {"address": address, "function": function, "n_bits": n_bits, "bits": data}
        for mode, name in enumerate(("auto", "numeric", "alpha")):
            out = subprocess.run([probe_exe, "text", "1200", str(mode), str(address), str(function), str(n_bits), data.hex() or "00"],
                                 check=True, capture_output=True, timeout=60).stdout.decode("latin-1")
            assert out == fmd.pocsag_text(msg, 1200, name) + "\n", (address, function, n_bits, name)
    assert fmd.pocsag_alpha({"n_bits": 40, "bits": cases[-1][3]}) == "AB"


def test_a_tone_only_page_an_orphan_message_word_and_an_idle_word_inside_a_message(fmd):
    from rtl_sdr_rs_amd.pocsag import POCSAG_IDLE as IDLE, pocsag_codeword as cw
    a1, a2 = cw(0x155 << 2 | 1), cw(0x2AA << 2 | 2)
    m = [cw(1 << 20 | v) for v in (0x12345, 0xABCDE, 0xFFFFF)]
    # frame 0: an orphan; frame 1: address 1 and a word; frame 2: idle, then a word that is an orphan again; frame 3: a tone-only page
    # closed by the address behind it; that one's message runs to the end of the batch and is closed by the lost sync
    words = [m[0], IDLE, a1, m[1], IDLE, m[2], a2, a1] + m * 2 + [m[0], m[1]]
    soft, hits = _soft(fmd.pocsag_encode(None, preamble=32, words=words))
    msgs, info = _both(fmd, soft, hits, cuts=[17] * 1000)
    assert [(x["address"], x["function"], x["n_bits"]) for x in msgs] == [(0x155 << 3 | 1, 1, 20), (0x2AA << 3 | 3, 2, 0), (0x155 << 3 | 3, 1, 160)]
    assert info["orphans"] == 2 and info["messages"] == 3 and info["locked"] == 0 and info["batches"] == 1
    assert msgs[0]["bits"] == bytes([0xAB, 0xCD, 0xE0])


@pytest.mark.parametrize("n_bits", [2560, 2580])
def test_bits_behind_2560_are_counted_and_not_stored(fmd, n_bits):
    rng = np.random.default_rng(n_bits)
    bits = rng.integers(0, 2, n_bits).tolist()
    soft, hits = _soft(fmd.pocsag_encode([(9, 2, bits, "bits")], preamble=64))
    msgs, info = _both(fmd, soft, hits, cuts=[4001] * 100)
    assert len(msgs) == 1 and msgs[0]["n_bits"] == n_bits and len(msgs[0]["bits"]) == 320
    assert np.unpackbits(np.frombuffer(msgs[0]["bits"], np.uint8)).tolist() == bits[:2560]
    assert info["batches"] == len(hits) == 9


def test_a_lost_sync_in_the_middle_of_a_message_closes_it_and_the_rest_are_orphans(fmd):
    bits = np.ones(900, np.int64).tolist()
    soft, hits = _soft(fmd.pocsag_encode([(16, 1, bits, "bits")], preamble=64))
    assert len(hits) == 3
    msgs, info = _both(fmd, soft, [hits[0], hits[2]], cuts=[999] * 100)     # the second sync word is not reported
    assert [(m["address"], m["n_bits"]) for m in msgs] == [(16, 300)] and info["batches"] == 2 and info["orphans"] == 14
    msgs, info = _both(fmd, soft, hits)
    assert [(m["address"], m["n_bits"]) for m in msgs] == [(16, 900)] and info["orphans"] == 0


def test_two_transmissions_of_opposite_polarity(fmd):
    a, ha = _soft(fmd.pocsag_encode([(100, 3, "first", "alpha")]), dc=900)
    b, hb = _soft(fmd.pocsag_encode([(204, 3, "second", "alpha")]), dc=-700, invert=True)
    soft = np.concatenate([a, b])
    hits = ha + [(k + len(a), d, c, t) for k, d, c, t in hb]
    msgs, info = _both(fmd, soft, hits, cuts=[333] * 1000)
    assert [(m["address"], m["inverted"], fmd.pocsag_alpha(m)) for m in msgs] == [(100, 0, "first"), (204, 1, "second")]
    # a record of the other polarity where the next sync is due does not count: the lock is lost
    two = fmd.pocsag_encode([(100, 3, "x" * 60, "alpha")])
    soft, hits = _soft(two)
    assert len(hits) == 2
    flipped = [hits[0], (hits[1][0], 32 | 1 << 31, -hits[1][2], hits[1][3])]
    msgs, info = _both(fmd, soft, flipped)
    assert info["batches"] == 1 and [(m["inverted"], m["n_bits"]) for m in msgs] == [(0, 140)] and info["locked"] == 0


def test_the_larger_correlation_wins_in_the_search_window_and_the_first_of_equals_at_slot_16(fmd):
    soft, hits = _soft(fmd.pocsag_encode([(8, 0, "12345", "numeric")], preamble=64))
    k, d, c, t = hits[0]
    # the true record two samples late with a smaller correlation in front of it; one outside the window is ignored
    early = [(k - 2, 1, c - 1000, t), (k, d, c, t), (k - 2 + SPB + 1, 0, c + 5000, t)]
    msgs, info = _both(fmd, soft, early)
    assert [fmd.pocsag_numeric(m) for m in msgs] == ["12345"] and info["batches"] == 1
    # equal correlations: the first stays
    msgs, info = _both(fmd, soft, [(k, d, c, t), (k + 1, d, c, 32 * 3000)])
    assert [fmd.pocsag_numeric(m) for m in msgs] == ["12345"]


@pytest.mark.parametrize("cap", [0, 1, 16])
def test_the_ring_of_64_with_70_messages(fmd, cap):
    from rtl_sdr_rs_amd import pocsag
    pages = [(8 * i, i & 3, "", "tone") for i in range(70)]  # all in frame 0: two to a batch
    soft, hits = _soft(fmd.pocsag_encode(pages, preamble=64))
    assert len(hits) == 35
    lib, h, n = fmd.lib(), C.c_void_p(), C.c_size_t(0)
    assert lib.fmd_pocsag_decoder_new(1200 * SPB, 1, 1200, 1, C.byref(h)) == 0
    ref = pr.Decoder(1200 * SPB, 1, 1200, 1)
    buf = (pocsag.PocsagMsg * 16)()
    rec = np.array(hits, pocsag.HIT_DTYPE)
    assert lib.fmd_pocsag_decoder_push(h, soft.ctypes.data, len(soft), rec.ctypes.data, len(rec), buf, cap, C.byref(n)) == 0
    want = ref.push(soft, hits, cap=cap)
    got = [buf[i].address for i in range(n.value)]
    assert n.value == len(want) == min(cap, 70) and got == [m["address"] for m in want]
    while True:                                              # drained: the newest 64 of what did not fit
        assert lib.fmd_pocsag_decoder_push(h, None, 0, None, 0, buf, 16, C.byref(n)) == 0
        more = ref.push([], [], cap=16)
        assert [buf[i].address for i in range(n.value)] == [m["address"] for m in more]
        got += [buf[i].address for i in range(n.value)]
        if n.value < 16:
            break
    assert got == [8 * i for i in range(70)][:cap] + [8 * i for i in range(70)][max(cap, 6):]
    info = pocsag.PocsagInfo()
    assert lib.fmd_pocsag_decoder_info(h, C.byref(info)) == 0 and info.messages == 70 == ref.info()["messages"]
    lib.fmd_pocsag_decoder_free(h)


def test_reset_and_pushes_of_single_samples(fmd):
    from rtl_sdr_rs_amd import pocsag
    soft, hits = _soft(fmd.pocsag_encode([(77, 1, "single samples", "alpha")], preamble=64), dc=-1200)
    whole, info = _both(fmd, soft, hits)
    ones, info1 = _both(fmd, soft, hits, cuts=[1] * len(soft))
    assert whole == ones and info == info1 and fmd.pocsag_alpha(whole[0]) == "single samples"
    dec = fmd.PocsagDecoder(1200 * SPB, 1, 1200)
    cut = hits[0][0] + 40 * SPB                              # inside the batch
    assert dec.push(soft[:cut], np.array(hits, pocsag.HIT_DTYPE)) == [] and dec.info()["locked"] == 1
    dec.reset()
    assert dec.info() == {"messages": 0, "batches": 0, "bad_codewords": 0, "orphans": 0, "locked": 0, "searching": 0}
    assert dec.push(soft, np.array(hits, pocsag.HIT_DTYPE)) == whole and dec.info() == info


def test_records_at_or_beyond_n_and_out_of_order_are_passed_over(fmd):
    soft, hits = _soft(fmd.pocsag_encode([(8, 0, "777", "numeric")], preamble=64))
    k, d, c, t = hits[0]
    junk = [(k - 50, 0, 10 ** 6, 0), (len(soft), 0, 10 ** 6, 0), (0xFFFFFFFF, 0, 10 ** 6, 0)]
    msgs, info = _both(fmd, soft, [hits[0]] + junk)
    assert [fmd.pocsag_numeric(m) for m in msgs] == ["777  "] and info["batches"] == 1


def test_bad_codewords_close_the_message_and_are_counted(fmd):
    from rtl_sdr_rs_amd.pocsag import pocsag_codeword as cw
    words = [cw(0x3 << 2), cw(1 << 20 | 0x11111), cw(1 << 20 | 0x22222) ^ 0x00300001, cw(1 << 20 | 0x33333) ^ 0x8000] + [0x7A89C197] * 12
    soft, hits = _soft(fmd.pocsag_encode(None, preamble=32, words=words))
    for e, bad, orphans, fixed in ((0, 2, 0, 0), (1, 1, 1, 0), (2, 1, 1, 0)):
        msgs, info = _both(fmd, soft, hits, max_errors=e)
        assert info["bad_codewords"] == bad and info["orphans"] == orphans and [m["n_bits"] for m in msgs] == [20]
        assert msgs[0]["corrected"] == fixed


# ---- the behaviour of the two definitions --------------------------------------------------------------------------------------------
def _demod(rate, baud):
    from rtl_sdr_rs_amd import pocsag
    d = pocsag.fsk_design(rate, baud)
    return d, fr.FskDemod(fr.Cfg(d.D, d.W, d.shift, d.tap, d.sync, d.tol, d.min_corr, d.hit_cap), 1)


def _receive(d, dem, rate, baud, audio, call=4096):
    dec = pr.Decoder(int(rate), d.D, int(baud), 1)
    msgs, syncs = [], 0
    for lo in range(0, len(audio), call):
        soft, counts, rec = dem.run(audio[None, lo:lo + call])
        syncs += int(counts[0])
        assert counts[0] <= d.hit_cap
        msgs += dec.push(soft[0], rec[0, :counts[0]].tolist())
    return msgs, dec.info(), syncs


CONDITIONS = [("clean", 4000, 2500, 0, False), ("noise-1500", 4000, -2500, 1500, False), ("weak", 1000, 600, 400, False),
              ("inverted", 4000, 2500, 1500, True)]


def _pages(rng, n=20):
    alphabet = "ABCDEFGHIJKLMNOPQRSTUVWXYZ abcdefghijklmnopqrstuvwxyz0123456789.,:-"
    return [(int(rng.integers(0, 1 << 21)), int(rng.integers(1, 4)),
             "".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(10, 41)))), "alpha") for _ in range(n)]


def _case(fmd, rng, rate, baud, amp, dc, noise, invert):
    pages = _pages(rng)
    audio = [np.clip(np.rint(dc + rng.normal(0, noise, 500) if noise else np.full(500, float(dc))), -32768, 32767).astype(np.int16)]
    for p in pages:
        audio.append(pr.fsk_audio(rng, fmd.pocsag_encode([p], preamble=576), rate, baud, amp, dc, noise, ppm=30.0,
                                  tail=int(rng.integers(200, 2001)), invert=invert))
    return pages, np.concatenate(audio)


@pytest.mark.parametrize("rate,baud", PAIRS, ids=["%d-%d" % p for p in PAIRS])
def test_twenty_of_twenty_pages_and_never_one_that_was_not_sent(fmd, rate, baud):
    """20 pages of 10 to 40 characters in transmissions of their own, 576 bits of preamble, the sender 30 ppm off at a
    random bit phase, 200 to 2000 samples of gap: all 20 and nothing else under every asserted condition."""
    rng = np.random.default_rng(rate * 10 + baud)
    for name, amp, dc, noise, invert in CONDITIONS:
        d, dem = _demod(rate, baud)
        pages, audio = _case(fmd, rng, rate, baud, amp, dc, noise, invert)
        msgs, info, syncs = _receive(d, dem, rate, baud, audio)
        got = [(m["address"], m["function"], fmd.pocsag_alpha(m)) for m in msgs]
        print("%d/%d %s: %d of 20, %d sync hits, %d batches, %d bad codewords" % (rate, baud, name,
              sum(g in [p[:3] for p in pages] for g in got), syncs, info["batches"], info["bad_codewords"]))
        assert got == [p[:3] for p in pages], (name, info)
        assert all(m["inverted"] == int(invert) for m in msgs)


@pytest.mark.parametrize("rate,baud", PAIRS, ids=["%d-%d" % p for p in PAIRS])
def test_forty_seconds_of_noise_alone_and_of_zeros_deliver_nothing(fmd, rate, baud):
    rng = np.random.default_rng(rate + baud)
    for noise in (3000.0, 0.0):
        d, dem = _demod(rate, baud)
        dec = pr.Decoder(int(rate), d.D, int(baud), 1)
        call = 100000
        for lo in range(0, 40 * rate, call):
            n = min(call, 40 * rate - lo)
            x = np.clip(np.rint(rng.normal(0, noise, n)), -32768, 32767).astype(np.int16) if noise else np.zeros(n, np.int16)
            soft, counts, rec = dem.run(x[None])
            assert dec.push(soft[0], rec[0, :min(int(counts[0]), d.hit_cap)].tolist()) == []
        assert dec.info()["messages"] == 0


# ---- the fuzz program ------------------------------------------------------------------------------------------------------------------
def test_decoder_fuzz_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/pocsag_fuzz.cpp with csrc/fmd_pocsag_decode.cpp, a program of its own: random soft streams and records (k_rel beyond
    n and out of order among them), transmissions intact, flipped and cut off, random push sizes, cap 0 / 1 / 16.  It ends clean."""
    exe = str(tmp_path / "pocsag_fuzz")
    # (the sanitizers' runtimes are linked in statically: the program needs nothing preloaded and runs in any environment)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "cpp", "pocsag_fuzz.cpp"),
                    os.path.join(PKG, "csrc", "fmd_pocsag_decode.cpp"), "-o", exe], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stderr.decode()[-2000:])
    words = p.stdout.decode().split()
    assert words[0] == "ok" and int(words[words.index("intact") + 1]) > 20


# ---- the tool ------------------------------------------------------------------------------------------------------------------------
USAGE = """usage: %s -r rate [-b baud] [-e max_errors] [-m auto|numeric|alpha] [in.s16]
       (pager decoder: raw mono s16 of an NFM channel in, one line per POCSAG message out, the counters on stderr)
"""
MISSING = "/nonexistent-dir/in.s16"
NO_DEVICE_TEXT = "error: no usable gfx950 device: "

EARLY = [
    (["-h"], 0, USAGE % CLI),
    (["--help"], 0, USAGE % CLI),
    ([], 2, "need -r rate\n"),
    (["-r"], 2, "-r needs a value\n"),
    (["-r", "12k"], 2, "bad -r: 12k\n"),
    (["-r", "12000", "-b", "0"], 2, "bad -b: 0\n"),
    (["-r", "12000", "-e", "-1"], 2, "bad -e: -1\n"),
    (["-r", "12000", "-m"], 2, "-m needs a value\n"),
    (["-r", "12000", "-m", "hex"], 2, "bad -m: hex\n"),
    (["-r", "12000", "a.s16", "b.s16"], 2, "too many files\n"),
    (["-r", "12000", MISSING], 2, MISSING + ": No such file or directory\n"),
    (["-r", "1000000", os.devnull], 1, "error: rate / baud out of range\n"),
    (["-r", "12000", "-e", "3", os.devnull], 1, "error: unsupported configuration (-6): need max_errors <= 2\n"),
]


def run_cli(args, cwd):
    p = subprocess.run([CLI] + args, cwd=cwd, capture_output=True, timeout=120)
    return p.returncode, p.stdout, p.stderr.decode()


@pytest.mark.parametrize("args,code,stderr", EARLY, ids=[" ".join(c[0]) for c in EARLY])
def test_cli_early_exits(fmd, args, code, stderr, tmp_path):
    fmd.lib()
    got = run_cli(args, tmp_path)
    if code == 1 and "(-6)" in stderr:                       # the library's refusal: its text follows the status name
        assert got[0] == 1 and got[1] == b"" and got[2].startswith("error: ") and got[2].endswith(stderr.split(": ")[-1])
    else:
        assert got == (code, b"", stderr)


@pytest.mark.parametrize("args", [[], ["-b", "512", "-e", "2", "-m", "numeric"], ["-b", "2400", "-e", "0"]], ids=["defaults", "512", "2400"])
def test_cli_no_device_is_exit_1_with_the_library_message(fmd, args, tmp_path):
    code, stdout, stderr = run_cli(["-r", "12000"] + args + [os.devnull], tmp_path)
    if fmd.device_count() > 0:                               # with a device the empty input gives no line and zero counters
        assert (code, stdout, stderr) == (0, b"", "messages 0 batches 0 bad_codewords 0 orphans 0\n")
    else:
        assert (code, stdout) == (1, b"") and stderr.startswith(NO_DEVICE_TEXT)
        assert stderr.count("\n") == 1 and stderr.endswith("\n")
