"""Test-side definition of the FM receiver bank (include/fmd.h, "FM receiver bank"): tests/stereo_ref.py's StereoRef and
tests/rds_ref.py's RdsRef over the same bytes, and the one rule the bank adds -- a call must complete an output of each, or it is
refused and nothing changes.  Independent of the library."""
import numpy as np

import channelizer_ref as cr
import rds_ref as rr
import stereo_ref as st
from stations_ref import TooShort  # noqa: F401  (re-exported)


class _SharedFront(cr.ChannelizerRef):
    """The channelizer of both definitions: the second feed of a call returns the y the first one formed (the two definitions form
    the same y from the same bytes; forming it once keeps the tests quick)."""

    def reset(self):
        super().reset()
        self._y = None

    def feed(self, buf):
        if self._y is not None:
            y, self._y = self._y, None
            return y
        self._y = super().feed(buf)
        return self._y


class ReceiverRef:
    """One input stream, K stations; feed() mirrors one fmd_receiver call of that stream and returns (audio int64 [K, na, 2],
    rds int64 [K, nr, 2])."""

    def __init__(self, taps, decim, incs, shift, capture_rate, audio_taps, audio_decim, audio_shift, rds_taps, rds_decim, rds_shift,
                 block=4096, pilot_min=0, z=None):
        self.stereo = st.StereoRef(taps, decim, incs, shift, capture_rate, audio_taps, audio_decim, block, pilot_min, audio_shift, z=z)
        self.rds = rr.RdsRef(taps, decim, incs, shift, capture_rate, rds_taps, rds_decim, rds_shift, block, pilot_min, z=z)
        self.stereo.ch = self.rds.ch = _SharedFront(taps, decim, incs, shift, z=z)
        self.K = self.stereo.K

    def reset(self):
        self.stereo.reset()
        self.rds.reset()

    def completes(self, nbytes):
        """(audio samples, baseband samples) a call of nbytes completes; the call is refused unless both are >= 1."""
        return self.stereo.completes(nbytes), self.rds.completes(nbytes)

    def outputs(self):
        return self.stereo.n_next, self.rds.n_next

    def feed(self, buf):
        b = np.asarray(buf, dtype=np.uint8)
        if min(self.completes(b.size)) < 1:
            raise TooShort()                                 # nothing changes, in either stage
        return self.stereo.feed(b), self.rds.feed(b)

    def pilot(self, k):
        p = self.stereo.pilot(k)
        assert p == self.rds.pilot(k)
        return p
