"""Test-side definition of the band-plan bank (include/fmd.h, "band-plan bank"): the narrow-band bank's definition
(tests/narrow_ref.py) over the uniform channelizer's y (tests/uniform_ref.py) -- a composition, no new arithmetic.  Independent of
the library.  `narrow_ref.direct` over the y of one row is the same definition one sample at a time."""
import numpy as np

import narrow_ref as nr
import stations_ref as sr
import uniform_ref as ur
from stations_ref import TooShort  # noqa: F401  (re-exported: a call that completes no audio sample)

IQ, FM, AM, SSB = nr.IQ, nr.FM, nr.AM, nr.SSB


def y_bound(h, n_channels, shift, channels=None):
    """B_y = ceil(256 G / 2^shift), G over the selected channels."""
    return -(-256 * sr.max_gain(h, ur.channel_incs(n_channels, channels)) >> int(shift))


def gain_sum(gr, gi=None):
    g = int(np.abs(np.asarray(gr, np.int64)).sum())
    return g + (0 if gi is None else int(np.abs(np.asarray(gi, np.int64)).sum()))


def min_chan_shift(h, n_channels, shift, gr, gi=None, channels=None, limit=16384):
    """The smallest chan_shift with ceil(B_y sum(|gr| + |gi|) / 2^chan_shift) <= limit."""
    peak, s = y_bound(h, n_channels, shift, channels) * gain_sum(gr, gi), 0
    while -(-peak >> s) > limit:
        s += 1
    return s


class BandPlanRef(nr.NarrowRef):
    """One input stream, the selected channels of a plan; feed() mirrors one fmd_bandplan call of that stream (whole hops) and
    returns int64 [n_selected, n] ([n_selected, n, 2] in IQ mode).  A call that completes no audio sample raises TooShort and
    changes nothing, stage one included."""

    def __init__(self, h, n_channels, hop, shift, gr, gi, mode, chan_decim, chan_shift, block, squelch, gain, channels=None,
                 z=sr.z_corr):
        incs = ur.channel_incs(int(n_channels), channels)
        super().__init__(h, hop, incs, shift, gr, gi, mode, chan_decim, chan_shift, block, squelch, gain, z=z)
        self.ch = ur.UniformRef(h, n_channels, hop, shift, channels=channels, z=z)
        self.hop = int(hop)

    def feed(self, buf):
        assert np.asarray(buf).size % (2 * self.hop) == 0
        return super().feed(buf)


def out_cap(hop, chan_decim, nbytes):
    return -(-nbytes // (2 * hop * chan_decim)) if hop and chan_decim else 0
