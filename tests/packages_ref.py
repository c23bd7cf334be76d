"""The definition of the package bank (include/fmd.h, fmd_packages_*) in plain Python: n_streams slicers of tests/pulse_slice_ref.py,
each with an unbounded waiting room.

Per call, stream s is pushed the first min(count_s, rec_cap) records with pos_s = samples_s - n_samples (samples_s: the stream's
fmd_pulses_totals.samples after the call) and is then given idle(state_s, run_s).  What closed in the call, in the order it closed, is
the call's packages; those with n_bits < min_bits count in `packages` and `skipped` and are not delivered.  count is every delivered
package, the first pkg_cap of them are kept.  n_pulses saturates at 2^32 - 1 as on the host."""
import pulse_slice_ref as sref

PWM, PPM, BAD, TRUNCATED = sref.PWM, sref.PPM, sref.BAD, sref.TRUNCATED
SAT = 2 ** 32 - 1
ZERO = {"records": 0, "packages": 0, "skipped": 0, "bad": 0, "open": 0, "open_pulses": 0}


def packages_max(n_records):
    return n_records + 1


class Unbounded(sref.Slicer):
    """sref.Slicer with room for every package, and n_pulses saturating as the host slicer's."""

    def _close(self):
        k = dict(self.cur)
        k["bits"], k["n_pulses"] = bytes(k["bits"]), min(k["n_pulses"], SAT)
        self.waiting.append(k)
        self.cur = None


class Stream:
    def __init__(self, modulation, short, long, tol, reset, min_bits=0, pkg_cap=1025):
        assert 0 <= min_bits <= 256 and 1 <= pkg_cap <= 1025
        self.args, self.min_bits, self.pkg_cap = (modulation, short, long, tol, reset), min_bits, pkg_cap
        self.reset()

    def reset(self):
        self.slicer = Unbounded(*self.args)
        self.tot = {"records": 0, "packages": 0, "skipped": 0, "bad": 0}

    @property
    def info(self):
        cur = self.slicer.cur
        return dict(self.tot, open=int(cur is not None), open_pulses=min(cur["n_pulses"], SAT) if cur else 0)

    def _harvest(self):
        closed = self.slicer.take(len(self.slicer.waiting))
        good = [k for k in closed if k["n_bits"] >= self.min_bits]
        self.tot["packages"] += len(closed)
        self.tot["skipped"] += len(closed) - len(good)
        self.tot["bad"] += sum(1 for k in closed if k["flags"] & BAD)
        return len(good), good[:self.pkg_cap]

    def run(self, count, recs, rec_cap, totals, n_samples):
        """One call: (count, kept packages).  recs: the stream's row, of which the first min(count, rec_cap) are read; totals: a dict
        with samples, state and run."""
        take = list(recs[:min(count, rec_cap)])
        assert len(take) == min(count, rec_cap)
        self.slicer.push(take, (totals["samples"] - n_samples) % 2 ** 64)
        self.slicer.idle(totals["state"], totals["run"])
        self.tot["records"] += len(take)
        return self._harvest()

    def flush(self):
        self.slicer.idle(0, self.args[4])
        return self._harvest()


class Bank:
    def __init__(self, n_streams, modulation, short, long, tol, reset, min_bits=0, pkg_cap=1025):
        self.streams = [Stream(modulation, short, long, tol, reset, min_bits, pkg_cap) for _ in range(n_streams)]

    def run(self, counts, recs, rec_cap, totals, n_samples):
        """(counts, kept packages per stream) of one call"""
        got = [st.run(int(counts[s]), recs[s], rec_cap, totals[s], n_samples) for s, st in enumerate(self.streams)]
        return [g[0] for g in got], [g[1] for g in got]

    def flush(self):
        got = [st.flush() for st in self.streams]
        return [g[0] for g in got], [g[1] for g in got]

    def reset(self):
        for st in self.streams:
            st.reset()

    @property
    def info(self):
        return [st.info for st in self.streams]
