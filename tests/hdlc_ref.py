"""The frame bank's definition (include/fmd.h, fmd_hdlc_*): n_rows decoders of tests/ax25_ref.py, each pushed exactly its row's samples
of a call, and the packaging of a call's results -- the count of the frames that passed in it, the first frame_cap of them as records
(data zero behind len), the cumulative counters."""
import numpy as np

import ax25_ref as ar

FRAME_DTYPE = np.dtype([("data", np.uint8, 512), ("len", np.uint32), ("pad", np.uint32), ("end_sample", np.uint64)])   # fmd_ax25_frame


class Framer:
    def __init__(self, rate_num, rate_den=1, baud=1200, frame_cap=4, rows=1):
        if not 1 <= frame_cap <= 16:
            raise ValueError("need 1 <= frame_cap <= 16")
        if rows < 1:
            raise ValueError("need n_rows >= 1")
        self.decs = [ar.Decoder(rate_num, rate_den, baud) for _ in range(rows)]
        self.rows, self.frame_cap, self.pos = rows, frame_cap, 0
        self.last = (np.zeros(rows, np.uint32), np.zeros((rows, frame_cap), FRAME_DTYPE), [[] for _ in range(rows)])

    def reset(self):
        for d in self.decs:
            d.reset()
        self.pos = 0
        self.last = (np.zeros(self.rows, np.uint32), np.zeros((self.rows, self.frame_cap), FRAME_DTYPE), [[] for _ in range(self.rows)])

    def run(self, soft):
        """soft int16 [rows, n] -> (counts uint32 [rows], records [rows, frame_cap], all the call's frames per row as the decoder
        gives them); a call of no samples leaves and returns the last call's."""
        soft = np.asarray(soft, np.int16)
        assert soft.ndim == 2 and soft.shape[0] == self.rows
        if soft.shape[1] == 0:
            return self.last
        counts, rec, every = np.zeros(self.rows, np.uint32), np.zeros((self.rows, self.frame_cap), FRAME_DTYPE), []
        for r, d in enumerate(self.decs):
            frames = d.push(soft[r])
            every.append(frames)
            counts[r] = len(frames)
            for k, f in enumerate(frames[:self.frame_cap]):
                rec[r, k]["data"][:len(f["data"])] = np.frombuffer(f["data"], np.uint8)
                rec[r, k]["len"] = len(f["data"])
                rec[r, k]["end_sample"] = f["end_sample"]
        self.pos += soft.shape[1]
        self.last = (counts, rec, every)
        return self.last

    def info(self):
        return [d.info() for d in self.decs]


def levels_to_soft(levels, num, den=1, amp=9000, start=0):
    """The line levels held for num / den samples each (sample i shows level floor((start + i) den / num)): int16 +amp for mark,
    -amp for space."""
    n = (len(levels) * num) // den - start
    idx = ((start + np.arange(n, dtype=np.int64)) * den) // num
    lv = np.asarray(levels, np.int64)[idx]
    return np.where(lv == 1, amp, -amp).astype(np.int16)
