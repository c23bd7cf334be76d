"""The page bank's definition (include/fmd.h, fmd_pager_*): n_rows decoders of tests/pocsag_ref.py, each pushed exactly its row's
samples of a call and the first min(count, hit_cap) records of that call, and the packaging of a call's results -- the count of the
messages that closed in it, the first msg_cap of them as records (bits zero behind (min(n_bits, 2560) + 7) / 8 bytes), the cumulative
counters with locked and searching."""
import numpy as np

import pocsag_ref as pr

MSG_DTYPE = np.dtype([("address", np.uint32), ("function", np.uint32), ("n_bits", np.uint32), ("bits", np.uint8, 320),
                      ("corrected", np.uint32), ("inverted", np.uint32), ("pad", np.uint32), ("end_sample", np.uint64)])   # fmd_pocsag_msg
HIT_DTYPE = np.dtype([("k_rel", np.uint32), ("d", np.uint32), ("corr", np.int32), ("thr", np.int32)])                      # fmd_fsk_hit


def max_messages(rate_num, rate_den, baud, n):
    """M(n) of the header: q = mod // step, B = ceil(n / q), (B + 31) // 32 + 1 + B // 512"""
    q = rate_num // (baud * rate_den)
    B = (n + q - 1) // q
    return (B + 31) // 32 + 1 + B // 512


class Pager:
    def __init__(self, rate_num, rate_den=1, baud=1200, max_errors=1, msg_cap=4, rows=1):
        if not 1 <= msg_cap <= 16:
            raise ValueError("need 1 <= msg_cap <= 16")
        if rows < 1:
            raise ValueError("need n_rows >= 1")
        self.decs = [pr.Decoder(rate_num, rate_den, baud, max_errors) for _ in range(rows)]
        self.rows, self.msg_cap = rows, msg_cap
        self.reset()

    def reset(self):
        for d in self.decs:
            d.reset()
        self.pos = 0
        self.last = (np.zeros(self.rows, np.uint32), np.zeros((self.rows, self.msg_cap), MSG_DTYPE), [[] for _ in range(self.rows)])

    def run(self, soft, counts=None, hits=None):
        """soft int16 [rows, n], counts [rows], hits [rows, hit_cap] records -> (counts uint32 [rows], records [rows, msg_cap], all
        the call's messages per row as the decoder gives them); a call of no samples leaves and returns the last call's."""
        soft = np.asarray(soft, np.int16)
        assert soft.ndim == 2 and soft.shape[0] == self.rows
        if soft.shape[1] == 0:
            return self.last
        if counts is None:
            counts, hits = np.zeros(self.rows, np.uint32), np.zeros((self.rows, 1), HIT_DTYPE)
        hits = np.asarray(hits, HIT_DTYPE)
        assert hits.ndim == 2 and hits.shape[0] == self.rows and 1 <= hits.shape[1] <= 64
        out, rec, every = np.zeros(self.rows, np.uint32), np.zeros((self.rows, self.msg_cap), MSG_DTYPE), []
        for r, d in enumerate(self.decs):
            h = hits[r, :min(int(counts[r]), hits.shape[1])]
            msgs = d.push(soft[r], [(x["k_rel"], x["d"], x["corr"], x["thr"]) for x in h])
            every.append(msgs)
            out[r] = len(msgs)
            for k, m in enumerate(msgs[:self.msg_cap]):
                for f in ("address", "function", "n_bits", "corrected", "inverted", "end_sample"):
                    rec[r, k][f] = m[f]
                rec[r, k]["bits"][:len(m["bits"])] = np.frombuffer(m["bits"], np.uint8)
        self.pos += soft.shape[1]
        self.last = (out, rec, every)
        return self.last

    def info(self):
        return [d.info() for d in self.decs]
