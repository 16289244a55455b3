"""What lfi_segment_stats and the blame record behind the step guard have to hold, restated in numpy fp64 (no kernels): the per-array
record, a table over a flat buffer with a segment list plus extra arrays, and the fill-first / clear protocol of the blame header."""
import numpy as np

NONE = 2 ** 64 - 1      # FIRST of an array without a non-finite element


def record(values):
    """{sumsq, nan, inf, first} of one fp32 array: fp64 sum of squares of the finite elements (squares of fp32 values are exact in
    fp64), counts of NaNs and of +-Inf, index of the first non-finite element (NONE without one)."""
    v = np.asarray(values, dtype=np.float32).reshape(-1)
    nan, inf = np.isnan(v), np.isinf(v)
    bad = np.flatnonzero(nan | inf)
    fin = v[~(nan | inf)].astype(np.float64)
    return {"sumsq": float(np.sum(fin * fin)), "nan": int(nan.sum()), "inf": int(inf.sum()), "first": int(bad[0]) if bad.size else NONE}


def table(flat, segments, extras=()):
    """Records of the segments [(offset, length)] of `flat`, then of the extra arrays. What lies in the gaps is never looked at."""
    flat = np.asarray(flat, dtype=np.float32).reshape(-1)
    return [record(flat[o:o + n]) for o, n in segments] + [record(x) for x in extras]


def sumsq_bound(length, ref):
    """|SUMSQ - ref| allowed: any summation order of `length` non-negative fp64 terms errs by at most length * 2^-53 relative, and
    the reference's own sum gets the same allowance."""
    return 2.0 * length * 2.0 ** -53 * ref


class BlameRecord:
    """The header protocol: a call behind a taken step (apply = 1) changes nothing; behind a skipped step it fills the table, the
    step number (APPLIED + SKIPPED as the decide kernel left them) and FILLED - unless FILLED is already 1: the first skipped step
    since the host cleared the header is the one kept."""

    def __init__(self):
        self.filled, self.step, self.table = 0, 0, None

    def call(self, apply, applied, skipped, make_table):
        if apply or self.filled:
            return False
        self.table, self.step, self.filled = make_table(), applied + skipped, 1
        return True

    def read(self, clear=True):
        if not self.filled:
            return None
        out = {"step": self.step, "table": self.table}
        if clear:
            self.filled, self.step = 0, 0
        return out
