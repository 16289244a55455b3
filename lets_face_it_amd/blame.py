"""Host side of the step guard's blame record (include/lfi.h, lfi_segment_stats_guard): pure arithmetic on the words the device left -
which input tensor, which frame and row, which gradient tensors held a NaN or an Inf on the first skipped step - and the short report
the Trainer prints. No device, no library: GlowEngine.blame_state() hands the copied record in."""
import math
import struct

from ._lib import BLAME_FILLED, BLAME_HEAD, BLAME_STEP, SEG_FIRST, SEG_INF, SEG_NAN, SEG_NONE, SEG_SLOTS, SEG_SUMSQ

MAX_NAMES = 8      # names listed in a report before "... and k more"


def _u64(word):
    return int(word) & (2 ** 64 - 1)


def _f64(word):
    return struct.unpack("<d", struct.pack("<Q", _u64(word)))[0]


def record_of(words, i):
    """Record i of a table of LFI_SEG_SLOTS 8-byte words per array -> {sumsq, nan, inf, first}; first is None without a non-finite
    element."""
    w = words[SEG_SLOTS * i:SEG_SLOTS * (i + 1)]
    first = _u64(w[SEG_FIRST])
    return {"sumsq": _f64(w[SEG_SUMSQ]), "nan": _u64(w[SEG_NAN]), "inf": _u64(w[SEG_INF]), "first": None if first == SEG_NONE else first}


def input_index(index, shape):
    """Flat index into a batch-first (B, T, dim) input tensor -> (row, frame, column)."""
    _, T, dim = shape
    return (index // (T * dim), (index // dim) % T, index % dim)


def nll_index(index, B):
    """Flat index into the frame-major (N, B) per-frame NLL -> (frame, row); frame 0 is the first modelled frame."""
    return (index // B, index % B)


def decode(words, keys, inputs, nll_shape, gmul=1.0):
    """The blame record as copied from the device (a sequence of 8-byte words: header, then one record per gradient segment, per
    input tensor and for the NLL) -> None while FILLED is 0, else
      {"step", "inputs": {name: {nan, inf, first: (row, frame, column)}}      only tensors holding a non-finite element,
       "nll": {nan, inf, count, first: (frame, row) | None} | None,
       "gradients": [{key, nan, inf, first}]                                   only tensors holding a non-finite element,
       "norms": {key: sqrt(SUMSQ) * |gmul|}, "tensors": number of gradient tensors}.
    keys: state_dict keys of the segments; inputs: [(name, shape)]; nll_shape: (N, B) or None."""
    if _u64(words[BLAME_FILLED]) == 0:
        return None
    table = words[BLAME_HEAD:]
    g = abs(float(gmul))
    grads, norms = [], {}
    for i, key in enumerate(keys):
        r = record_of(table, i)
        norms[key] = math.sqrt(r["sumsq"]) * g
        if r["nan"] or r["inf"]:
            grads.append({"key": key, "nan": r["nan"], "inf": r["inf"], "first": r["first"]})
    bad_inputs = {}
    for j, (name, shape) in enumerate(inputs):
        r = record_of(table, len(keys) + j)
        if r["nan"] or r["inf"]:
            bad_inputs[name] = {"nan": r["nan"], "inf": r["inf"], "first": input_index(r["first"], shape)}
    nll = None
    if nll_shape is not None:
        r = record_of(table, len(keys) + len(inputs))
        nll = {"nan": r["nan"], "inf": r["inf"], "count": int(nll_shape[0]) * int(nll_shape[1]),
               "first": None if r["first"] is None else nll_index(r["first"], int(nll_shape[1]))}
    return {"step": _u64(words[BLAME_STEP]), "inputs": bad_inputs, "nll": nll, "gradients": grads, "norms": norms, "tensors": len(keys)}


def _cut(names):
    names = list(names)
    if len(names) <= MAX_NAMES:
        return ", ".join(names)
    return ", ".join(names[:MAX_NAMES]) + " ... and %d more" % (len(names) - MAX_NAMES)


def report(state):
    """One line for the log and for the stopping error: where the first skipped step's non-finite values sat."""
    parts = []
    if state["inputs"]:
        parts.append("inputs: " + _cut("%s %d non-finite (first: row %d, frame %d, column %d)" % ((name, v["nan"] + v["inf"]) + tuple(v["first"]))
                                       for name, v in state["inputs"].items()))
    else:
        parts.append("inputs: finite")
    nll = state["nll"]
    if nll is not None and (nll["nan"] or nll["inf"]):
        parts.append("NLL: %d of %d frames (first: frame %d, row %d)" % ((nll["nan"] + nll["inf"], nll["count"]) + tuple(nll["first"])))
    elif nll is not None:
        parts.append("NLL: finite")
    bad = state["gradients"]
    if bad:
        parts.append("gradients: %d of %d tensors non-finite (first: %s)" % (len(bad), state["tensors"], _cut(b["key"] for b in bad)))
    else:
        parts.append("gradients: no tensor non-finite")
    return "step %d: %s" % (state["step"], "; ".join(parts))
