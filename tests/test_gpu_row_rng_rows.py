"""GPU: the row-state moves of the keyed noise (lfi_row_rng_seed_rows / lfi_row_rng_save_rows / lfi_row_rng_load_rows,
csrc/lfi_noise.hip) through the C ABI, on a (B, 2) int64 state between guard words, at B = 5 and at B = 300, which is more than one
launch's list: only the listed rows change, bit for bit."""
import ctypes as C

import pytest
import torch

from lets_face_it_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 8                       # (key, position) pairs either side of the state
SENTINEL = -0x0123456789abcdef
MASK = (1 << 64) - 1


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _word(v):
    return v - (1 << 64) if v >> 63 else v


def _key(r):
    return (0x9e3779b97f4a7c15 * (r + 1) + (r << 61)) & MASK         # both halves used, the top bit set in many


def _pos(r):
    return ((r * 7919) << 29) + r                                     # crosses the 32-bit word from r = 8


class _State:
    """B rows of (key, position) between guard pairs, and the host's copy of what they must hold."""

    def __init__(self, B, device, fill=True):
        self.B = B
        self.want = torch.tensor([[_word(_key(r)), _word(_pos(r))] if fill else [SENTINEL, SENTINEL] for r in range(B)],
                                 dtype=torch.int64).view(B, 2)
        self.buf = torch.full((GUARD + B + GUARD, 2), SENTINEL, dtype=torch.int64, device=device)
        self.buf[GUARD:GUARD + B] = self.want.to(device)
        self.ptr = self.buf.data_ptr() + 16 * GUARD

    def check(self):
        host = self.buf.cpu()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + self.B:] == SENTINEL).all(), "guard words written"
        assert torch.equal(host[GUARD:GUARD + self.B], self.want)


def _ints(v):
    return (C.c_int * len(v))(*v)


def _u64(v):
    return (C.c_ulonglong * len(v))(*v)


def _seed(st, rows, keys, pos):
    n = st.B if rows is None else len(rows)
    _lib.check(_lib.lib().lfi_row_rng_seed_rows(st.ptr, st.B, n, None if rows is None else _ints(rows), None if keys is None else _u64(keys),
                                                None if pos is None else _u64(pos), _stream()), "lfi_row_rng_seed_rows")
    for j, r in enumerate(range(n) if rows is None else rows):
        if keys is not None:
            st.want[r, 0] = _word(keys[j])
        st.want[r, 1] = 0 if pos is None else _word(pos[j])
    st.check()


def _lists(B):
    """The row lists of a case: [4, 0] at B = 5; at B = 300 a shuffled list of 281 rows - three launches, the last one partial."""
    if B == 5:
        return [4, 0]
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B)).tolist()
    return perm[:281]


@pytest.mark.parametrize("B", (5, 300))
def test_seed_rows_all_listed_and_positions_only(B, gpu_device):
    st = _State(B, gpu_device, fill=False)
    # every row, rows == NULL: keys at position 0, then keys with positions
    _seed(st, None, [_key(r) for r in range(B)], None)
    _seed(st, None, [_key(r + 1000) for r in range(B)], [_pos(r) for r in range(B)])
    # listed rows only
    rows = _lists(B)
    _seed(st, rows, [_key(7 * r + 3) for r in rows], [_pos(r + 5) for r in rows])
    _seed(st, rows, [MASK - j for j in range(len(rows))], None)                  # positions default to 0
    # keys == NULL: every listed row keeps its key and takes the new position; with neither, position 0
    _seed(st, rows, None, [MASK - 3 * j for j in range(len(rows))])
    _seed(st, rows[:1], None, None)
    # a shorter identity list touches rows 0 .. nrows - 1 only
    _lib.check(_lib.lib().lfi_row_rng_seed_rows(st.ptr, B, 3, None, _u64([11, 12, 13]), None, _stream()), "lfi_row_rng_seed_rows")
    for r in range(3):
        st.want[r] = torch.tensor([11 + r, 0])
    st.check()
    # nothing listed: no launch, nothing moves
    _lib.check(_lib.lib().lfi_row_rng_seed_rows(st.ptr, B, 0, None, None, None, _stream()), "lfi_row_rng_seed_rows")
    st.check()


@pytest.mark.parametrize("B", (5, 300))
def test_save_then_load_with_repeating_entries_and_replacement_keys(B, gpu_device):
    L = _lib.lib()
    st = _State(B, gpu_device)
    rows = _lists(B)
    n = len(rows)
    out = torch.full((GUARD + n + GUARD, 2), SENTINEL, dtype=torch.int64, device=gpu_device)
    _lib.check(L.lfi_row_rng_save_rows(st.ptr, B, n, _ints(rows), out.data_ptr() + 16 * GUARD, _stream()), "lfi_row_rng_save_rows")
    st.check()                                                                   # (a save writes nothing of the state)
    saved = out.cpu()
    assert (saved[:GUARD] == SENTINEL).all() and (saved[GUARD + n:] == SENTINEL).all()
    assert torch.equal(saved[GUARD:GUARD + n], st.want[rows])
    saved_ptr = out.data_ptr() + 16 * GUARD
    # load into another state: other rows, entries that repeat (a branch)
    dst = _State(B, gpu_device, fill=False)
    into = rows[::-1]
    entries = [(3 * j) % max(n // 2, 1) for j in range(n)]
    assert len(set(entries)) < n
    _lib.check(L.lfi_row_rng_load_rows(dst.ptr, B, n, _ints(into), _ints(entries), n, saved_ptr, None, _stream()), "lfi_row_rng_load_rows")
    for r, e in zip(into, entries):
        dst.want[r] = st.want[rows[e]]
    dst.check()
    # replacement keys: the row takes the new key and the entry's position
    keys = [_key(r + 4242) for r in into]
    _lib.check(L.lfi_row_rng_load_rows(dst.ptr, B, n, _ints(into), _ints(entries), n, saved_ptr, _u64(keys), _stream()),
               "lfi_row_rng_load_rows")
    for j, (r, e) in enumerate(zip(into, entries)):
        dst.want[r, 0] = _word(keys[j])
        dst.want[r, 1] = st.want[rows[e], 1]
    dst.check()
    # one row from the last entry, and nothing listed
    _lib.check(L.lfi_row_rng_load_rows(dst.ptr, B, 1, _ints([into[0]]), _ints([n - 1]), n, saved_ptr, None, _stream()),
               "lfi_row_rng_load_rows")
    dst.want[into[0]] = st.want[rows[n - 1]]
    dst.check()
    _lib.check(L.lfi_row_rng_load_rows(dst.ptr, B, 0, None, None, n, None, None, _stream()), "lfi_row_rng_load_rows")
    dst.check()
    st.check()


def test_a_refused_list_launches_nothing(gpu_device):
    L = _lib.lib()
    st = _State(5, gpu_device)
    assert L.lfi_row_rng_seed_rows(st.ptr, 5, 2, _ints([1, 5]), _u64([1, 2]), None, _stream()) == -1
    assert L.lfi_row_rng_seed_rows(st.ptr, 5, 2, _ints([1, 1]), _u64([1, 2]), None, _stream()) == -1
    assert L.lfi_row_rng_load_rows(st.ptr, 5, 2, _ints([1, 2]), _ints([0, 2]), 2, st.ptr, None, _stream()) == -1
    st.check()
