"""CPU: keyed sampling noise per conversation (open_stream(row_seeds=...)) without a device - the C ABI's three row-state entry
points against their declarations, the key helper, the position rules as one pure function against a literal copy of DESIGN.md
section 16's table, the refusals a session makes before any launch, and StreamRows.rng through its round trips."""
import io
import os
from argparse import Namespace

import pytest
import torch

from lets_face_it_amd import _lib
from lets_face_it_amd import stream as S
from lets_face_it_amd.engine import StreamRows
from lets_face_it_amd.glow.models import SeqGlow
from test_stream_candidates_cpu import _declaration, _stub_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = (16, 8, 2, "gru", False, (("p2_face", 3, 16),), 2, 3 * 16 + 3 * 16 + 2 * 8)


def test_row_state_entry_points_are_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "lfi.h")).read()
    assert _declaration(text, "lfi_row_rng_seed_rows") == ("unsigned long long* rng, int B, int nrows, const int* rows, "
                                                           "const unsigned long long* keys, const unsigned long long* positions, "
                                                           "void* stream")
    assert _declaration(text, "lfi_row_rng_save_rows") == ("const unsigned long long* rng, int B, int nrows, const int* rows, "
                                                           "unsigned long long* out, void* stream")
    assert _declaration(text, "lfi_row_rng_load_rows") == ("unsigned long long* rng, int B, int nrows, const int* rows, "
                                                           "const int* entries, int nsaved, const unsigned long long* saved, "
                                                           "const unsigned long long* keys, void* stream")
    L = _lib.lib()
    C = _lib.C
    vp, i, pi, pk = C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)
    assert L.lfi_row_rng_seed_rows.argtypes == [vp, i, i, pi, pk, pk, vp]
    assert L.lfi_row_rng_save_rows.argtypes == [vp, i, i, pi, vp, vp]
    assert L.lfi_row_rng_load_rows.argtypes == [vp, i, i, pi, pi, i, vp, pk, vp]
    for name in ("lfi_row_rng_seed_rows", "lfi_row_rng_save_rows", "lfi_row_rng_load_rows"):
        assert name in _lib.EXPORTS and getattr(L, name).restype == i


def test_row_state_argument_errors_come_before_any_launch():
    """No device here: every call below must return from the host checks. The state's address is a host array standing in for a
    device pointer that is never dereferenced."""
    L = _lib.lib()
    C = _lib.C
    words = (C.c_ulonglong * 16)()
    rng = C.addressof(words)
    rows, twice, far = (C.c_int * 2)(4, 0), (C.c_int * 2)(3, 3), (C.c_int * 2)(0, 5)
    ents, keys = (C.c_int * 2)(0, 0), (C.c_ulonglong * 2)(1, 2)
    # all null
    assert L.lfi_row_rng_seed_rows(None, 0, 0, None, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_row_rng_save_rows(None, 0, 0, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    assert L.lfi_row_rng_load_rows(None, 0, 0, None, None, 0, None, None, None) == -1
    assert b"null pointer" in L.lfi_last_error()
    # partly null
    assert L.lfi_row_rng_seed_rows(None, 5, 2, rows, keys, None, None) == -1
    assert L.lfi_row_rng_save_rows(rng, 5, 2, None, rng, None) == -1 and b"rows" in L.lfi_last_error()
    assert L.lfi_row_rng_save_rows(rng, 5, 2, rows, None, None) == -1 and b"out" in L.lfi_last_error()
    assert L.lfi_row_rng_load_rows(rng, 5, 2, None, ents, 1, rng, None, None) == -1 and b"rows" in L.lfi_last_error()
    assert L.lfi_row_rng_load_rows(rng, 5, 2, rows, None, 1, rng, None, None) == -1 and b"entries" in L.lfi_last_error()
    assert L.lfi_row_rng_load_rows(rng, 5, 2, rows, ents, 1, None, keys, None) == -1 and b"saved" in L.lfi_last_error()
    # misaligned state, negative sizes, indices out of range, a row twice
    assert L.lfi_row_rng_seed_rows(rng + 4, 5, 2, rows, keys, None, None) == -1 and b"misaligned" in L.lfi_last_error()
    for B, n in ((-1, 0), (5, -1)):
        assert L.lfi_row_rng_seed_rows(rng, B, n, None, None, None, None) == -1 and b"negative" in L.lfi_last_error()
        assert L.lfi_row_rng_save_rows(rng, B, n, rows, rng, None) == -1 and b"negative" in L.lfi_last_error()
        assert L.lfi_row_rng_load_rows(rng, B, n, rows, ents, 1, rng, None, None) == -1 and b"negative" in L.lfi_last_error()
    assert L.lfi_row_rng_load_rows(rng, 5, 2, rows, ents, -1, rng, None, None) == -1 and b"negative" in L.lfi_last_error()
    assert L.lfi_row_rng_seed_rows(rng, 5, 6, None, None, None, None) == -1 and b"6 rows listed for a batch of 5" in L.lfi_last_error()
    for call in (lambda r: L.lfi_row_rng_seed_rows(rng, 5, 2, r, keys, None, None), lambda r: L.lfi_row_rng_save_rows(rng, 5, 2, r, rng, None),
                 lambda r: L.lfi_row_rng_load_rows(rng, 5, 2, r, ents, 1, rng, None, None)):
        assert call(twice) == -1 and b"row 3 is listed twice" in L.lfi_last_error()
        assert call(far) == -1 and b"outside the batch (0 .. 4)" in L.lfi_last_error()
    for bad in ((C.c_int * 2)(0, 1), (C.c_int * 2)(-1, 0)):
        assert L.lfi_row_rng_load_rows(rng, 5, 2, rows, bad, 1, rng, None, None) == -1
        assert b"outside the saved rows (0 .. 0)" in L.lfi_last_error()
    # nothing listed: OK without a launch
    assert L.lfi_row_rng_seed_rows(rng, 5, 0, None, None, None, None) == 0
    assert L.lfi_row_rng_save_rows(rng, 5, 0, None, None, None) == 0
    assert L.lfi_row_rng_load_rows(rng, 5, 0, None, None, 0, None, None, None) == 0
    assert all(w == 0 for w in words)


def test_key_helper_round_trip_and_refusals():
    for key, word in ((0, 0), (1, 1), (2 ** 63 - 1, 2 ** 63 - 1), (2 ** 63, -2 ** 63), (2 ** 64 - 1, -1)):
        assert S.key_to_word(key) == word and S.word_to_key(word) == key
        assert S.word_to_key(torch.tensor([word], dtype=torch.int64)[0]) == key          # (what row_rng() hands back)
    keys = [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1]
    assert S.row_keys(keys, 5) == keys
    assert S.row_keys(tuple(keys), 5) == keys
    assert S.row_keys([7, 7, 7], 3) == [7, 7, 7]                                         # keys may repeat
    # a CPU integer tensor is taken as bit patterns
    assert S.row_keys(torch.tensor([0, 1, 2 ** 63 - 1, -2 ** 63, -1], dtype=torch.int64), 5) == keys
    assert S.row_keys(torch.tensor([3, 4], dtype=torch.int32), 2) == [3, 4]
    for bad in ([-1, 0], [0, 2 ** 64]):
        with pytest.raises(ValueError, match=r"row_seeds: -?\d+ outside \[0, 2\*\*64\)"):
            S.row_keys(bad, 2)
    for bad in ([True, 0], [1.0, 2], [0.5, 2], ["a", 1], 5, torch.tensor([1.0, 2.0]), torch.tensor([True, False]),
                torch.zeros(2, 1, dtype=torch.int64), torch.tensor(3)):
        with pytest.raises(ValueError, match="row_seeds: expected a sequence of ints or a 1-D CPU integer tensor"):
            S.row_keys(bad, 2)
    for bad in ([1, 2, 3], [1], torch.tensor([1, 2, 3])):
        with pytest.raises(ValueError, match=r"row_seeds: \d listed for 2 rows"):
            S.row_keys(bad, 2)
    with pytest.raises(ValueError, match="row_seeds: expected a sequence of ints or a 1-D CPU integer tensor"):
        S.row_keys(_FakeCuda(), 2)                                                       # a CUDA tensor: host data is wanted
    for bad in (True, 1.0, "1", None):
        with pytest.raises(ValueError, match="row_seeds: expected ints"):
            S.key_to_word(bad)


class _FakeCuda(torch.Tensor):
    """A tensor that says it lives on a GPU (there is none here): what the helper looks at before anything else."""

    @staticmethod
    def __new__(cls):
        return torch.Tensor._make_subclass(cls, torch.zeros(2, dtype=torch.int64))

    @property
    def is_cuda(self):
        return True


# DESIGN.md section 16, "Position rules", copied literally: (kind of call, n, lengths) -> what every row's position moves by
TABLE = [
    ("step", 1, None, 1), ("observe", 1, None, 1), ("step_rows", 1, None, 1),
    ("step_many", 5, None, 5), ("observe_many", 5, None, 5), ("step_rows_many", 5, None, 5),
    ("step_many", 1, None, 1), ("observe_many", 7, [3, 0, 7, 1], [3, 0, 7, 1]),
    ("step_candidates", 1, None, 0), ("commit", 1, None, 1),
    ("rollout_candidates", 6, None, 0), ("commit", 6, None, 6), ("discard", 6, None, 0), ("reset", 1, None, 0),
]


def _walk(script, B):
    pos = [0] * B
    for kind, n, lens in script:
        move = S.row_position_advance(kind, n, lens)
        pos = [p + (move[r] if isinstance(move, list) else move) for r, p in enumerate(pos)]
    return pos


def test_position_function_is_the_design_table():
    for kind, n, lens, want in TABLE:
        assert S.row_position_advance(kind, n, lens) == want, (kind, n, lens)
    # the function takes no noise argument: a frame taken with the caller's noise= moves the position as a drawn one does
    assert S.row_position_advance("step") == S.row_position_advance("step", 1) == 1
    # candidates then commit: + 1 in total; rollouts then discard: + 0; rollouts then commit: + n; ragged with a 0
    assert _walk([("step_candidates", 1, None), ("commit", 1, None)], 3) == [1, 1, 1]
    assert _walk([("rollout_candidates", 4, None), ("discard", 4, None)], 3) == [0, 0, 0]
    assert _walk([("rollout_candidates", 4, None), ("commit", 4, None)], 3) == [4, 4, 4]
    assert _walk([("step", 1, None), ("observe_many", 4, [2, 0, 4]), ("step_rows_many", 3, None), ("step_candidates", 1, None),
                  ("reset", 1, None)], 3) == [6, 4, 8]
    with pytest.raises(ValueError, match="not a kind of session call"):
        S.row_position_advance("save_rows")
    with pytest.raises(ValueError, match="only observe_many takes lengths"):
        S.row_position_advance("step_many", 3, [1, 2])
    with pytest.raises(ValueError, match=r"lengths \[4\] outside 0 \.\. 3"):
        S.row_position_advance("observe_many", 3, [1, 4])
    for bad in (-1, True, 1.5):
        with pytest.raises(ValueError, match="not a frame count"):
            S.row_position_advance("step_many", bad)


def _rows(n=3, rng=True):
    data = torch.arange(n * SIG[-1], dtype=torch.float32).view(n, SIG[-1])
    words = torch.tensor([[S.key_to_word(2 ** 63 + r), 10 * r] for r in range(n)], dtype=torch.int64)
    return StreamRows(data, SIG, rng=words if rng else None)


def test_a_session_refuses_keyed_arguments_it_cannot_honour_before_any_launch():
    st = _stub_session()
    st.row_signature = SIG
    seed = {"p1_face": torch.zeros(3, 4, 16)}
    assert st.rng is None
    # row_seeds on an unkeyed session
    with pytest.raises(ValueError, match="row_seeds: the session was opened without row_seeds"):
        st.reset_rows([0, 2], seed, row_seeds=[1, 2])
    with pytest.raises(ValueError, match="row_seeds: the session was opened without row_seeds"):
        st.load_rows([0], _rows(), row_seeds=[1])
    with pytest.raises(ValueError, match="row_seeds: the session was opened without row_seeds"):
        st.row_rng()
    st._check_seed = lambda seed, B=None: None          # (the stub has no engine to check a seed against)
    with pytest.raises(ValueError, match="row_seeds: the session was opened without row_seeds"):
        st.reset(seed, row_seeds=[1, 2, 3])
    # a keyed session (the state is never touched: every call below is refused first)
    st.rng = torch.zeros(3, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="the rows carry no keyed-noise state"):
        st.load_rows([0, 1], _rows(rng=False))
    with pytest.raises(ValueError, match=r"row_seeds: 1 listed for 2 rows"):
        st.load_rows([0, 1], _rows(rng=False), row_seeds=[5])
    with pytest.raises(ValueError, match=r"row_seeds: -1 outside"):
        st.reset_rows([0, 1], seed, row_seeds=[5, -1])
    with pytest.raises(ValueError, match="saved.rng: expected a contiguous int64 tensor"):
        st.load_rows([0, 1], _rows())                   # (rows paused on the host: to(device) comes first)
    assert torch.equal(st.rng, torch.zeros(3, 2, dtype=torch.int64))


def test_inference_refuses_noise_together_with_row_seeds():
    with pytest.raises(ValueError, match="noise and row_seeds are both given"):
        SeqGlow.inference(Namespace(), 30, {}, noise=torch.zeros(6, 2, 16), row_seeds=[1, 2])


def test_stream_rows_carry_rng_through_every_round_trip():
    rows = _rows()
    assert rows.rng.dtype == torch.int64 and tuple(rows.rng.shape) == (3, 2)
    buf = io.BytesIO()
    torch.save(rows.state_dict(), buf)
    buf.seek(0)
    back = StreamRows.from_state_dict(torch.load(buf))
    assert torch.equal(back.rng, rows.rng) and torch.equal(back.data, rows.data) and back.signature == rows.signature
    sel = rows.select([2, 0, 2])
    assert torch.equal(sel.rng, rows.rng[[2, 0, 2]]) and torch.equal(sel.data, rows.data[[2, 0, 2]])
    assert [S.word_to_key(w) for w in sel.rng[:, 0]] == [2 ** 63 + 2, 2 ** 63, 2 ** 63 + 2]
    for moved in (rows.cpu(), rows.to("cpu"), rows._like(rows.data, rows.rng)):
        assert torch.equal(moved.rng, rows.rng)
    # without rng: the key is absent from the state dict, and a state dict without it loads (rows stored before the keys existed)
    plain = _rows(rng=False)
    d = plain.state_dict()
    assert "rng" not in d and set(d) == set(S._ROW_FIELDS) | {"data"}
    old = StreamRows.from_state_dict(d)
    assert old.rng is None and old.select([1]).rng is None and old.cpu().rng is None and old.to("cpu").rng is None
    assert "rng" in rows.state_dict() and set(rows.state_dict()) == set(d) | {"rng"}
    for bad in (torch.zeros(3, 2), torch.zeros(2, 2, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), [[0, 0]] * 3):
        with pytest.raises(ValueError, match="StreamRows: rng: expected an int64 tensor"):
            StreamRows(rows.data, SIG, rng=bad)
