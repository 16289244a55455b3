"""GPU: the chunk window launches through the C ABI - all seven entry points over the one kernel pair (lfi_stream.hip:
stream_chunk_in_kernel / stream_chunk_out_kernel) - against a torch restatement of the copies.

The kernels copy and take a max, so every comparison is torch.equal and the guard word is the exact max |v| of the values that are
read: there is no tolerance. Every slot that must not be read holds NaN (a NaN that is read shows in the guard word, whose bits are
above every finite value's), and every buffer that is written starts from a sentinel, so a write too many shows too.

B = 3, start = 4; windows (hist, dim, lead): a conditioning window with a frame in front of it, one whose 300 floats per frame take
more than one pass of the 256-thread loops, and the faces window with hist - lead == start; n below, between and above the hists."""
import pytest
import torch

from lets_face_it_amd import _lib

pytestmark = pytest.mark.gpu

B, START, SENTINEL = 3, 4, 7.0
SHAPES = ((3, 5, 0), (2, 300, 0), (START + 1, 6, 1))
GEN = 2                 # the faces window: the one a chain writes
C_ = SHAPES[GEN][1]
NS = (1, 2, 5)


def _tab(ts):
    return (_lib.C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _ints(i):
    return (_lib.C.c_int * len(SHAPES))(*[s[i] for s in SHAPES])


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _guard_value(guard):
    return guard.view(torch.float32).item()


class _Case:
    """Windows, the chunk's frames, sentinel-filled sequences, a guard word and the counters, for n frames."""

    def __init__(self, n, dev, seed=11):
        g = torch.Generator().manual_seed(seed + n)
        self.n, self.dev = n, dev
        self.wins = [torch.randn(B, h, d, generator=g).to(dev) for h, d, _ in SHAPES]
        self.srcs = [torch.randn(B, n, d, generator=g) for _, d, _ in SHAPES]       # (host: the tests poke NaN in, then .to(dev))
        self.noise = torch.randn(n, B, C_, generator=g)
        self.made = torch.randn(B, n, C_, generator=g).to(dev)                       # what a chain would write
        self.seqs = [torch.full((B, START + n, d), SENTINEL, device=dev) for _, d, _ in SHAPES]
        self.guard = torch.zeros(1, dtype=torch.int32, device=dev)
        self.frame_nb = torch.tensor([3.0, 5.0, 7.0], device=dev)

    def head(self):
        return B, self.n, START, len(SHAPES), _tab(self.wins)

    def tabs(self):
        return _ints(0), _ints(1), _ints(2)


def _want_in(case, srcs, lens=None, gen=-1, noise=None, roles=None):
    """The sequences and the guard value the in-launch must leave: live frames, then each row's frames (zeros behind its length); the
    generated window keeps its slots except where the row observes."""
    n, amax, want = case.n, 0.0, []
    for i, ((h, d, lead), win, src) in enumerate(zip(SHAPES, case.wins, srcs)):
        w = torch.full((B, START + n, d), SENTINEL, device=case.dev)
        w[:, START - (h - lead):START] = win[:, lead:]
        for b in range(B):
            if i != gen:
                v = n if lens is None else lens[b]
                w[b, START:START + v] = src[b, :v]
                w[b, START + v:] = 0.0
                if v:
                    amax = max(amax, src[b, :v].abs().max().item())
                continue
            for f in range(n):
                if roles is not None and roles[f][b]:
                    w[b, START + f] = src[b, f]
                    amax = max(amax, src[b, f].abs().max().item())
                else:
                    amax = max(amax, noise[f, b].abs().max().item())
        want.append(w)
    return want, amax


def _want_out(case, lens=None):
    """The windows and counters the out-launch must leave: the hist frames that end at each row's length; a row of length 0 as it was."""
    wins, nb = [w.clone() for w in case.wins], case.frame_nb.clone()
    for b in range(B):
        v = case.n if lens is None else lens[b]
        if v:
            for (h, _, _), w, seq in zip(SHAPES, wins, case.seqs):
                w[b] = seq[b, START + v - h:START + v]
            nb[b] += 2.0 * v
    return wins, nb


def _check_in(case, want, amax, tag):
    for i, (seq, w) in enumerate(zip(case.seqs, want)):
        assert torch.equal(seq, w), (tag, "sequence", i)
    assert _guard_value(case.guard) == amax, (tag, _guard_value(case.guard), amax)


def _check_out(case, want_wins, want_nb, tag):
    for i, (win, w) in enumerate(zip(case.wins, want_wins)):
        assert torch.equal(win, w), (tag, "window", i)
    assert torch.equal(case.frame_nb, want_nb), (tag, case.frame_nb.tolist(), want_nb.tolist())


def _run_plain(case, srcs, lens=None):
    """chunk_in / chunk_out, or their _rows forms with lengths, each checked against the restatement."""
    L = _lib.lib()
    tag = "dense" if lens is None else "ragged %s" % (lens,)
    want, amax = _want_in(case, srcs, lens)
    if lens is None:
        _lib.check(L.lfi_stream_chunk_in(*case.head(), _tab(srcs), _tab(case.seqs), *case.tabs(), case.guard.data_ptr(), _stream()),
                   "lfi_stream_chunk_in")
    else:
        lengths = torch.tensor(lens, dtype=torch.int32, device=case.dev)
        _lib.check(L.lfi_stream_chunk_in_rows(*case.head(), _tab(srcs), _tab(case.seqs), *case.tabs(), case.guard.data_ptr(),
                                              lengths.data_ptr(), _stream()), "lfi_stream_chunk_in_rows")
    _check_in(case, want, amax, tag)
    want_wins, want_nb = _want_out(case, lens)
    if lens is None:
        _lib.check(L.lfi_stream_chunk_out(*case.head(), _tab(case.seqs), *case.tabs(), case.frame_nb.data_ptr(), _stream()),
                   "lfi_stream_chunk_out")
    else:
        _lib.check(L.lfi_stream_chunk_out_rows(*case.head(), _tab(case.seqs), *case.tabs(), case.frame_nb.data_ptr(),
                                               lengths.data_ptr(), _stream()), "lfi_stream_chunk_out_rows")
    _check_out(case, want_wins, want_nb, tag)


@pytest.mark.parametrize("n", NS)
def test_the_dense_and_the_ragged_pair_against_a_torch_restatement(n, gpu_device):
    dense = _Case(n, gpu_device)
    _run_plain(dense, [s.to(gpu_device) for s in dense.srcs])
    assert dense.frame_nb.tolist() == [3.0 + 2 * n, 5.0 + 2 * n, 7.0 + 2 * n]
    # ragged: NaN behind every length
    lens = [0, 1, n]
    ragged = _Case(n, gpu_device)
    srcs = [s.clone() for s in ragged.srcs]
    for s in srcs:
        for b, v in enumerate(lens):
            s[b, v:] = float("nan")
    _run_plain(ragged, [s.to(gpu_device) for s in srcs], lens)
    assert ragged.frame_nb.tolist() == [3.0, 5.0 + 2.0, 7.0 + 2.0 * n]
    # all lengths n is the dense pair: sequences, windows, counters and guard word
    full = _Case(n, gpu_device)
    _run_plain(full, [s.to(gpu_device) for s in full.srcs], [n] * B)
    for a, b in zip(dense.seqs + dense.wins + [dense.frame_nb, dense.guard], full.seqs + full.wins + [full.frame_nb, full.guard]):
        assert torch.equal(a, b)


def _gen_out(case, tag):
    """chunk_gen_out behind a chain's writes: the windows back, the counters, the n fresh frames into a pitched `out`, folded."""
    L, n = _lib.lib(), case.n
    pitch = n * C_ + 5
    out = torch.full((B, pitch), SENTINEL, device=case.dev)
    want_wins, want_nb = _want_out(case)
    fresh = case.seqs[GEN][:, START:].reshape(B, n * C_).clone()
    case.guard.zero_()
    _lib.check(L.lfi_stream_chunk_gen_out(*case.head(), _tab(case.seqs), *case.tabs(), GEN, out.data_ptr(), pitch,
                                          case.frame_nb.data_ptr(), case.guard.data_ptr(), _stream()), "lfi_stream_chunk_gen_out")
    _check_out(case, want_wins, want_nb, tag)
    assert torch.equal(out[:, :n * C_], fresh), tag
    assert torch.equal(out[:, n * C_:], torch.full((B, 5), SENTINEL, device=case.dev)), (tag, "padding")
    assert _guard_value(case.guard) == fresh.abs().max().item(), tag
    assert case.frame_nb.tolist() == [3.0 + 2 * n, 5.0 + 2 * n, 7.0 + 2 * n]


@pytest.mark.parametrize("given", ("no source", "a source of NaN"))
@pytest.mark.parametrize("n", NS)
def test_the_generating_pair_against_a_torch_restatement(n, given, gpu_device):
    L = _lib.lib()
    case = _Case(n, gpu_device)
    srcs = [s.to(gpu_device) for s in case.srcs]
    srcs[GEN] = None if given == "no source" else torch.full_like(srcs[GEN], float("nan"))     # never read
    noise = case.noise.to(gpu_device)
    want, amax = _want_in(case, srcs, gen=GEN, noise=noise)
    _lib.check(L.lfi_stream_chunk_gen_in(*case.head(), _tab(srcs), _tab(case.seqs), *case.tabs(), GEN, noise.data_ptr(), C_,
                                         case.guard.data_ptr(), _stream()), "lfi_stream_chunk_gen_in")
    _check_in(case, want, amax, "gen_in")
    assert torch.equal(case.seqs[GEN][:, START:], torch.full((B, n, C_), SENTINEL, device=gpu_device))      # the chain's to write
    case.seqs[GEN][:, START:] = case.made
    _gen_out(case, "gen_out")


@pytest.mark.parametrize("n", NS)
def test_the_roles_pair_against_a_torch_restatement(n, gpu_device):
    L = _lib.lib()
    case = _Case(n, gpu_device)
    observed = torch.tensor([[True, False, f % 2 == 0] for f in range(n)])      # (n, B): all observe, all generate, alternating
    srcs = [s.clone() for s in case.srcs]
    srcs[GEN][~observed.t()] = float("nan")                                     # given faces at generating slots: never read
    noise = case.noise.clone()
    noise[observed] = float("nan")                                              # noise at observing slots: never read
    srcs, noise = [s.to(gpu_device) for s in srcs], noise.to(gpu_device)
    roles = observed.to(torch.int32).to(gpu_device)
    want, amax = _want_in(case, srcs, gen=GEN, noise=noise, roles=observed.tolist())
    _lib.check(L.lfi_stream_chunk_roles_in(*case.head(), _tab(srcs), _tab(case.seqs), *case.tabs(), GEN, noise.data_ptr(), C_,
                                           roles.data_ptr(), case.guard.data_ptr(), _stream()), "lfi_stream_chunk_roles_in")
    _check_in(case, want, amax, "roles_in")
    # the rows chain writes the generating slots only
    generating = ~observed.t().to(gpu_device)
    case.seqs[GEN][:, START:][generating] = case.made[generating]
    assert torch.isfinite(case.seqs[GEN][:, START:]).all()
    _gen_out(case, "gen_out behind roles_in")
