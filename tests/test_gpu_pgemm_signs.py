"""GPU: sign words of a planes matrix (include/lfi.h) and the persistent tile loop of the in-place dpre product.

The cond_transform forward product (gemm_epilogue_direct16<3>) writes one bit per element of c - (hi plane value > 0) - beside c's
planes; the dpre product (gemm_epilogue_direct16<4>) takes its LeakyReLU-gradient mask from those bits instead of reading the hi
plane of c back. LFI_PGEMM_SIGNS=0 / LFI_PGEMM_PERSIST=0 are the paths without either; every comparison here is bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(gpu_device):
    from argparse import Namespace
    from helpers import Fixture
    from lets_face_it_amd.engine import GlowEngine, ModelSpec
    return GlowEngine(ModelSpec(Namespace(**Fixture("tiny").hp)), gpu_device)


# ---- the format of include/lfi.h, "sign words of a planes matrix", on the host
def _word_and_bit(rows, cols):
    """(word index, bit) of every element of the rows x cols matrix, rows and cols multiples of 64."""
    r = np.arange(rows, dtype=np.int64)[:, None]
    c = np.arange(cols, dtype=np.int64)[None, :]
    word = ((r >> 6) * (cols >> 6) + (c >> 6)) * 64 + (r & 15) + 16 * ((c >> 2) & 3)
    bit = 16 * ((r >> 4) & 3) + 4 * ((c >> 4) & 3) + (c & 3)
    return word, np.broadcast_to(bit, word.shape)


def unpack_signs(words, rows, cols):
    """-> bool (rows_pad, cols_pad): the bit of every element of the padded matrix."""
    R, Cc = (rows + 63) // 64 * 64, (cols + 63) // 64 * 64
    word, bit = _word_and_bit(R, Cc)
    w = words.cpu().numpy().view(np.uint64)
    return ((w[word] >> bit.astype(np.uint64)) & np.uint64(1)).astype(bool)


def pack_signs(pos):
    """bool (rows, cols) -> int64 tensor of sign words of the matrix (padding bits 0)."""
    rows, cols = pos.shape
    R, Cc = (rows + 63) // 64 * 64, (cols + 63) // 64 * 64
    full = np.zeros((R, Cc), dtype=np.uint64)
    full[:rows, :cols] = pos
    word, bit = _word_and_bit(R, Cc)
    out = np.zeros(R * Cc // 64, dtype=np.uint64)
    np.bitwise_or.at(out, word.ravel(), (full << bit.astype(np.uint64)).ravel())
    return torch.from_numpy(out.view(np.int64))


def hi_plane(planes, M, nkt):
    """The hi plane's values of the (row tiles that exist of the) matrix a planes buffer holds -> float (Mpad32, 16 nkt), by the
    block format of lfi_planes_from_f32: block (rt, ct), row l & 31, chunk l >> 5 at lfi_u_plane_offset (chunks swapped in rows
    8-15 and 24-31)."""
    nrt = (M + 31) // 32
    blk = planes[:nrt * nkt * 1024].view(nrt, nkt, 2, 32, 2, 8)[:, :, 0].float().cpu()   # (rt, ct, row, chunk slot, 8)
    row = torch.arange(32)
    swap = ((row >> 3) & 1).bool()                                                           # rows 8-15, 24-31
    lo = torch.where(swap[None, None, :, None], blk[:, :, :, 1], blk[:, :, :, 0])           # columns 0-7 of the block
    hi = torch.where(swap[None, None, :, None], blk[:, :, :, 0], blk[:, :, :, 1])           # columns 8-15
    full = torch.cat([lo, hi], dim=-1)                                                       # (rt, ct, 32, 16)
    return full.permute(0, 2, 1, 3).reshape(nrt * 32, nkt * 16)


def test_hi_plane_reader_of_this_file(eng, gpu_device):
    """(the helper above against lfi_planes_from_f32 itself: every later check leans on it)"""
    X = torch.randn(70, 96, generator=torch.Generator().manual_seed(1)).to(gpu_device)
    Xp, nk = eng.planes("test.sx", X, 96, 70, 96)
    torch.cuda.synchronize()
    assert torch.equal(hi_plane(Xp, 70, nk)[:70, :96], X.bfloat16().float().cpu())


@pytest.mark.parametrize("M,N,K,zero_rows", [(40, 64, 32, False), (130, 192, 64, True), (700, 512, 96, False)])
@pytest.mark.parametrize("hi_only", [False, True])
def test_forward_product_writes_sign_words(eng, gpu_device, M, N, K, hi_only, zero_rows):
    """Writer: planes out + sign words, bias and LeakyReLU. The words, unpacked by the header's formula, equal (hi plane as float) > 0
    inside M x N and are 0 in the padding of existing patches; the planes are those of a run without a sign buffer, bit for bit.
    zero_rows: a block of all-zero rows of A, so that the result there is the bias alone - exact values, among them columns with
    bias < 0 and bias == 0 (a LeakyReLU output of exactly 0: not positive)."""
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g)
    if zero_rows:
        A[32:96] = 0.0
        bias[::5] = 0.0
    A, W, bias = A.to(gpu_device), W.to(gpu_device), bias.to(gpu_device)
    Ap, nka = eng.planes("test.pa", A, K, M, K)
    Wp, nkw = eng.planes("test.pw", W, K, N, K)
    nkr = N // 16
    n_el = eng.L.lfi_planes_elems(M, N)
    nw = eng.L.lfi_planes_sign_words(M, N)
    assert nw == ((M + 63) // 64) * ((N + 63) // 64) * 64
    kw = dict(bias=bias, act=1, store=False, cr_nkt=nkr, hi_only=hi_only, tile=1)   # (128 x 256 tiles: the writer's; see _dpre)
    plain = torch.full((n_el,), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, N, Cr=plain, **kw)
    Cr = torch.full((n_el,), float("nan"), dtype=torch.bfloat16, device=gpu_device)
    words = torch.full((nw + 64,), -1, dtype=torch.int64, device=gpu_device)
    assert eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, N, Cr=Cr, sign_out=words, signs_query=True, **kw)
    eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, N, Cr=Cr, sign_out=words, **kw)
    torch.cuda.synchronize()
    assert torch.equal(Cr.view(torch.int16), plain.view(torch.int16))
    assert bool((words[nw:] == -1).all()), "wrote past lfi_planes_sign_words"
    got = unpack_signs(words[:nw], M, N)
    hi = hi_plane(Cr, M, nkr)
    want = np.zeros_like(got)
    want[:M, :N] = (hi[:M, :N] > 0).numpy()
    print("sign words %d x %d: %d bits set of %d inside, %d outside" % (M, N, int(got[:M, :N].sum()), M * N,
                                                                        int(got.sum()) - int(got[:M, :N].sum())))
    assert np.array_equal(got, want)
    if zero_rows:
        b = bias.cpu()
        assert bool((b == 0).any()) and bool((b < 0).any())
        assert not got[40, :N][(b <= 0).numpy()].any() and got[40, :N][(b > 0).numpy()].all()


def test_sign_words_are_refused_where_no_kernel_honours_them(eng, gpu_device, monkeypatch):
    """A sign buffer on a product that cannot take it is an error, not a silent no-op: fp32 rows stored too (through-LDS epilogue),
    a plane matrix that is not whole 64-column patches, LFI_PGEMM_SIGNS=0."""
    from lets_face_it_amd import _lib
    M, N, K = 40, 96, 32
    A = torch.randn(M, K).to(gpu_device)
    W = torch.randn(N, K).to(gpu_device)
    Ap, nka = eng.planes("test.pa", A, K, M, K)
    Wp, nkw = eng.planes("test.pw", W, K, N, K)
    Cr = torch.zeros(eng.L.lfi_planes_elems(M, 128), dtype=torch.bfloat16, device=gpu_device)
    words = torch.zeros(eng.L.lfi_planes_sign_words(M, 128), dtype=torch.int64, device=gpu_device)
    out = torch.zeros(M, N, device=gpu_device)
    cases = [dict(Cm=out, store=True, cr_nkt=8), dict(Cm=None, store=False, cr_nkt=6)]
    for c in cases:
        kw = dict(act=1, store=c["store"], Cr=Cr, cr_nkt=c["cr_nkt"], sign_out=words, tile=1)
        assert not eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, c["Cm"], N, signs_query=True, **kw)
        with pytest.raises(_lib.LfiError):
            eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, c["Cm"], N, **kw)
    ok = dict(act=1, store=False, Cr=Cr, cr_nkt=8, sign_out=words, tile=1)
    assert eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, N, signs_query=True, **ok)
    assert not eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, N, signs_query=True, **dict(ok, tile=2))   # 256 x 128 tiles: no writer
    monkeypatch.setenv("LFI_PGEMM_SIGNS", "0")
    assert not eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, N, signs_query=True, **ok)
    with pytest.raises(_lib.LfiError):
        eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, N, **ok)
    torch.cuda.synchronize()


def _dpre(eng, dev, M, N, K, batch, signs, seed, grid=None):
    """One run of the in-place dpre product on FRESH buffers (operands, planes of c, sums: nothing is warm in L2 from a run before).
    signs: mask from sign words (packed on the host from the same c) or from the hi plane of c's planes. -> (hi planes, sums)
    (tile = 1 pins the 128 x 256 tile, the dpre kernel's: left to itself the library gives an N of 64 the 256 x 128 one.)
    grid: a list that receives the workgroups of the persistent launch this run gets (0: one workgroup per tile)."""
    g = torch.Generator().manual_seed(seed)
    Ncols = batch * N
    A = torch.randn(M, batch * K, generator=g).to(dev)
    W = torch.randn(batch * K, N, generator=g).to(dev)
    Gm = torch.randn(M, Ncols, generator=g)
    tag = "%d.%d" % (seed, int(signs))
    Ap, nka = eng.planes("test.sa" + tag, A, batch * K, M, batch * K)
    Wp, nkw = eng.planes("test.sw" + tag, W, N, batch * K, N)
    Gp, nkg = eng.planes("test.sg" + tag, Gm.to(dev), Ncols, M, Ncols)
    words = pack_signs((Gm.bfloat16().float() > 0).numpy()).to(dev) if signs else None
    sums = torch.zeros(Ncols, device=dev)
    kw = dict(act=2, slope=0.01, batch=batch, b_fmt=1, a_stride=(K // 16) * 1024, b_stride=(K // 32) * nkw * 1024, sC=N,
              store=False, Cr=Gp, cr_nkt=nkg, hi_only=True, colsum_into=sums, cls="t", tile=1)
    if signs:
        kw["sign_in"] = words
    else:
        kw.update(Gr=Gp, gr_nkt=nkg)
    eng.pass_skip = {"t": 1}
    try:
        if signs:
            assert eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, Ncols, signs_query=True, **kw)
        if grid is not None:
            grid.append(eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, Ncols, persist_query=True, **kw))
        assert eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, Ncols, **kw)
    finally:
        eng.pass_skip = {}
    torch.cuda.synchronize()
    nblk = (M + 31) // 32 * nkg
    hi = Gp[:nblk * 1024].view(-1, 2, 512)[:, 0].view(torch.int16).clone()
    for name in ("test.sa", "test.sw", "test.sg"):
        eng._ws.pop(name + tag, None)
    return hi, sums


@pytest.mark.parametrize("M,N,K,batch", [(333, 64, 96, 2), (700, 512, 384, 1), (64, 64, 32, 3)])
def test_dpre_mask_from_sign_words_matches_mask_from_planes(eng, gpu_device, monkeypatch, M, N, K, batch):
    """Reader: the same lanes apply the same predicate to the same elements, only from one 8-byte word per lane instead of sixteen
    8-byte loads on c's hi plane: hi planes bit for bit, column sums torch.equal (same lanes, same order)."""
    seed = M + N + K + batch
    hs, ss = _dpre(eng, gpu_device, M, N, K, batch, True, seed)
    monkeypatch.setenv("LFI_PGEMM_SIGNS", "0")
    hp, sp = _dpre(eng, gpu_device, M, N, K, batch, False, seed)
    assert torch.equal(hs, hp)
    assert torch.equal(ss, sp)


@pytest.fixture(scope="module")
def persist_ref(eng, gpu_device):
    """(M, N, K, batch, signs) -> (hi planes, sums) of the dpre product with one workgroup per tile (LFI_PGEMM_PERSIST=0): computed
    once per shape, shared by the workgroup counts of the test below and left unchanged."""
    import os
    cache = {}

    def get(M, N, K, batch, signs):
        key = (M, N, K, batch, signs)
        if key not in cache:
            saved = {k: os.environ.get(k) for k in ("LFI_PGEMM_PERSIST", "LFI_PGEMM_PERSIST_WGS")}
            os.environ["LFI_PGEMM_PERSIST"] = "0"
            os.environ.pop("LFI_PGEMM_PERSIST_WGS", None)
            try:
                cache[key] = _dpre(eng, gpu_device, M, N, K, batch, signs, M + N + K + batch)
            finally:
                for k, v in saved.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return cache[key]
    return get


@pytest.mark.parametrize("wgs", [1, 2, 3, 1000])
@pytest.mark.parametrize("signs", [True, False])
@pytest.mark.parametrize("M,N,K,batch", [(333, 64, 32, 2), (333, 64, 64, 2), (333, 64, 96, 2), (333, 64, 128, 2), (1000, 512, 128, 3)])
def test_dpre_persistent_tile_loop(eng, gpu_device, monkeypatch, persist_ref, M, N, K, batch, signs, wgs):
    """Persistent walk (LFI_PGEMM_PERSIST=1; LFI_PGEMM_PERSIST_WGS caps the grid: every tile on one workgroup, tile counts the grid
    does not divide, more workgroups than tiles) against one workgroup per tile (LFI_PGEMM_PERSIST=0): planes bit for bit, column
    sums torch.equal. (333, 64, K, 2) is 3 x 1 x 2 = 6 work items, (1000, 512, 128, 3) 8 x 2 x 3 = 48; K = 32 .. 128 is one to four
    pairs of k-tiles: the three ring slots through one wrap. Fresh operands for every run: the next item's prefetch finds nothing in
    L2. That the run under test is launched persistent with the grid asked for, and the reference is not, is asked of the library
    (lfi_gemm_planes_persist_grid: the launch path's own decision) and asserted."""
    seed = M + N + K + batch
    items = ((M + 127) // 128) * ((N + 255) // 256) * batch
    h0, s0 = persist_ref(M, N, K, batch, signs)
    monkeypatch.setenv("LFI_PGEMM_PERSIST", "1")
    monkeypatch.setenv("LFI_PGEMM_PERSIST_WGS", str(wgs))
    grid = []
    h1, s1 = _dpre(eng, gpu_device, M, N, K, batch, signs, seed, grid)
    assert grid == [min(wgs, items)], "not the persistent launch asked for: %r" % grid
    assert torch.equal(h1, h0)
    assert torch.equal(s1, s0)


def test_dpre_one_workgroup_per_tile_without_the_switch(eng, gpu_device, monkeypatch):
    """LFI_PGEMM_PERSIST=0 launches one workgroup per tile (grid query 0), =1 without a cap min(items, 2 x CUs) workgroups."""
    monkeypatch.setenv("LFI_PGEMM_PERSIST", "0")
    grid = []
    _dpre(eng, gpu_device, 333, 64, 96, 2, True, 7, grid)
    assert grid == [0]
    monkeypatch.setenv("LFI_PGEMM_PERSIST", "1")
    monkeypatch.delenv("LFI_PGEMM_PERSIST_WGS", raising=False)
    grid = []
    _dpre(eng, gpu_device, 333, 64, 96, 2, True, 7, grid)
    assert grid == [min(6, 2 * torch.cuda.get_device_properties(gpu_device).multi_processor_count)]


def test_whole_training_step_with_and_without_signs_and_persistence(gpu_device, monkeypatch):
    """One fused training step of a final_model-shaped model (K = 2 flow steps, two-product backward classes as at the benchmark's
    size: the dpre product then runs on the kernel that reads sign words) with both switches on against both off: the loss and
    every parameter after the step are bit for bit equal. B = 32, T = 25: engine._chain_ok asks a backward pass for F = N B a
    multiple of 32 and lfi_flow_bwd_emits_planes for B a multiple of 32; the longest history is 24 frames, so T = 25 (N = 1,
    F = 32) is the smallest such step - and that the chain is taken is asserted, not assumed."""
    import copy
    from argparse import Namespace
    from test_gpu_parity import final_model_hparams, to_dev
    from lets_face_it_amd.glow.lets_face_it_glow import LetsFaceItGlow
    from oracle import seqglow_oracle as oracle
    B, T = 32, 25
    hp = final_model_hparams(50, 27, K=2)
    hp["engine_precision"] = "bf16x3"
    hp["engine_backward_products"] = 2
    hp["Train"]["use_negative_nll_loss"] = False
    batch = to_dev(oracle.synthetic_batch(B, T, 50, 27, seed=3), gpu_device)
    g = torch.Generator().manual_seed(5)
    masks = {}
    for name in ("p2_face", "p1_speech", "p2_speech"):
        cfg = hp["Conditioning"][name]
        keep = 1.0 - cfg["dropout"]
        masks[name] = (torch.rand(T - 24, B, cfg["history"], generator=g) < keep).float() / keep
    outs = []
    for on in ("1", "0"):
        monkeypatch.setenv("LFI_PGEMM_SIGNS", on)
        monkeypatch.setenv("LFI_PGEMM_PERSIST", on)
        torch.manual_seed(11)
        np.random.seed(11)
        lm = LetsFaceItGlow(Namespace(**copy.deepcopy(hp)))
        lm.to(gpu_device)
        lm.train()
        lm.seq_glow.injected_masks = masks
        loss = lm.fused_training_step(batch, 1e-3)
        torch.cuda.synchronize()
        e = lm.seq_glow.engine
        assert e._last.chain and (e._last.signs is not None) == (on == "1")
        outs.append((float(loss), e.params.clone(), {n: p.detach().clone() for n, p in lm.seq_glow.named_parameters()}))
    assert np.isfinite(outs[0][0]) and outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1])
    for n in outs[0][2]:
        assert torch.equal(outs[0][2][n], outs[1][2][n]), n
