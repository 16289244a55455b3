"""GPU: the transposed fragment reads of gemm_planes16t_kernel by inline assembly (LFI_PGEMM_TR_ASM, default on) against the builtin
reads (LFI_PGEMM_TR_ASM=0), bit for bit.

With the asm reads the compiler no longer drains the LDS-DMA ring in front of every transposing read, so the hand-counted s_waitcnt
vmcnt(n) at the loop's barriers bind for the first time, and the compiler no longer counts the reads on lgkmcnt. A wrong count or a
fragment used before its wait shows up as wrong VALUES (and, being a race, not as the same wrong values every time): every case
runs three times with the switch on, the three runs agree bit for bit, and they equal the switch-off run bit for bit.

The four products are built as the engine builds them (engine._backward_chain): A's lo planes never read (skip bit 0: they are
poisoned with NaN here), dpre in place with sign words and column sums, split K. Shapes: K = 1, 2, 3, 4, 5, 7 pairs of k-tiles (the
ring of three slots wraps after three; the pair loop is unrolled by three and leaves at any of its three exits), M = 64 and 130,
N = 64 and 320 (a partial 256-wide and a partial 128-wide tile), batch 2, split K 2 with an odd number of pairs (3, 5, 7: the
splits then get different numbers of pairs), both tile forms."""
import os

import numpy as np
import pytest
import torch

from test_gpu_pgemm_signs import pack_signs

pytestmark = pytest.mark.gpu

PAIRS = [1, 2, 3, 4, 5, 7]
MS, NS = (64, 130), (64, 320)


@pytest.fixture(scope="module")
def eng(gpu_device):
    from argparse import Namespace
    from helpers import Fixture
    from lets_face_it_amd.engine import GlowEngine, ModelSpec
    return GlowEngine(ModelSpec(Namespace(**Fixture("tiny").hp)), gpu_device)


class _switch:
    """LFI_PGEMM_TR_ASM for the length of a with block (the library reads it per call)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.saved = os.environ.get("LFI_PGEMM_TR_ASM")
        os.environ["LFI_PGEMM_TR_ASM"] = "1" if self.on else "0"

    def __exit__(self, *exc):
        if self.saved is None:
            os.environ.pop("LFI_PGEMM_TR_ASM", None)
        else:
            os.environ["LFI_PGEMM_TR_ASM"] = self.saved


def _poison_lo(P):
    P.view(-1, 2, 512)[:, 1] = float("nan")   # every lo block: skip bit 0 never fetches A's


def _operands(eng, dev, product, M, N, K, batch, seed):
    """Operand planes of one product, laid out as the engine lays them out. -> (A fp32, B fp32, descriptor keywords)
       dwc    dW_c = dgi[k]^T c[:, k]:   A = (batch K) x M by columns (transposed use), B = K x (batch N) transposed, batch entries =
              row tiles of A / column tiles of B, C batch entries apart
       wgrad  dwf = dpre^T cond:         A = K x M transposed, B = K x N transposed
       dgrad  dcond = dpre W:            A = M x K by rows, B = K x N transposed"""
    g = torch.Generator().manual_seed(seed)
    if product == "dwc":
        A = torch.randn(batch * K, M, generator=g).to(dev)
        Bm = torch.randn(K, batch * N, generator=g).to(dev)
        Ap, nka = eng.planes("test.tra", A, M, batch * K, M)
        Bp, nkb = eng.planes("test.trb", Bm, batch * N, K, batch * N)
        kw = dict(a_fmt=1, b_fmt=1, batch=batch, a_stride=(K // 32) * nka * 1024, b_stride=(N // 16) * 1024, sC=M * N)
    elif product == "wgrad":
        A = torch.randn(K, M, generator=g).to(dev)
        Bm = torch.randn(K, N, generator=g).to(dev)
        Ap, nka = eng.planes("test.tra", A, M, K, M)
        Bp, nkb = eng.planes("test.trb", Bm, N, K, N)
        kw = dict(a_fmt=1, b_fmt=1)
    else:
        A = torch.randn(M, K, generator=g).to(dev)
        Bm = torch.randn(K, N, generator=g).to(dev)
        Ap, nka = eng.planes("test.tra", A, K, M, K)
        Bp, nkb = eng.planes("test.trb", Bm, N, K, N)
        kw = dict(a_fmt=0, b_fmt=1)
    _poison_lo(Ap)
    return A, Bm, Ap, nka, Bp, nkb, kw


def _run(eng, dev, M, N, K, Ap, nka, Bp, nkb, kw, batch, splitk, tile):
    Cm = torch.full((batch, M, N), 7.0, device=dev)
    eng.pass_skip = {"t": 1}
    try:
        eng.gemm_planes(M, N, K, Ap, nka, Bp, nkb, Cm, N, splitk=splitk, tile=tile, cls="t", **kw)
    finally:
        eng.pass_skip = {}
    return Cm


def _four_runs(run):
    """-> (switch-off result, [three switch-on results])"""
    with _switch(False):
        off = run()
    with _switch(True):
        on = [run() for _ in range(3)]
    torch.cuda.synchronize()
    return off, on


def _assert_same(off, on, what):
    for t in ([off] if isinstance(off, torch.Tensor) else off):
        assert bool(torch.isfinite(t).all()), "%s: A's poisoned lo planes were read" % what
    for i, r in enumerate(on):
        assert _equal(r, on[0]), "%s: run %d of the asm reads differs from run 0" % (what, i)
    assert _equal(on[0], off), "%s: asm reads differ from the builtin reads" % what


def _equal(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _splits(pairs):
    return (1, 2) if pairs in (3, 5, 7) else (1,)


@pytest.mark.parametrize("tile", [1, 2])
@pytest.mark.parametrize("pairs", PAIRS)
@pytest.mark.parametrize("product", ["dwc", "wgrad", "dgrad"])
def test_asm_reads_match_builtin_reads(eng, gpu_device, product, pairs, tile):
    """dW_c, the cond_transform weight gradient (A transposed) and the feature gradient (A by rows): every M, N and split of the
    module's list at this K and tile form."""
    K = 32 * pairs
    batch = 2 if product == "dwc" else 1
    for M in MS:
        for N in NS:
            _, _, Ap, nka, Bp, nkb, kw = _operands(eng, gpu_device, product, M, N, K, batch, 1000 * pairs + M + N)
            for splitk in _splits(pairs):
                off, on = _four_runs(lambda: _run(eng, gpu_device, M, N, K, Ap, nka, Bp, nkb, kw, batch, splitk, tile))
                _assert_same(off, on, "%s M=%d N=%d K=%d splitk=%d tile=%d" % (product, M, N, K, splitk, tile))


def _dpre(eng, dev, M, N, K, batch, seed):
    """The in-place dpre product (engine._dpre_product): planes of c rewritten in place, mask from sign words, hi planes only, column
    sums; dgi's lo planes never read. Fresh buffers for every run (the product overwrites its own mask source's planes).
    -> (hi planes, column sums, dgi fp32, W fp32, c fp32)"""
    g = torch.Generator().manual_seed(seed)
    Ncols = batch * N
    A = torch.randn(M, batch * K, generator=g).to(dev)
    W = torch.randn(batch * K, N, generator=g).to(dev)
    Gm = torch.randn(M, Ncols, generator=g)
    Ap, nka = eng.planes("test.trda", A, batch * K, M, batch * K)
    Wp, nkw = eng.planes("test.trdw", W, N, batch * K, N)
    Gp, nkg = eng.planes("test.trdg", Gm.to(dev), Ncols, M, Ncols)
    _poison_lo(Ap)
    words = pack_signs((Gm.bfloat16().float() > 0).numpy()).to(dev)
    sums = torch.zeros(Ncols, device=dev)
    kw = dict(act=2, slope=0.01, batch=batch, b_fmt=1, a_stride=(K // 16) * 1024, b_stride=(K // 32) * nkw * 1024, sC=N,
              store=False, Cr=Gp, cr_nkt=nkg, hi_only=True, colsum_into=sums, cls="t", tile=1, sign_in=words)
    eng.pass_skip = {"t": 1}
    try:
        assert eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, Ncols, signs_query=True, **kw)
        assert eng.gemm_planes(M, N, K, Ap, nka, Wp, nkw, None, Ncols, **kw)
    finally:
        eng.pass_skip = {}
    nblk = (M + 31) // 32 * nkg
    hi = Gp[:nblk * 1024].view(-1, 2, 512)[:, 0].view(torch.int16).clone()
    return (hi, sums), (A, W, Gm, Gp, nkg)


@pytest.mark.parametrize("pairs", PAIRS)
def test_dpre_asm_reads_match_builtin_reads(eng, gpu_device, pairs):
    """dpre (A by rows, the direct in-place epilogue, sign words, the sign word load riding the VM counter ahead of the ring fill)."""
    K = 32 * pairs
    for M in MS:
        for N in NS:
            seed = 2000 * pairs + M + N
            off, on = _four_runs(lambda: _dpre(eng, gpu_device, M, N, K, 2, seed)[0])
            _assert_same(off, on, "dpre M=%d N=%d K=%d" % (M, N, K))


def _rel_l2(x, ref):
    return float((x.double().cpu() - ref.cpu()).norm() / ref.cpu().norm())


@pytest.mark.parametrize("product", ["dwc", "wgrad", "dgrad", "dpre"])
def test_against_fp64_product(eng, gpu_device, monkeypatch, product):
    """One case per product against the fp64 product of the same inputs (A rounded to bf16, as the kernel takes it): the asm path's
    relative L2 error may not exceed the builtin path's (they are bit-identical: this guards the harness - a comparison of two
    empty or two equally wrong results would pass the tests above). The builtin path's error is printed; it is a two-product
    bf16 x 3 product, so 2^-16 per term at the worst, and a harness that compared nothing useful would be far above 1e-3."""
    M, N, K, dev = 130, 320, 224, gpu_device
    if product == "dpre":
        with _switch(False):
            (h0, s0), (A, W, Gm, _, _) = _dpre(eng, dev, M, N, K, 2, 77)
        with _switch(True):
            (h1, s1), _ = _dpre(eng, dev, M, N, K, 2, 77)
        torch.cuda.synchronize()
        Ad, Wd = A.bfloat16().double().cpu(), W.double().cpu()
        ref = torch.cat([Ad[:, b * K:(b + 1) * K] @ Wd[b * K:(b + 1) * K] for b in range(2)], dim=1)
        ref = ref * torch.where(Gm.bfloat16().double() > 0, 1.0, 0.01)
        e0, e1 = _rel_l2(s0, ref.sum(0)), _rel_l2(s1, ref.sum(0))   # (the column sums: fp32 sums of the fp32 result)
        assert torch.equal(h0, h1)
    else:
        batch = 2 if product == "dwc" else 1
        A, Bm, Ap, nka, Bp, nkb, kw = _operands(eng, dev, product, M, N, K, batch, 78)
        with _switch(False):
            c0 = _run(eng, dev, M, N, K, Ap, nka, Bp, nkb, kw, batch, 1, 1)
        with _switch(True):
            c1 = _run(eng, dev, M, N, K, Ap, nka, Bp, nkb, kw, batch, 1, 1)
        monkeypatch.setenv("LFI_PGEMM_16T", "0")   # the 32 x 32 x 16 kernel: the same products in another summation order
        c32 = _run(eng, dev, M, N, K, Ap, nka, Bp, nkb, kw, batch, 1, 1)
        torch.cuda.synchronize()
        assert not torch.equal(c32, c1), "the product did not run on gemm_planes16t_kernel: the switch was not exercised"
        Ad, Bd = A.bfloat16().double().cpu(), Bm.double().cpu()
        if product == "dwc":
            ref = torch.stack([Ad[b * K:(b + 1) * K].t() @ Bd[:, b * N:(b + 1) * N] for b in range(2)])
        elif product == "wgrad":
            ref = (Ad.t() @ Bd)[None]
        else:
            ref = (Ad @ Bd)[None]
        e0, e1 = _rel_l2(c0, ref), _rel_l2(c1, ref)
    print("%s: relative L2 error against fp64, builtin reads %.3e, asm reads %.3e" % (product, e0, e1))
    assert e1 <= e0
    assert e0 < 1e-3


def test_two_training_steps_switch_on_and_off(gpu_device, monkeypatch):
    """Two fused training steps of the smallest final_model-shaped fixture that takes the planes chain (see
    test_gpu_pgemm_signs.test_whole_training_step_with_and_without_signs_and_persistence for B = 32, T = 25) with the switch on
    and off: loss of both steps and every parameter afterwards byte-identical."""
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
        monkeypatch.setenv("LFI_PGEMM_TR_ASM", on)
        torch.manual_seed(11)
        np.random.seed(11)
        lm = LetsFaceItGlow(Namespace(**copy.deepcopy(hp)))
        lm.to(gpu_device)
        lm.train()
        lm.seq_glow.injected_masks = masks
        losses = []
        for _ in range(2):
            losses.append(float(lm.fused_training_step(batch, 1e-3)))
            torch.cuda.synchronize()
            assert lm.seq_glow.engine._last.chain
        e = lm.seq_glow.engine
        outs.append((losses, e.params.clone(), {n: p.detach().clone() for n, p in lm.seq_glow.named_parameters()}))
    assert all(np.isfinite(v) for v in outs[0][0]) and outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1])
    for n in outs[0][2]:
        assert torch.equal(outs[0][2][n], outs[1][2][n]), n
