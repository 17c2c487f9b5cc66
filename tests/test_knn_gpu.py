"""csrc/knn.hip (fused similarity + top-k, weighted vote) against the fp64 torch compositions of
ops/knn.py.

Bounds.  On exactly summable inputs (entries from {-1, -0.5, 0, 0.5, 1} * 2^-3: every dot product is
exact in fp32 in any summation order) ``idx`` and ``sim`` EQUAL the fp64 oracle, ties included, at
every ``splits``.  On random unit rows ``eps = 2 * D * 2^-24``: twice the standard bound on fp32
accumulation of a sum whose absolute terms add to at most 1 (the MFMA's internal summation order is
not documented, hence the factor 2); every query must keep each reported similarity within ``eps``
of the fp64 dot product of the row it names, a sorted list without repeats, and every reported
neighbour's fp64 score at least the oracle's k-th score minus ``eps``.  The vote is exact: both
sides add the same fp64 terms in the same order, and every tie in the inputs is one by
construction."""

import os
import subprocess
import sys
import textwrap

import pytest
import torch

import knn_ref as KR
from jumbo_mae_tpu_amd.ops import _ext
from jumbo_mae_tpu_amd.ops import knn as K
from jumbo_mae_tpu_amd.ops import prims as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON_I = 0x5A5A5A5A
POISON_F = 0x7FC12345  # a NaN with a payload


def _run(q, bank, k, self_idx=None, splits=0):
    """The kernel into the middle rows of poisoned buffers: (idx, sim) on the CPU, after checking that
    the rows before and after the outputs still hold the poison."""
    Nq = q.shape[0]
    bi = torch.full((Nq + 2, k), POISON_I, dtype=torch.int32, device="cuda")
    bs = torch.full((Nq + 2, k), POISON_F, dtype=torch.int32, device="cuda").view(torch.float32)
    si = None if self_idx is None else self_idx.cuda()
    idx, sim = K.knn_topk(q.cuda(), bank.cuda(), k, si, splits, out=(bi[1:Nq + 1], bs[1:Nq + 1]))
    assert idx.data_ptr() == bi[1].data_ptr() and sim.data_ptr() == bs[1].data_ptr()
    torch.cuda.synchronize()
    for guard in (bi[0], bi[Nq + 1]):
        assert (guard == POISON_I).all()
    for guard in (bs[0], bs[Nq + 1]):
        assert (guard.view(torch.int32) == POISON_F).all()
    return idx.cpu(), sim.cpu()


def _oracle(q, bank, k, self_idx=None):
    return K.knn_topk_torch(q, bank, k, self_idx, dtype=torch.float64)


# ------------------------------------------------------------------ exactly summable inputs
@pytest.fixture(scope="module")
def exact_203():
    return KR.exact_inputs(37, 203, 96, seed=11)


@pytest.mark.parametrize("k", [1, 5, 20, 64])
def test_topk_exact(exact_203, k):
    q, bank = exact_203
    ridx, rsim = _oracle(q, bank, k)
    idx, sim = _run(q, bank, k)
    assert idx.dtype == torch.int32 and sim.dtype == torch.float32
    assert torch.equal(idx, ridx)
    assert torch.equal(sim.double(), rsim)
    if k > 1:  # the inputs do contain ties between different bank rows
        assert ((rsim[:, 1:] == rsim[:, :-1]) & (ridx[:, 1:] > ridx[:, :-1])).any()
    i2, s2 = _run(q, bank, k)
    assert torch.equal(i2, idx) and torch.equal(s2, sim)  # a rerun is bit-identical


def test_topk_bank_smaller_than_k():
    q, bank = KR.exact_inputs(70, 13, 32, seed=12)
    ridx, rsim = _oracle(q, bank, 20)
    idx, sim = _run(q, bank, 20)
    assert torch.equal(idx, ridx) and torch.equal(sim.double(), rsim)
    assert (idx[:, 13:] == -1).all() and (sim[:, 13:] == float("-inf")).all() and (idx[:, :13] >= 0).all()


def test_topk_does_not_depend_on_splits():
    q, bank = KR.exact_inputs(130, 5000, 160, seed=13)
    ridx, rsim = _oracle(q, bank, 20)
    ext = _ext.load(True)
    assert ext.knn_splits(130, 5000, 3) == 3 and ext.knn_splits(130, 5000, 0) >= 1
    for splits in (0, 1, 3, 7):
        idx, sim = _run(q, bank, 20, splits=splits)
        assert torch.equal(idx, ridx), splits
        assert torch.equal(sim.double(), rsim), splits


def test_topk_leave_one_out():
    q, _ = KR.exact_inputs(150, 150, 64, seed=14, q_from_bank=False)
    bank = q.clone()
    bank[100:110] = bank[0:10]  # duplicates at other indices
    q = bank.clone()
    me = torch.arange(150, dtype=torch.int32)
    ridx, rsim = _oracle(q, bank, 20, me)
    idx, sim = _run(q, bank, 20, self_idx=me)
    assert torch.equal(idx, ridx) and torch.equal(sim.double(), rsim)
    assert not (idx == me[:, None]).any()  # no row returns itself
    for r in range(10):  # its duplicate at another index is still found, first
        assert idx[r, 0] == 100 + r and idx[100 + r, 0] == r
    # -1 = nothing to skip: that query finds itself first
    me2 = me.clone()
    me2[5] = -1
    idx2, _ = _run(q, bank, 20, self_idx=me2)
    assert idx2[5, 0] == 5 and torch.equal(idx2[6:], idx[6:])


def test_topk_bad_arguments_return_an_error():
    ext = _ext.load(True)
    q = torch.zeros(8, 64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="k must be in 1..64"):
        ext.knn_topk(q, q, 65)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ext.knn_topk(q[:, :48], q[:, :48], 5)
    flat = torch.zeros(8 * 64 + 8, dtype=torch.bfloat16, device="cuda")
    odd = flat[4:4 + 8 * 64].view(8, 64)  # rows 8 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="knn_topk"):
        ext.knn_topk(odd, q, 5)
    with pytest.raises(RuntimeError, match="knn_topk"):
        ext.knn_topk(q, q, 5, splits=5000)
    torch.cuda.synchronize()
    # the Python layer realigns the rows, and sends a width that is no multiple of 32 to the composition
    qa, ba = KR.exact_inputs(8, 40, 64, seed=15)
    flat[4:4 + 8 * 64] = qa.cuda().reshape(-1)
    idx, sim = K.knn_topk(odd, ba.cuda(), 5)
    ridx, rsim = _oracle(qa, ba, 5)
    assert torch.equal(idx.cpu(), ridx) and torch.equal(sim.cpu().double(), rsim)
    idx, sim = K.knn_topk(qa[:, :48].cuda(), ba[:, :48].cuda(), 5)
    ridx, rsim = _oracle(qa[:, :48], ba[:, :48], 5)
    assert torch.equal(idx.cpu(), ridx) and torch.equal(sim.cpu().double(), rsim)


# ------------------------------------------------------------------ random unit rows
@pytest.mark.parametrize("Nq,Nb,D", [(64, 1000, 3072), (37, 203, 96)])
def test_topk_random_unit_rows(Nq, Nb, D):
    k = 20
    g = torch.Generator().manual_seed(Nb)
    q = K.normalize_features(torch.randn(Nq, D, generator=g))
    bank = K.normalize_features(torch.randn(Nb, D, generator=g))
    S = q.double() @ bank.double().t()  # fp64 from the same bf16 values
    kth = S.topk(k, dim=1).values[:, -1]
    eps = 2 * D * 2.0 ** -24
    idx, sim = _run(q, bank, k)
    assert (idx >= 0).all() and (idx < Nb).all()
    named = S.gather(1, idx.long())
    err = (sim.double() - named).abs().max().item()
    short = (kth[:, None] - named).max().item()
    print(f"knn_topk random rows ({Nq}, {Nb}, {D}): max |sim - fp64| = {err:.3e}, "
          f"max (oracle k-th - neighbour's fp64 score) = {short:.3e}, eps = {eps:.3e}")
    assert err <= eps
    assert (sim[:, 1:] <= sim[:, :-1]).all()
    tie = sim[:, 1:] == sim[:, :-1]
    assert (idx[:, 1:][tie] > idx[:, :-1][tie]).all()
    assert short <= eps
    assert all(len(set(row.tolist())) == k for row in idx)


# ------------------------------------------------------------------ vote
@pytest.mark.parametrize("k", [1, 5, 20, 64])
@pytest.mark.parametrize("classes", [10, 1000])
def test_vote_exact(k, classes):
    idx, sim, bank_labels, labels = KR.vote_inputs(129, k, classes)
    rp, r1, r5 = K.knn_vote_torch(idx, sim, bank_labels, labels, 0.07, dtype=torch.float64)
    args = [t.cuda() for t in (idx, sim, bank_labels, labels)]
    pred, h1, h5 = K.knn_vote(*args, 0.07)
    assert pred.dtype == torch.int32 and h1.dtype == torch.bool and h5.dtype == torch.bool
    assert torch.equal(pred.cpu(), rp) and torch.equal(h1.cpu(), r1) and torch.equal(h5.cpu(), r5)
    assert not h1.cpu()[labels == -1].any() and not h5.cpu()[labels == -1].any()
    if k >= 4:  # the constructed tie: equal scores, the smaller class id first
        assert pred[1].tolist() == [1, 3, -1, -1, -1]
    p2, a1, a5 = K.knn_vote(*args, 0.07)
    assert torch.equal(p2, pred) and torch.equal(a1, h1) and torch.equal(a5, h5)


# ------------------------------------------------------------------ end to end
def _clusters():
    """20 classes x 30 rows in D = 192: unit centroids + 0.03 Gaussian noise (seed 5)."""
    g = torch.Generator().manual_seed(5)
    cent = torch.nn.functional.normalize(torch.randn(20, 192, generator=g), dim=-1)
    x = cent.repeat_interleave(30, 0) + 0.03 * torch.randn(600, 192, generator=g)
    return K.normalize_features(x), torch.arange(20).repeat_interleave(30)


def test_classify_clusters_leave_one_out():
    feats, labels = _clusters()
    me = torch.arange(600)
    oi, os_ = K.knn_topk_torch(feats, feats, 10, me, dtype=torch.float64)
    _, o1, _ = K.knn_vote_torch(oi, os_, labels, labels, 0.07, dtype=torch.float64)
    assert o1.all()  # the fp64 oracle scores 100 % on these inputs
    h1, h5 = K.knn_classify(feats.cuda(), labels.cuda(), 10, 0.07)
    assert h1.all() and h5.all()


def test_switch_routes_to_the_composition(monkeypatch):
    feats, labels = _clusters()
    f, y = feats[:64].cuda(), labels[:64].cuda()
    want = K.knn_classify(f, y, 5, 0.07)
    calls = []
    topk_t, vote_t = K.knn_topk_torch, K.knn_vote_torch
    monkeypatch.setattr(K, "knn_topk_torch", lambda *a, **kw: (calls.append("topk"), topk_t(*a, **kw))[1])
    monkeypatch.setattr(K, "knn_vote_torch", lambda *a, **kw: (calls.append("vote"), vote_t(*a, **kw))[1])
    assert K.knn_classify(f, y, 5, 0.07)[0].is_cuda and calls == []  # the kernels
    monkeypatch.setattr(P, "_KNN_OURS", False)
    got = K.knn_classify(f, y, 5, 0.07)
    assert calls == ["topk", "vote"]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_pretrain_features_on_the_gpu():
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.classifier import FinetuneModel
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    from jumbo_mae_tpu_amd.ops import mae as mae_ops

    kw = dict(layers=2, dim=64, heads=2, image_size=32, patch_size=16, posemb="sincos2d", droppath=0.1)
    pm = PretrainModel(ViTConfig(labels=0, image_mask_ratio=0.75, **kw),
                       DecoderConfig(dec_layers=1, dec_dim=64, dec_heads=2, image_size=32, patch_size=16))
    pm = pm.to("cuda", torch.bfloat16, seed=0)
    fm = FinetuneModel(ViTConfig(labels=10, **kw)).to("cuda", torch.bfloat16, seed=1)
    src, dst = pm.store.to_flax_tree(), fm.store.to_flax_tree()
    dst["model"] = {**src["model"], "head": dst["model"]["head"]}
    fm.store.load_flax_tree(dst, strict=True)
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (8, 3, 32, 32), generator=g, dtype=torch.uint8).cuda()
    f = pm.features(img)
    assert f.shape == (8, 192) and f.dtype == torch.float32 and torch.isfinite(f).all()
    assert torch.equal(pm.features(img), f)
    rows = mae_ops.mixed_patches(img, None, 16, fm.store.compute_dtype)
    with torch.no_grad():
        assert torch.equal(fm.features(rows, 8), f)
    # and the monitor's numbers come out of them
    h1, h5 = K.knn_classify(K.normalize_features(f), torch.arange(8, device="cuda") % 2, 3, 0.07)
    assert h1.shape == (8,) and (h5 | ~h1).all()


# ------------------------------------------------------------------ debug build
DEBUG_SCRIPT = textwrap.dedent("""
    import torch
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    assert ext.debug_build and ext.debug_lines() == {}
    idx = torch.tensor([[0, 3, -1], [1, 2, 2]], dtype=torch.int32, device="cuda")
    sim = torch.tensor([[0.5, 0.25, 0.0], [0.5, 0.5, 0.25]], device="cuda")
    bank_labels = torch.tensor([4, 5, 6, 4], dtype=torch.int32, device="cuda")
    labels = torch.tensor([4, 6], dtype=torch.int32, device="cuda")
    pred, h1, h5 = ext.knn_vote(idx, sim, bank_labels, labels, 0.07)
    torch.cuda.synchronize()
    assert ext.debug_lines() == {} and h1.tolist() == [True, True]
    idx[1, 0] = 4                               # one past the bank: ignored, and recorded
    pred, h1, h5 = ext.knn_vote(idx, sim, bank_labels, labels, 0.07)
    torch.cuda.synchronize()
    lines = ext.debug_lines()
    assert set(lines) == {"knn"} and lines["knn"] > 0, lines
    assert pred[1].tolist() == [6, -1, -1, -1, -1]
    print("KNN_DEBUG_OK")
""")


def test_debug_build_checks_the_vote_indices():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], capture_output=True, text=True, timeout=110, env=env,
                       cwd=ROOT)
    assert r.returncode == 0 and "KNN_DEBUG_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
