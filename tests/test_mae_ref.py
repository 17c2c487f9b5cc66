"""tests/mae_ref.py without a GPU: the fp64 references against the project's torch compositions,
the bf16 helpers against torch's own rounding and hand-built ties, the input builders, and the
near-tie share of every seeded case of tests/test_mae_glue_structured_gpu.py (a property of the
inputs and the references alone)."""

import pytest
import torch

import mae_ref as M
from jumbo_mae_tpu_amd.ops import mae as mae_ops
from jumbo_mae_tpu_amd.utils.mae import extract_patches_nchw, index_sequence, masking_ids
from jumbo_mae_tpu_amd.utils.mixup import Mixup

F64 = torch.float64


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ bf16 helpers
def test_bf16_rne_matches_torch_on_random_data():
    g = _gen(0)
    x = torch.cat([torch.randn(20000, generator=g, dtype=F64) * s for s in (1e-30, 1e-3, 1.0, 300.0, 1e30)])
    x = x.float().double()  # fp32-representable: torch's double -> float -> bf16 then rounds once
    assert torch.equal(M.bits16(M.bf16_rne(x)), M.bits16(x.bfloat16()))
    assert torch.equal(M.bits16(M.bf16_rne(-x)), M.bits16((-x).bfloat16()))


def test_bf16_rne_on_hand_built_ties():
    # 1 + k 2^-7 are adjacent bf16 values in [1, 2); their midpoints tie to the even significand
    k = torch.arange(0, 8, dtype=F64)
    mid = 1.0 + (k + 0.5) * 2.0 ** -7
    want = 1.0 + (k + (k % 2)) * 2.0 ** -7
    assert torch.equal(M.bf16_rne(mid).double(), want)
    assert torch.equal(M.bf16_rne(-mid).double(), -want)
    assert torch.equal(M.bits16(M.bf16_rne(mid)), M.bits16(mid.bfloat16()))
    assert (M.bf16_tie_distance(mid) == 0).all()
    # one fp64 ulp off the tie decides, which a detour through fp32 would lose
    up = torch.nextafter(mid, torch.full_like(mid, 9.0))
    dn = torch.nextafter(mid, torch.full_like(mid, -9.0))
    assert torch.equal(M.bf16_rne(up).double(), 1.0 + (k + 1) * 2.0 ** -7)
    assert torch.equal(M.bf16_rne(dn).double(), 1.0 + k * 2.0 ** -7)
    # across a binade boundary: 2 - 2^-8 is the midpoint of 2 - 2^-7 and 2
    assert M.bf16_rne(torch.tensor([2.0 - 2.0 ** -8], dtype=F64)).item() == 2.0
    # bf16 values themselves are half a spacing away from every midpoint
    v = torch.tensor([1.0, 1.5, -3.0, 0.0078125], dtype=F64)
    assert torch.equal(M.bf16_tie_distance(v), torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -15], dtype=F64))
    assert torch.equal(M.bf16_rne(torch.zeros(3, dtype=F64)).double(), torch.zeros(3, dtype=F64))


def test_check_rules_catch_injected_faults():
    g = _gen(1)
    ref = torch.randn(4000, generator=g, dtype=F64)
    comp = ref.float()
    good = M.bf16_rne(ref)
    M.check_bf16(good, ref, comp, "self")
    bad = good.clone()
    bad.view(torch.int16)[17] += 1  # one bf16 step on one element
    with pytest.raises(AssertionError):
        M.check_bf16(bad, ref, comp, "one step off")
    with pytest.raises(AssertionError):  # truncation instead of round to nearest even
        M.check_bf16((ref.float().view(torch.int32) & -65536).view(torch.float32).bfloat16(), ref, comp, "truncated")
    M.check_f32(comp, ref, comp, "self")
    off = comp.clone()
    off[5] = torch.nextafter(torch.nextafter(torch.nextafter(off[5], torch.tensor(9.0)), torch.tensor(9.0)),
                             torch.tensor(9.0))
    with pytest.raises(AssertionError):
        M.check_f32(off, ref, comp, "three ulps off")


# ------------------------------------------------------------------ input builders
def test_coded_images_tell_every_index_apart():
    img = M.coded_images(3, 32, 48)
    assert img.dtype == torch.uint8 and img.shape == (3, 3, 32, 48)
    assert int(img[2, 1, 5, 7]) == (17 * 2 + 85 + 35 + 91) % 256
    assert not torch.equal(img[..., :32, :32], img[..., :32, :32].transpose(2, 3))  # y <-> x
    assert not torch.equal(img[0], img[1]) and not torch.equal(img[:, 0], img[:, 1])  # b, c
    assert not torch.equal(img.reshape(3, 3, 48, 32)[..., :32, :], img[..., :32])  # H <-> W
    r = M.random_coded_images(3, 32, 48, seed=3)
    assert torch.equal(r, M.random_coded_images(3, 32, 48, seed=3)) and not torch.equal(r, img)


def test_byte_table_and_special_patches():
    t = M.byte_table_images(2, 16, 24)
    for b in range(2):
        for c in range(3):
            assert t[b, c].unique().numel() == 256
    for B, H, W, p in M.PATCH_SHAPES + M.MIX_SHAPES:
        img = M.patch_images(B, H, W, p)
        assert img.shape == (B, 3, H, W)
        if (H, W) == (32, 48):  # all 768 (channel, byte) pairs survive the painted patches
            assert all(img[:, c].unique().numel() == 256 for c in range(3))
    img, rows = M.special_images(3, 32, 48, 16)
    pt = extract_patches_nchw(img, 16).reshape(18, -1)
    assert (pt[rows["zero"]] == 0).all() and (pt[rows["full"]] == 255).all()
    assert torch.equal(pt[rows["flat"]].view(-1, 3), torch.tensor(M.FLAT_RGB, dtype=torch.uint8).expand(256, 3))
    var = M.exact_target(img, 16, False).reshape(18, -1).var(-1, unbiased=False)
    assert var[rows["flat"]] < 1e-4 and var[rows["zero"]] < 0.05 and var[rows["full"]] < 0.05


def test_exact_activations_sum_exactly():
    g = _gen(2)
    e, pos = M.small_int_bf16((64, 20), g), M.dyadic_f32((64, 20), g)
    assert torch.equal((e.float() + pos).double(), e.double() + pos.double())
    d = M.dyadic_f32((3000, 8), g)
    for order in (torch.arange(3000), torch.randperm(3000, generator=g)):
        s = torch.zeros(8)
        for chunk in d[order].split(7):
            s = s + chunk.sum(0)
        assert torch.equal(s.double(), d.double().sum(0))


# ------------------------------------------------------------------ references vs the torch compositions
@pytest.mark.parametrize("B,H,W,p", [(2, 32, 48, 16), (1, 28, 42, 14), (3, 8, 12, 4), (1, 4, 6, 2), (2, 48, 32, 16)])
def test_patch_references(B, H, W, p):
    img = M.random_coded_images(B, H, W, seed=p)
    t64 = M.patches64(img, p)
    m, s = mae_ops._mean_std("cpu")
    comp = extract_patches_nchw((img.double() / 255.0 - m.double()) / s.double(), p)
    assert torch.equal(t64, comp) and torch.equal(t64, M.exact_target(img, p, False))
    assert (t64 - extract_patches_nchw(mae_ops.normalize_images(img), p).double()).abs().max() < 1e-6
    assert (M.exact_target(img, p, True) - mae_ops.norm_pix(t64)).abs().max() == 0
    N = t64.shape[1]
    g = _gen(5)
    for ids in (torch.randperm(N, generator=g)[: max(1, N // 2)],
                torch.stack([torch.randperm(N, generator=g)[: max(1, N // 2)] for _ in range(B)])):
        want = index_sequence(comp, ids).reshape(-1, 3 * p * p)
        assert torch.equal(M.gather64(img, ids.to(torch.int32), p), want)
        assert torch.equal(M.gather32(img, ids.to(torch.int32), p),
                           index_sequence(M.patches32(img, p), ids).reshape(-1, 3 * p * p))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_mix_reference(mode):
    B, H, W, p = 3, 32, 48, 8
    img = M.random_coded_images(B, H, W, seed=9)
    perm, box, ratio = M.mix_perm(B), (5, 27, 3, 41), 0.3
    assert sorted(perm.tolist()) == [0, 1, 2] and int(perm[2]) == 2 and int(perm[0]) != 0
    got = M.mix64(img, p, mode, ratio, perm, box)
    plan = M.mix_plan(mode, torch.tensor(ratio, dtype=torch.float32).double().item(), perm, box)
    want = extract_patches_nchw(Mixup.mix_images(M.normalized64(img), plan), p).reshape(got.shape)
    assert (got - want).abs().max() < 1e-15  # 1 - r and the box mask are formed differently, same value
    assert (M.mix32(img, p, mode, ratio, perm, box).double() - got).abs().max() < 2e-6
    if mode == 2:  # the box is the half-open pixel range of the plan
        inside = M.box_mask(H, W, box)
        assert int(inside.sum()) == (27 - 5) * (41 - 3) and inside[5, 3] and not inside[27, 3] and not inside[5, 41]


@pytest.mark.parametrize("per_sample", [False, True])
def test_embed_and_unshuffle_references(per_sample):
    B, C, N, K, d = 3, 2, 9, 4, 8
    g = _gen(11)
    noise = torch.rand((B, N) if per_sample else (N,), generator=g)
    _, restore, keep, _ = masking_ids(noise, K)
    e = torch.randn(B * K, d, generator=g).bfloat16()
    pos, cls = torch.randn(N, d, generator=g), torch.randn(C, d, generator=g)
    ev = e.double().view(B, K, d) + pos.double()[keep]
    want = torch.cat([cls.double().expand(B, C, d), ev], 1)
    assert torch.equal(M.embed_finish64(e, pos, keep, cls, B), want)
    assert torch.equal(M.embed_finish64(e, None, keep, cls, B)[:, C:], e.double().view(B, K, d))

    y = torch.randn(B, C + K, d, generator=g).bfloat16()
    tok = torch.randn(d, generator=g)
    yr, tr = y.double().requires_grad_(), tok.double().requires_grad_()
    out = mae_ops.unshuffle(yr, tr, restore, pos.double(), C)
    assert torch.equal(M.unshuffle_fwd64(y, tok, restore, pos, C), out.detach())
    dout = torch.randn(B, C + N, d, generator=g)
    out.backward(dout.double())
    dy, dtok = M.unshuffle_bwd64(dout, restore, C, K)
    assert torch.equal(dy, yr.grad) and (dtok - tr.grad).abs().max() < 1e-12


@pytest.mark.parametrize("norm_pix", [False, True])
def test_patch_mse_references(norm_pix):
    c = M.mse_case(2, 16, 24, 8, norm_pix)
    pr = c["pred"].double().requires_grad_()
    t = extract_patches_nchw(M.normalized64(c["img"]), 8).reshape(pr.shape)
    if norm_pix:
        t = mae_ops.norm_pix(t)
    mse = (t - pr).square().mean(-1)
    mse.backward(c["dmse"].double())
    assert (mse.detach() - c["mse64"]).abs().max() < 1e-14
    assert (pr.grad - c["dpred64"]).abs().max() < 1e-15
    assert (c["dpred64"][::3] == 0).all() and (c["dmse"][1::3] != 0).all()
    assert (c["mse32"].double() - c["mse64"]).abs().max() < 1e-5 * c["mse64"].max()


def test_mask_ids_reference():
    g = _gen(13)
    noise = torch.rand(3, 50, generator=g)
    noise[:, 1::7] = noise[:, 0:1]
    noise[1, :6] = torch.tensor([0.0, -0.0, float("inf"), 0.0, float("inf"), -0.0])
    sh, rs, keep, mask = M.mask_ids_ref(noise, 12)
    ref_sh = torch.argsort(noise, dim=-1, stable=True)
    ref_rs = torch.argsort(ref_sh, dim=-1, stable=True)
    assert torch.equal(sh, ref_sh) and torch.equal(rs, ref_rs) and torch.equal(keep, ref_sh[:, :12])
    assert torch.equal(mask, (ref_rs >= 12).float())
    s2, r2, k2, m2 = masking_ids(noise[0], 12)  # the CPU composition of the project (no ties in row 0 but 1::7)
    assert torch.equal(r2, torch.argsort(s2)) and torch.equal(m2, (r2 >= 12).float())


# ------------------------------------------------------------------ near-tie shares of the seeded cases
@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm-pix"])
@pytest.mark.parametrize("shape", M.MSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_near_tie_share_dpred(shape, norm_pix):
    c = M.mse_case(*shape, norm_pix)
    live = c["dmse"] != 0
    share = M.near_tie_share(c["dpred64"][live], c["dpred32"][live])
    print(f"[mae] dpred {shape} norm_pix={norm_pix}: near-tie share {share:.2e}")
    assert share <= M.NEAR_TIE_CAP
    # the patch-wide statistics: the fp32 composition stays close enough for the bound to mean something
    assert (c["mse32"].double() - c["mse64"]).abs().max() <= 1e-5 * c["mse64"].abs().max()


@pytest.mark.parametrize("shape", M.PATCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_near_tie_share_gather(shape):
    B, H, W, p = shape
    img = M.patch_images(B, H, W, p)
    ids = torch.arange((H // p) * (W // p), dtype=torch.int32)
    share = M.near_tie_share(M.gather64(img, ids, p), M.gather32(img, ids, p))
    print(f"[mae] gather {shape}: near-tie share {share:.2e}")
    assert share <= M.NEAR_TIE_CAP


@pytest.mark.parametrize("ratio", M.MIX_RATIOS)
@pytest.mark.parametrize("shape", M.MIX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_near_tie_share_mixup(shape, ratio):
    B, H, W, p = shape
    img = M.patch_images(B, H, W, p)
    perm = M.mix_perm(B)
    share = M.near_tie_share(M.mix64(img, p, 1, ratio, perm, None), M.mix32(img, p, 1, ratio, perm, None))
    print(f"[mae] mixup {shape} r={ratio}: near-tie share {share:.2e}")
    assert share <= M.NEAR_TIE_CAP
