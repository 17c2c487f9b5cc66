"""csrc/mae.hip, every dispatched path, per element against the fp64 references of tests/mae_ref.py
(rules and bounds: that module's docstring; they come from the fp32 torch compositions, never from
the kernels).  Copy-only kernels and single fp32 adds are compared bit for bit; reruns are identical.

Which kernel a case runs, from the host dispatch of csrc/mae.hip:

  patch_mse (fwd and bwd)
    p = 16, any pred / image layout          patch_mse_*_kernel<12, true>; its ``vec`` flags:
      contiguous pred, pred view ldp = 772     8-byte pred accesses, 16-byte image staging
      ldp = 770, pred view one element in      2-byte pred accesses (ldp % 4 != 0 / base not 8-byte aligned)
      image at byte offset 1                   byte staging of the image (base not 16-byte aligned)
    p = 14 (P3 = 588 = 9 x 64 + 12)          <12, false>, partial last lane group
    p = 12 (P3 = 432)                        <12, false>
    p = 8 (P3 = 192), also ldp = 200         <4, false>
    p = 4 (P3 = 48 < 64)                     <4, false>, lanes 48..63 idle
    p = 18 (P3 = 972)                        <16, false>
    p = 20 (P3 = 1200)                       no kernel: the binding raises, ops.patch_mse composes in torch
  gather_patches / mix_patches   p = 16, 4-byte aligned image: the *16 word kernels; p = 16 at byte
                                 offset 1 and every other p: the generic kernels
  patchify_normalize             4-byte loads when W % 4 == 0 and the base is aligned, else byte loads

All p = 16 forms keep one arithmetic order, so they agree bit for bit, norm_pix included.
"""

import pytest
import torch

import mae_ref as M
from jumbo_mae_tpu_amd.ops import _ext
from jumbo_mae_tpu_amd.ops import mae as mae_ops

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ext():
    return _ext.load(True)


def _sid(s):
    return "x".join(map(str, s))


def _offset_copy(t, off=1):
    """The same bytes in a contiguous view ``off`` elements into a fresh buffer (as test_recon_gpu.py)."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device="cuda")
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + off * t.element_size()
    return v


def _row_strided(t, ld):
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device="cuda")
    v = buf[:, : t.shape[1]]
    v.copy_(t)
    assert v.stride() == (ld, 1)
    return v


def _same_bits(a, b):
    if a.dtype == BF16:
        return torch.equal(M.bits16(a), M.bits16(b))
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------ patch_mse
def _mse_run(ext, pred, img, dmse, p, norm_pix):
    out = []
    for _ in range(2):
        mse = ext.patch_mse_fwd(pred, img, p, norm_pix)
        dpred = ext.patch_mse_bwd(pred, img, dmse, p, norm_pix)
        out.append((mse.cpu(), dpred.cpu()))
    assert _same_bits(out[0][0], out[1][0]) and _same_bits(out[0][1], out[1][1])  # reruns
    return out[0]


def _mse_check(c, mse, dpred, label):
    M.check_f32(mse, c["mse64"], c["mse32"], label + " mse")
    live = c["dmse"] != 0
    assert (M.bits16(dpred[~live]) == 0).all()
    M.check_bf16(dpred[live], c["dpred64"][live], c["dpred32"][live], label + " dpred")


@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm-pix"])
@pytest.mark.parametrize("shape", M.MSE_SHAPES, ids=_sid)
def test_patch_mse(ext, shape, norm_pix):
    """Measured on an MI355X: ``mse`` worst miss / bound 0.28 .. 0.49 (at most 0.49 fp32 ulps) over the
    12 cases.  With fp32 patch sums and statistics the kernels missed this bound in 6 of them (worst
    miss / bound 1.16 .. 1.75, up to 5.2 ulps) and one ``dpred`` element at p = 14 with norm_pix;
    they now work in fp64 like csrc/recon.hip."""
    B, H, W, p = shape
    c = M.mse_case(B, H, W, p, norm_pix)
    # rows = 18, 6, 6, 12, 18, 6: all but p = 8 end in a partial block of four rows
    img, dmse = c["img"].cuda(), c["dmse"].cuda()
    mse, dpred = _mse_run(ext, c["pred"].cuda(), img, dmse, p, norm_pix)
    _mse_check(c, mse, dpred, f"patch_mse {shape}")
    # row stride beyond P3: pred is read with ldp, dpred written with stride P3
    mse2, dpred2 = _mse_run(ext, _row_strided(c["pred"].cuda(), c["P3"] + 8), img, dmse, p, norm_pix)
    assert dpred2.is_contiguous() and _same_bits(mse, mse2) and _same_bits(dpred, dpred2)


@pytest.mark.parametrize("norm_pix", [False, True], ids=["plain", "norm-pix"])
def test_patch_mse_p16_forms(ext, norm_pix):
    """Every layout of pred and of the image at p = 16: same bounds, same bits (one arithmetic order;
    the byte-staged image too, with and without norm_pix)."""
    B, H, W, p = M.MSE_SHAPES[0]
    c = M.mse_case(B, H, W, p, norm_pix)
    assert p == 16 and c["rows"] == 18
    pred, img, dmse = c["pred"].cuda(), c["img"].cuda(), c["dmse"].cuda()
    forms = {"contiguous": (pred, img), "ldp=772": (_row_strided(pred, 772), img),
             "ldp=770": (_row_strided(pred, 770), img), "pred+1": (_offset_copy(pred), img),
             "img+1": (pred, _offset_copy(img))}
    assert forms["ldp=772"][0].data_ptr() % 8 == 0 and forms["pred+1"][0].data_ptr() % 8 == 2
    assert forms["img+1"][1].data_ptr() % 16 == 1 and img.data_ptr() % 16 == 0
    got = {}
    for name, (pr, im) in forms.items():
        got[name] = _mse_run(ext, pr, im, dmse, p, norm_pix)
        _mse_check(c, *got[name], f"patch_mse p16 {name}")
    for name in forms:
        assert _same_bits(got[name][0], got["contiguous"][0]), name
        assert _same_bits(got[name][1], got["contiguous"][1]), name


@pytest.mark.parametrize("shape", [(3, 32, 48, 16), (2, 16, 24, 8), (1, 28, 42, 14)], ids=_sid)
def test_patch_mse_bwd_skips_zero_rows(ext, shape):
    """dmse == 0 (-0.0 too) rows are zero bits and are not read: a NaN row of pred stays out."""
    p = shape[3]
    c = M.mse_case(*shape, True)
    pred, dmse = c["pred"].clone(), c["dmse"].clone()
    assert dmse[0] == 0 and dmse[3] == 0 and dmse[1] != 0
    dmse[3] = -0.0
    pred[0] = float("nan")
    pred[3] = float("nan")
    for pr in (pred.cuda(), _row_strided(pred.cuda(), c["P3"] + 2)):
        dpred = ext.patch_mse_bwd(pr, c["img"].cuda(), dmse.cuda(), p, True).cpu()
        live = dmse != 0
        assert (M.bits16(dpred[~live]) == 0).all()
        assert _same_bits(dpred[live], ext.patch_mse_bwd(c["pred"].cuda(), c["img"].cuda(), c["dmse"].cuda(), p,
                                                         True).cpu()[live])


def test_patch_mse_limit_and_shapes(ext):
    """3 p^2 > 1024 has no kernel: the binding says so, ops.patch_mse composes in torch."""
    B, H, W, p = 1, 20, 40, 20
    img = M.coded_images(B, H, W).cuda()
    g = torch.Generator().manual_seed(20)
    pred = torch.randn(2, 1200, generator=g).to(BF16).cuda()
    dmse = torch.ones(2, device="cuda")
    with pytest.raises(RuntimeError, match="patch_mse_fwd"):
        ext.patch_mse_fwd(pred, img, p, False)
    with pytest.raises(RuntimeError, match="patch_mse_bwd"):
        ext.patch_mse_bwd(pred, img, dmse, p, False)
    for norm_pix in (False, True):
        t = mae_ops.normalized_patches(img, p)
        t = mae_ops.norm_pix(t) if norm_pix else t
        want = (t - pred.float().view(B, 2, -1)).square().mean(-1)
        got = mae_ops.patch_mse(pred, img, p, norm_pix)
        assert got.shape == (B, 2) and torch.equal(got, want)
        ref = M.patch_mse64(pred.cpu(), img.cpu(), p, norm_pix)
        assert ((got.cpu().view(-1).double() - ref).abs() <= 1e-5 * ref).all()  # the composition, not a kernel
    # the width of pred is checked on both sides
    img16 = M.coded_images(1, 16, 16).cuda()
    for bad in (torch.zeros(1, 764, dtype=BF16, device="cuda"), torch.zeros(1, 772, dtype=BF16, device="cuda")):
        with pytest.raises(RuntimeError, match="shapes"):
            ext.patch_mse_fwd(bad, img16, 16, False)
        with pytest.raises(RuntimeError, match="shapes"):
            ext.patch_mse_bwd(bad, img16, torch.ones(1, device="cuda"), 16, False)


# ------------------------------------------------------------------ patchify / gather
@pytest.mark.parametrize("shape", M.PATCH_SHAPES, ids=_sid)
def test_patchify_normalize(ext, shape):
    B, H, W, p = shape
    img = M.patch_images(B, H, W, p)
    ref64, comp32 = M.patches64(img, p), M.patches32(img, p)
    out = ext.patchify_normalize(img.cuda(), p).cpu()
    M.check_f32(out, ref64, comp32, f"patchify {shape} ({'word' if W % 4 == 0 else 'byte'} loads)")
    assert _same_bits(out, ext.patchify_normalize(img.cuda(), p).cpu())
    off = _offset_copy(img.cuda())  # base not 4-byte aligned: byte loads, the same values
    assert off.data_ptr() % 4 == 1
    assert _same_bits(out, ext.patchify_normalize(off, p).cpu())


@pytest.mark.parametrize("shape", M.PATCH_SHAPES, ids=_sid)
def test_gather_patches(ext, shape):
    B, H, W, p = shape
    N = (H // p) * (W // p)
    img = M.patch_images(B, H, W, p)
    dev, off = img.cuda(), _offset_copy(img.cuda())
    for name, ids in M.gather_ids(B, N, seed=p).items():
        K = ids.shape[-1]
        out = ext.gather_patches(dev, ids.cuda(), p)
        assert out.dtype == BF16 and out.shape == (B * K, 3 * p * p)
        if K == 0:
            continue
        if name.startswith("ends"):
            assert (ids == 0).any() and (ids == N - 1).any()
        M.check_bf16(out.cpu(), M.gather64(img, ids, p), M.gather32(img, ids, p), f"gather {shape} {name}")
        assert _same_bits(out, ext.gather_patches(dev, ids.cuda(), p))
        assert _same_bits(out, ext.gather_patches(off, ids.cuda(), p))  # p = 16: the byte kernel


# ------------------------------------------------------------------ mix_patches
def _mix(ext, img, p, mode, ratio=1.0, perm=None, box=(0, 0, 0, 0)):
    """Device buffers as Mixup.plan delivers them: params [mode, ratio, label_w] fp32, box int32, perm int32."""
    if mode == 0 and perm is None:
        return ext.mix_patches(img, None, None, None, p)
    prm = torch.tensor([float(mode), ratio, 1.0], dtype=torch.float32, device="cuda")
    bx = torch.tensor(list(box), dtype=torch.int32, device="cuda")
    return ext.mix_patches(img, perm.cuda(), prm, bx, p)


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "byte-offset"])
@pytest.mark.parametrize("shape", M.MIX_SHAPES, ids=_sid)
def test_mix_patches(ext, shape, offset):
    B, H, W, p = shape
    N = (H // p) * (W // p)
    img = M.patch_images(B, H, W, p)
    dev = _offset_copy(img.cuda()) if offset else img.cuda()
    perm = M.mix_perm(B)
    pl = perm.long()
    none = (0, 0, 0, 0)

    mode0 = _mix(ext, dev, p, 0).cpu()
    M.check_bf16(mode0, M.mix64(img, p, 0, 1.0, perm, none), M.mix32(img, p, 0, 1.0, perm, none), f"mix {shape} mode 0")
    assert _same_bits(mode0, _mix(ext, dev, p, 0, 0.3, perm, (5, 27, 3, 41)).cpu())  # mode 0 through the buffers
    assert _same_bits(mode0, ext.gather_patches(dev, torch.arange(N, dtype=torch.int32, device="cuda"), p).cpu())
    mode0_perm = mode0.view(B, N, -1)[pl].reshape(mode0.shape)
    assert not _same_bits(mode0, mode0_perm)

    for r in M.MIX_RATIOS:
        out = _mix(ext, dev, p, 1, r, perm).cpu()
        M.check_bf16(out, M.mix64(img, p, 1, r, perm, none), M.mix32(img, p, 1, r, perm, none), f"mixup {shape} r={r}")
        assert _same_bits(out, _mix(ext, dev, p, 1, r, perm).cpu())
        if r == 1.0:
            assert _same_bits(out, mode0)
        if r == 0.0:
            assert _same_bits(out, mode0_perm)

    for name in M.MIX_BOXES:
        box = M.mix_box(name, H, W)
        out = _mix(ext, dev, p, 2, 0.3, perm, box).cpu()
        inside = M.patches_of(M.box_mask(H, W, box).expand(B, 3, H, W).contiguous(), p).reshape(mode0.shape)
        assert int(inside.sum()) == 3 * B * (box[1] - box[0]) * (box[3] - box[2])
        assert _same_bits(out, torch.where(inside, mode0_perm, mode0)), name
        M.check_bf16(out, M.mix64(img, p, 2, 0.3, perm, box), M.mix32(img, p, 2, 0.3, perm, box), f"cutmix {shape} {name}")
        if name == "empty":
            assert _same_bits(out, mode0)
        if name == "full":
            assert _same_bits(out, mode0_perm)


def test_mix_patches_word_and_byte_kernels_agree(ext):
    B, H, W, p = M.MIX_SHAPES[0]
    img = M.patch_images(B, H, W, p).cuda()
    off = _offset_copy(img)
    perm = M.mix_perm(B)
    for mode, r, box in ((0, 1.0, (0, 0, 0, 0)), (1, 0.3, (0, 0, 0, 0)), (2, 0.3, (5, 27, 3, 41))):
        assert _same_bits(_mix(ext, img, p, mode, r, perm, box), _mix(ext, off, p, mode, r, perm, box)), mode


# ------------------------------------------------------------------ embed_finish / unshuffle
# (D or d, C, N, K, B); the last one has B (C + N) = 150 rows: above 128 and no multiple of 64
GLUE_SHAPES = [(4, 1, 6, 1, 3), (20, 3, 6, 6, 2), (384, 1, 16, 4, 3), (768, 3, 16, 4, 2), (1024, 1, 9, 2, 3),
               (384, 1, 49, 12, 3)]


def _glue_ids(B, N, K, per_sample, seed):
    g = torch.Generator().manual_seed(seed)
    noise = torch.rand((B, N) if per_sample else (N,), generator=g)
    _, restore, keep, _ = M.mask_ids_ref(noise.view(-1, N), K)
    if not per_sample:
        restore, keep = restore[0], keep[0]
    return restore.to(torch.int32), keep.to(torch.int32)


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("shape", GLUE_SHAPES, ids=_sid)
def test_embed_finish(ext, shape, per_sample):
    D, C, N, K, B = shape
    assert (B * (C + K) * (D // 4)) % 256 != 0 or D == 1024  # the last grid block is partial
    g = torch.Generator().manual_seed(D + N)
    _, keep = _glue_ids(B, N, K, per_sample, seed=D)
    cls = torch.randn(C, D, generator=g)
    for exact in (True, False):
        e = M.small_int_bf16((B * K, D), g) if exact else torch.randn(B * K, D, generator=g).to(BF16)
        pos = M.dyadic_f32((N, D), g) if exact else torch.randn(N, D, generator=g)
        for ps in (pos, None):
            out = ext.embed_finish(e.cuda(), None if ps is None else ps.cuda(), keep.cuda(), cls.cuda(), B).cpu()
            ref = M.embed_finish64(e, ps, keep, cls, B)
            assert out.shape == (B, C + K, D) and out.dtype == torch.float32
            assert _same_bits(out, ref.float())  # one fp32 add: the correctly rounded sum
            if exact:
                assert torch.equal(out.double(), ref)


@pytest.mark.parametrize("per_sample", [False, True], ids=["shared", "per-sample"])
@pytest.mark.parametrize("shape", GLUE_SHAPES, ids=_sid)
def test_unshuffle(ext, shape, per_sample):
    """The mask-token gradient of RANDOM dout is a column sum of normal values that cancels: one fp32
    ulp of the result lies far below the rounding of its terms, so the bound asks for the correctly
    rounded sum.  Measured on an MI355X: worst miss <= 0.5 ulp in every case.  With fp32 sums and
    partials the kernel missed it in 9 of the 12 cases (worst miss / bound 1.8 .. 191, up to 7296 ulps
    of a cancelled sum); it now sums in fp64 and the binding rounds once."""
    d, C, N, K, B = shape
    assert (B * (C + N) * (d // 4)) % 256 != 0 or d == 1024  # partial last grid block of the forward
    g = torch.Generator().manual_seed(d + N + 1)
    restore, _ = _glue_ids(B, N, K, per_sample, seed=d + 1)
    for exact in (True, False):
        y = M.small_int_bf16((B, C + K, d), g) if exact else torch.randn(B, C + K, d, generator=g).to(BF16)
        tok = M.dyadic_f32((d,), g) if exact else torch.randn(d, generator=g)
        pos = M.dyadic_f32((N, d), g) if exact else torch.randn(N, d, generator=g)
        out = ext.unshuffle_fwd(y.cuda(), tok.cuda(), restore.cuda(), pos.cuda(), C).cpu()
        ref = M.unshuffle_fwd64(y, tok, restore, pos, C)
        assert _same_bits(out, ref.float())
        if exact:
            assert torch.equal(out.double(), ref)

        dout = M.dyadic_f32((B, C + N, d), g) if exact else torch.randn(B, C + N, d, generator=g)
        dy, part = ext.unshuffle_bwd(dout.cuda(), restore.cuda(), C, K)
        dy2, part2 = ext.unshuffle_bwd(dout.cuda(), restore.cuda(), C, K)
        assert _same_bits(dy, dy2) and _same_bits(part, part2)
        dy, part = dy.cpu(), part.cpu()
        assert part.shape == (1, d) and part.dtype == torch.float32  # the blocks' fp64 partials, summed
        dy64, dtok64 = M.unshuffle_bwd64(dout.to(BF16).float(), restore, C, K)  # dout.bfloat16() gathered
        assert _same_bits(dy, dy64.to(BF16))
        _, dtok64 = M.unshuffle_bwd64(dout, restore, C, K)
        if K == N:
            assert (part.view(torch.int32) == 0).all()
        elif exact:  # sums of multiples of 1/16: exact in fp32 in any order
            assert torch.equal(part.sum(0).double(), dtok64)
        else:  # the fp32 composition: autograd of ops.unshuffle
            tr = tok.clone().requires_grad_()
            mae_ops.unshuffle(y.float(), tr, restore.long(), pos, C).backward(dout)
            M.check_f32(part.sum(0), dtok64, tr.grad, f"unshuffle_bwd {shape} dtok")


@pytest.mark.parametrize("d", [1028, 1032])
def test_unshuffle_width_limit(ext, d, monkeypatch):
    """d > 1024: the backward has no kernel (the binding raises) and unshuffle_fused composes in torch."""
    B, C, N, K = 1, 1, 3, 1
    g = torch.Generator().manual_seed(d)
    restore = torch.tensor([2, 0, 1], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="unshuffle_bwd"):
        ext.unshuffle_bwd(torch.zeros(B, C + N, d, device="cuda"), restore, C, K)
    y = torch.randn(B, C + K, d, generator=g).to(BF16).cuda()
    tok, pos = torch.randn(d, generator=g).cuda(), torch.randn(N, d, generator=g).cuda()

    class Tok:  # the part of a parameter Handle that the torch path touches
        def note_use(self):
            pass

    from jumbo_mae_tpu_amd.ops import params_fn
    monkeypatch.setattr(params_fn, "param_value", lambda h: tok)
    monkeypatch.setattr(mae_ops._Unshuffle, "apply", lambda *a: pytest.fail("the HIP path was taken"))
    out = mae_ops.unshuffle_fused(y, Tok(), restore.long(), pos, C)
    assert torch.equal(out, mae_ops.unshuffle(y, tok, restore.long(), pos, C))
    assert _same_bits(out.cpu(), M.unshuffle_fwd64(y.cpu(), tok.cpu(), restore.cpu(), pos.cpu(), C).float())


# ------------------------------------------------------------------ mask_ids
def _mask_ids_check(ext, noise, keep):
    sh, rs, keep32, rs32, mask = ext.mask_ids(noise.cuda().contiguous(), keep)
    x = noise.view(-1, noise.shape[-1])
    r_sh, r_rs, r_keep, r_mask = M.mask_ids_ref(x, keep)
    t_sh = torch.argsort(x, dim=-1, stable=True)
    assert torch.equal(r_sh, t_sh) and torch.equal(r_rs, torch.argsort(t_sh, dim=-1, stable=True))
    assert sh.dtype == torch.int64 and keep32.dtype == torch.int32 and sh.shape == noise.shape
    assert torch.equal(sh.cpu().view_as(r_sh), r_sh) and torch.equal(rs.cpu().view_as(r_rs), r_rs)
    assert torch.equal(rs32.cpu().long().view_as(r_rs), r_rs)
    assert torch.equal(keep32.cpu().long().view(x.shape[0], keep), r_keep)
    assert torch.equal(mask.cpu().view_as(r_mask), r_mask)


def test_mask_ids_edges(ext):
    g = torch.Generator().manual_seed(6)
    _mask_ids_check(ext, torch.rand(1, generator=g), 1)  # N = 1
    _mask_ids_check(ext, torch.rand(1, generator=g), 0)
    _mask_ids_check(ext, torch.rand(3, 1, generator=g), 1)
    _mask_ids_check(ext, torch.rand(2, 1024, generator=g), 1024)  # keep = N at the row limit
    same = torch.full((2, 37), 0.25)
    _mask_ids_check(ext, same, 9)
    sh = ext.mask_ids(same.cuda(), 9)[0].cpu()
    assert torch.equal(sh, torch.arange(37).expand(2, 37))  # all equal: the identity
    x = torch.rand(3, 41, generator=g)
    x[:, 5::6] = x[:, 2:3]  # repeated values
    x[0, :8] = torch.tensor([0.0, -0.0, float("inf"), 0.0, -0.0, float("inf"), 0.5, -0.0])
    x[1, 30:34] = torch.tensor([float("inf"), 0.0, -0.0, float("inf")])
    _mask_ids_check(ext, x, 10)
    _mask_ids_check(ext, x[0].clone(), 41)
