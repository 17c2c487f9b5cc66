"""csrc/qknorm.hip (``jm_qknorm_fwd`` / ``jm_qknorm_bwd``) against ``qknorm_torch`` (ops/qknorm.py) in fp64,
fed the same (bf16 or fp32) input bits, the same fp32 scales and the same fp32 rotation table.

Forward bound, per element, derived for the kernel's operation order (sum of squares in fp32, divided by
hd, plus eps, square root, reciprocal, then (x r) g, then the rotation of rope.hip, one rounding to the
tensor's dtype): the fp32 sum of hd squares carries at most hd 2^-24 relative error and enters r halved; the
division by hd, add-eps, sqrt and reciprocal cost 4 roundings (the first three halved as well -- counted
whole), the two products 2: at most (hd/2 + 6) 2^-24 |y| before the rotation, which adds
2^-22 (|y0| + |y1|) (tests/test_rope_gpu.py).  Required:
|got - ref| <= (hd/2 + 12) 2^-24 (|y0| + |y1|) + u over the oracle's pre-rotation pair, u = half a bf16 ulp
of |ref| for bf16 and 0 for fp32.

Backward: dx, dg_q and dg_k against fp64 autograd of ``qknorm_torch`` on the same bits, per element within
max(2 x the error of the fp32 composition on the same bits, 1 fp32 ulp of the value) -- the rule of
tests/test_cls_loss_gpu.py and tests/test_batchnorm_gpu.py, computed here from the composition, never from
the kernel -- plus half a bf16 ulp of the value for a bf16 dx."""

import os
import subprocess
import sys
import textwrap

import pytest
import torch

from bn_ref import bound as comp_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GW, G = 3, 4
B, H = 2, 3
KINDS = ("none", "shared", "per-sample")


def _ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def _rope(kind, n_cls, hd, B=B, Sp=5):
    """An ``ops.rope.Rope`` on the GPU, or None.  ``order``: patch t - n_cls (no pos list)."""
    from jumbo_mae_tpu_amd.ops.rope import Rope, rope_table
    if kind == "none":
        return None
    table = rope_table(G, hd, 100.0, DEV)
    g = torch.Generator().manual_seed(7)
    if kind == "shared":
        pos = torch.randperm(9, generator=g)[:Sp].to(torch.int32).to(DEV)
    else:
        rows = torch.stack([torch.randperm(9, generator=g)[:Sp] for _ in range(B)])
        assert not torch.equal(rows[0], rows[1])
        pos = rows.to(torch.int32).to(DEV)
    return Rope(n_cls, GW, table, pos)


def _args(rope):
    return (0, 1, None, None) if rope is None else (rope.n_cls, rope.gw, rope.table, rope.pos)


def _input(B, S, H, hd, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, S, 3 * H * hd, generator=g) * 2.0).to(dtype).to(DEV)
    gq = (1 + 0.5 * torch.randn(hd, generator=g)).to(DEV)
    gk = (1 + 0.5 * torch.randn(hd, generator=g)).to(DEV)
    return x, gq, gk


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _half_ulp_bf16(ref):
    """half a bf16 ulp (8 significant bits) of |ref|, fp64; the smallest normal's below it"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=ref.device), e - 7)


def _fwd_bound(x, heads, gq, gk, rope):
    """(ref, bound) of the forward on the bits of x: the module docstring's bound."""
    from jumbo_mae_tpu_amd.ops.qknorm import qknorm_torch
    Bx, S, W = x.shape
    hd = W // (3 * heads)
    ref = qknorm_torch(x.double(), heads, gq.double(), gk.double(), rope)
    pre = qknorm_torch(x.double(), heads, gq.double(), gk.double(), None)
    pair = pre.abs().view(Bx, S, 3, heads, hd // 2, 2).sum(-1, keepdim=True).expand(Bx, S, 3, heads, hd // 2, 2)
    bound = (hd / 2 + 12) * 2.0 ** -24 * pair.reshape(Bx, S, W)
    if x.dtype == torch.bfloat16:
        bound = bound + _half_ulp_bf16(ref)
    return ref, bound


def _check_fwd(x, heads, gq, gk, rope, what):
    """One forward launch, twice: the bound, v's and saved's bits, determinism.  Returns (out, saved)."""
    ext = _ext()
    Bx, S, W = x.shape
    hd = W // (3 * heads)
    got = x.clone()
    saved = ext.qknorm_fwd(got, heads, gq, gk, *_args(rope))
    again = x.clone()
    saved2 = ext.qknorm_fwd(again, heads, gq, gk, *_args(rope))
    assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(saved), _bits(saved2)), what
    ref, bound = _fwd_bound(x, heads, gq, gk, rope)
    x5, g5 = x.view(Bx, S, 3, heads, hd), got.view(Bx, S, 3, heads, hd)
    err = (got.double() - ref).abs().view(Bx, S, 3, heads, hd)[:, :, :2]
    bnd = bound.view(Bx, S, 3, heads, hd)[:, :, :2]
    worst = (err / bnd.clamp_min(1e-300)).max().item()
    print(f"{what}: forward err / bound {worst:.3f}")
    assert bool((err <= bnd).all()), (what, worst)
    assert torch.equal(_bits(x5[:, :, 2]), _bits(g5[:, :, 2])), what  # v: bits
    assert saved.dtype == x.dtype and tuple(saved.shape) == (Bx, S, 2 * heads * hd) and saved.is_contiguous()
    assert torch.equal(_bits(saved.view(Bx, S, 2, heads, hd)), _bits(x5[:, :, :2])), what  # the input q|k bits
    return got, saved


def _grads(x, dy, heads, gq, gk, rope, dtype):
    """(dx, dg_q, dg_k) of sum(qknorm_torch(x) * dy) by autograd with everything in ``dtype``."""
    from jumbo_mae_tpu_amd.ops.qknorm import qknorm_torch
    xa, qa, ka = (t.to(dtype).requires_grad_(True) for t in (x, gq, gk))
    y = qknorm_torch(xa, heads, qa, ka, rope)
    return torch.autograd.grad((y * dy.to(dtype)).sum(), (xa, qa, ka))


def _check_bwd(x, dy, heads, gq, gk, rope, what, saved=None):
    """One backward launch, twice, on the bits of x (saved) and dy: the module docstring's rule."""
    ext = _ext()
    Bx, S, W = x.shape
    hd = W // (3 * heads)
    if saved is None:
        saved = x.view(Bx, S, 3, heads, hd)[:, :, :2].reshape(Bx, S, -1).clone(memory_format=torch.contiguous_format)
    got = dy.clone()
    dg = ext.qknorm_bwd(got, saved, heads, gq, gk, *_args(rope))
    again = dy.clone()
    dg2 = ext.qknorm_bwd(again, saved, heads, gq, gk, *_args(rope))
    assert torch.equal(_bits(got), _bits(again)) and torch.equal(_bits(dg), _bits(dg2)), what
    assert dg.dtype == torch.float32 and tuple(dg.shape) == (2, hd)
    assert torch.isfinite(got.float()).all() and torch.isfinite(dg).all(), what
    d5, g5 = dy.view(Bx, S, 3, heads, hd), got.view(Bx, S, 3, heads, hd)
    assert torch.equal(_bits(d5[:, :, 2]), _bits(g5[:, :, 2])), what  # the v third: bits
    r64 = _grads(x, dy, heads, gq, gk, rope, torch.float64)
    r32 = _grads(x, dy, heads, gq, gk, rope, torch.float32)
    out = {}
    for name, val, v32, v64 in (("dx", g5[:, :, :2], r32[0].view(d5.shape)[:, :, :2], r64[0].view(d5.shape)[:, :, :2]),
                                ("dg_q", dg[0], r32[1], r64[1]), ("dg_k", dg[1], r32[2], r64[2])):
        bnd = comp_bound(v32, v64)
        if name == "dx" and x.dtype == torch.bfloat16:
            bnd = bnd + _half_ulp_bf16(v64)
        err = (val.double() - v64).abs()
        out[name] = (err / bnd).max().item()
    print(f"{what}: backward err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    assert all(v <= 1.0 for v in out.values()), (what, out)
    return got, dg


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [32, 64, 80, 96, 128])
def test_forward_matches_fp64_oracle(hd, dtype):
    for n_cls in (0, 3):
        x, gq, gk = _input(B, n_cls + 5, H, hd, dtype, seed=hd + n_cls)
        for kind in KINDS:
            got, _ = _check_fwd(x, H, gq, gk, _rope(kind, n_cls, hd), f"hd {hd} n_cls {n_cls} rope {kind}")
            assert not torch.equal(got, x)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [32, 64, 80, 96, 128])
def test_backward_matches_fp64_autograd(hd, dtype):
    for n_cls in (0, 3):
        x, gq, gk = _input(B, n_cls + 5, H, hd, dtype, seed=hd + n_cls)
        dy = _input(B, n_cls + 5, H, hd, dtype, seed=1000 + hd + n_cls)[0]
        for kind in KINDS:
            _check_bwd(x, dy, H, gq, gk, _rope(kind, n_cls, hd), f"hd {hd} n_cls {n_cls} rope {kind}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [32, 64, 80, 96, 128])
def test_rows_of_very_different_magnitude(hd, dtype):
    """The rows of batch element 1 are 2^10 times those of element 0 (an exact scaling in both dtypes), and
    every head row has its own magnitude: a row sum that took in a lane of another row would show."""
    n_cls = 3
    x, gq, gk = _input(B, n_cls + 5, H, hd, dtype, seed=hd)
    x5 = x.view(B, n_cls + 5, 3, H, hd)
    x5[1] = x5[0] * 1024.0
    x5[:, :, :2] *= 2.0 ** torch.arange(-3, 3, device=DEV, dtype=torch.float32).to(dtype).view(1, 1, 2, H, 1)
    dy = _input(B, n_cls + 5, H, hd, dtype, seed=77 + hd)[0]
    rope = _rope("per-sample", n_cls, hd)
    _check_fwd(x, H, gq, gk, rope, f"magnitudes hd {hd}")
    _check_bwd(x, dy, H, gq, gk, rope, f"magnitudes hd {hd}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_zero_scale_and_zero_row(dtype):
    hd, n_cls = 80, 3
    x, gq, gk = _input(B, n_cls + 5, H, hd, dtype, seed=5)
    dy = _input(B, n_cls + 5, H, hd, dtype, seed=6)[0]
    rope = _rope("shared", n_cls, hd)
    zero = torch.zeros_like(gq)
    got, saved = _check_fwd(x, H, zero, gk, rope, "g_q == 0")
    assert bool((got.view(B, -1, 3, H, hd)[:, :, 0] == 0).all())
    d, dg = _check_bwd(x, dy, H, zero, gk, rope, "g_q == 0", saved)
    assert bool((d.view(B, -1, 3, H, hd)[:, :, 0] == 0).all()) and dg[0].abs().max().item() > 0.1
    x0 = x.clone()
    x0.view(B, -1, 3, H, hd)[1, 4, 1, 2] = 0  # one all-zero k row, a rotated one
    got, saved = _check_fwd(x0, H, gq, gk, rope, "zero row")
    assert bool((got.view(B, -1, 3, H, hd)[1, 4, 1, 2] == 0).all())
    _check_bwd(x0, dy, H, gq, gk, rope, "zero row", saved)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_dg_over_more_than_one_workgroup(dtype):
    """B 3, S 70, H 2, hd 80: 840 head rows in groups of 16 lanes are 53 workgroups of partials."""
    Bx, S, Hx, hd, n_cls = 3, 70, 2, 80, 3
    assert _ext().qknorm_bwd_blocks(Bx, S, Hx, hd) > 1
    x, gq, gk = _input(Bx, S, Hx, hd, dtype, seed=9)
    dy = _input(Bx, S, Hx, hd, dtype, seed=10)[0]
    from jumbo_mae_tpu_amd.ops.rope import Rope, rope_table
    rope = Rope(n_cls, 9, rope_table(9, hd, 100.0, DEV), None)  # 67 patch rows in order on a 9-wide grid
    _check_fwd(x, Hx, gq, gk, rope, "B 3 S 70")
    _check_bwd(x, dy, Hx, gq, gk, rope, "B 3 S 70")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [32, 80])
def test_fused_launch_against_norm_then_rope(hd, dtype):
    """One fused launch against qknorm without rope followed by rope_apply: the separate path rounds to the
    tensor's dtype in between, so both are held to the forward bound (bf16: the rope kernel's own half ulp
    more), not to equal bits."""
    ext = _ext()
    n_cls = 3
    x, gq, gk = _input(B, n_cls + 5, H, hd, dtype, seed=3 + hd)
    rope = _rope("per-sample", n_cls, hd)
    fused = x.clone()
    ext.qknorm_fwd(fused, H, gq, gk, *_args(rope))
    sep = x.clone()
    ext.qknorm_fwd(sep, H, gq, gk)
    ext.rope_apply(sep, H, n_cls, GW, rope.table, rope.pos, False)
    ref, bound = _fwd_bound(x, H, gq, gk, rope)
    assert bool(((fused.double() - ref).abs() <= bound).all())
    extra = 0
    if dtype == torch.bfloat16:  # the intermediate rounding of y: half a bf16 ulp of each element of the pair
        from jumbo_mae_tpu_amd.ops.qknorm import qknorm_torch
        pre = qknorm_torch(x.double(), H, gq.double(), gk.double(), None)
        hu = _half_ulp_bf16(pre).view(B, -1, 3, H, hd // 2, 2).sum(-1, keepdim=True)
        extra = hu.expand(B, n_cls + 5, 3, H, hd // 2, 2).reshape(x.shape)
    assert bool(((sep.double() - ref).abs() <= bound + extra).all())
    assert torch.equal(_bits(fused.view(B, -1, 3, H, hd)[:, :, 2]), _bits(sep.view(B, -1, 3, H, hd)[:, :, 2]))


def test_prims_route_and_composition_path():
    """prims.qknorm_fwd_ / qknorm_bwd_: the kernel for a supported head dim (the same bits as the extension), the
    composition for head dim 48 and with ``_QKNORM_OURS = False`` -- the same forward bound."""
    from jumbo_mae_tpu_amd.ops import prims as P
    n_cls = 3
    x, gq, gk = _input(B, n_cls + 5, H, 64, torch.bfloat16, seed=4)
    rope = _rope("shared", n_cls, 64)
    a, b = x.clone(), x.clone()
    sa = P.qknorm_fwd_(a, H, gq, gk, rope)
    sb = _ext().qknorm_fwd(b, H, gq, gk, *_args(rope))
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(sa), _bits(sb))
    for hd, ours in ((64, False), (48, True)):
        x, gq, gk = _input(B, n_cls + 5, H, hd, torch.bfloat16, seed=hd)
        rope = _rope("shared", n_cls, hd)
        keep = P._QKNORM_OURS
        try:
            P._QKNORM_OURS = ours
            got = x.clone()
            saved = P.qknorm_fwd_(got, H, gq, gk, rope)
            d, dg = P.qknorm_bwd_(torch.ones_like(x), saved, H, gq, gk, rope)
        finally:
            P._QKNORM_OURS = keep
        ref, bound = _fwd_bound(x, H, gq, gk, rope)
        assert bool(((got.double() - ref).abs() <= bound).all())
        assert torch.equal(_bits(saved.view(B, -1, 2, H, hd)), _bits(x.view(B, -1, 3, H, hd)[:, :, :2]))
        assert tuple(dg.shape) == (2, hd) and torch.isfinite(dg).all() and torch.isfinite(d.float()).all()


def test_bad_arguments_are_refused():
    ext = _ext()
    x, gq, gk = _input(2, 8, 3, 32, torch.bfloat16)
    from jumbo_mae_tpu_amd.ops.rope import rope_table
    with pytest.raises(RuntimeError, match="32, 64, 80, 96, 128"):
        x48, q48, k48 = _input(2, 8, 3, 48, torch.bfloat16)
        ext.qknorm_fwd(x48, 3, q48, k48)
    with pytest.raises(RuntimeError, match="g_q and g_k"):
        ext.qknorm_fwd(x, 3, gq[:16].contiguous(), gk)
    with pytest.raises(RuntimeError, match="g_q and g_k"):
        ext.qknorm_fwd(x, 3, gq.bfloat16(), gk)
    with pytest.raises(RuntimeError, match="table"):
        ext.qknorm_fwd(x, 3, gq, gk, 3, GW, rope_table(G, 64, 100.0, DEV))
    with pytest.raises(RuntimeError, match="pos"):
        ext.qknorm_fwd(x, 3, gq, gk, 3, GW, rope_table(G, 32, 100.0, DEV), torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="saved"):
        ext.qknorm_bwd(x, x, 3, gq, gk)


DEBUG_SCRIPT = textwrap.dedent("""
    import torch
    from jumbo_mae_tpu_amd.ops import _ext
    from jumbo_mae_tpu_amd.ops.rope import rope_table
    ext = _ext.load(True)
    assert ext.__name__.endswith("_C_debug") and ext.debug_build
    table = rope_table(4, 32, 100.0, "cuda")
    x = torch.randn(2, 8, 3 * 3 * 32, device="cuda").bfloat16()
    g = torch.ones(32, device="cuda")
    good = torch.tensor([0, 11, 5, 7, 2], dtype=torch.int32, device="cuda")
    saved = ext.qknorm_fwd(x.clone(), 3, g, g, 3, 3, table, good)
    ext.qknorm_bwd(x.clone(), saved, 3, g, g, 3, 3, table, good)
    assert ext.debug_lines() == {}, ext.debug_lines()
    for bad in (12, -1):                       # outside 0 <= p < G * gw = 12: reported, nothing traps
        pos = good.clone()
        pos[2] = bad
        for fwd in (True, False):
            y = x.clone()
            if fwd:
                ext.qknorm_fwd(y, 3, g, g, 3, 3, table, pos)
            else:
                ext.qknorm_bwd(y, saved, 3, g, g, 3, 3, table, pos)
            torch.cuda.synchronize()
            lines = ext.debug_lines()
            assert set(lines) == {"qknorm"} and lines["qknorm"] > 0, lines
            assert ext.debug_lines() == {}         # reading cleared it
            assert torch.isfinite(y.float()).all()
    print("QKNORM_DEBUG_OK")
""")


def test_debug_build_reports_out_of_range_positions():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], capture_output=True, text=True, timeout=110, env=env,
                       cwd=ROOT)
    assert r.returncode == 0 and "QKNORM_DEBUG_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
