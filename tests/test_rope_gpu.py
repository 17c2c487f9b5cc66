"""csrc/rope.hip ``jm_rope_apply`` against ``rope_torch`` (ops/rope.py) in fp64, fed the same fp32 table and
the same (bf16 or fp32) input values.

Per-element bound, derived: with |c|, |s| <= 1 the kernel's two fp32 products carry at most
2^-24 (|x0| + |x1|) together, the fp32 add at most 2^-24 |o| <= 2^-24 (|x0| + |x1|) more; required is
|got - ref| <= 2^-22 (|x0| + |x1|) + u, u = half a bf16 ulp of |ref| for bf16 output and 0 for fp32."""

import os
import subprocess
import sys
import textwrap

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GW, G = 3, 4


def _table(hd, G=G):
    from jumbo_mae_tpu_amd.ops.rope import rope_table
    return rope_table(G, hd, 100.0, DEV)


def _pos(kind, B, Sp):
    g = torch.Generator().manual_seed(7)
    if kind == "none":
        return None
    if kind == "shared":
        return torch.randperm(9, generator=g)[:Sp].to(torch.int32).to(DEV)
    rows = torch.stack([torch.randperm(9, generator=g)[:Sp] for _ in range(B)])
    assert not torch.equal(rows[0], rows[1])
    return rows.to(torch.int32).to(DEV)


def _input(B, S, H, hd, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, S, 3 * H * hd, generator=g) * 2.0).to(dtype).to(DEV)


def _half_ulp_bf16(ref):
    """half a bf16 ulp (8 significant bits) of |ref|, fp64; the smallest normal's below it"""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=ref.device), e - 7)


def _check(got, x, heads, n_cls, gw, table, pos, inverse):
    """got (the tensor's dtype) against the fp64 oracle on the same input values, element by element."""
    from jumbo_mae_tpu_amd.ops.rope import rope_torch
    B, S, W = x.shape
    hd = W // (3 * heads)
    ref = rope_torch(x.double(), heads, n_cls, gw, table, pos, inverse)
    pair = x.double().abs().view(B, S, 3, heads, hd // 2, 2).sum(-1, keepdim=True).expand(B, S, 3, heads, hd // 2, 2)
    bound = 2.0 ** -22 * pair.reshape(B, S, W)
    if x.dtype == torch.bfloat16:
        bound = bound + _half_ulp_bf16(ref)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), (err - bound).max().item()
    x5, g5 = x.view(B, S, 3, heads, hd), got.view(B, S, 3, heads, hd)
    assert torch.equal(x5[:, :, 2], g5[:, :, 2]) and torch.equal(x5[:, :n_cls], g5[:, :n_cls])  # v, CLS rows: bits
    if S > n_cls:
        assert not torch.equal(x5[:, n_cls:, :2], g5[:, n_cls:, :2])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hd", [32, 64, 80, 96, 128])
def test_kernel_matches_fp64_oracle(hd, dtype):
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    B, H = 2, 3
    table = _table(hd)
    for n_cls in (0, 3):
        S = n_cls + 5
        x = _input(B, S, H, hd, dtype, seed=hd + n_cls)
        for kind in ("none", "shared", "per-sample"):
            pos = _pos(kind, B, 5)
            for inverse in (False, True):
                got = x.clone()
                out = ext.rope_apply(got, H, n_cls, GW, table, pos, inverse)
                assert out.data_ptr() == got.data_ptr()  # in place
                _check(got, x, H, n_cls, GW, table, pos, inverse)
                again = x.clone()
                ext.rope_apply(again, H, n_cls, GW, table, pos, inverse)
                assert torch.equal(got.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                   again.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_row_count_that_is_no_multiple_of_a_workgroups_share(dtype):
    """B S = 1031 rows (1028 patch rows on a 33-wide grid): the last workgroup is partly filled."""
    from jumbo_mae_tpu_amd.ops import _ext
    from jumbo_mae_tpu_amd.ops.rope import rope_table
    H, hd, n_cls, gw = 3, 32, 3, 33
    table = rope_table(33, hd, 100.0, DEV)
    x = _input(1, 1031, H, hd, dtype, seed=11)
    guard = torch.full((4096,), 3.0, dtype=dtype, device=DEV)  # right behind x in a shared buffer
    buf = torch.cat([x.reshape(-1), guard])
    got = buf[:x.numel()].view_as(x)
    _ext.load(True).rope_apply(got, H, n_cls, gw, table, None, False)
    _check(got, x, H, n_cls, gw, table, None, False)
    assert bool((buf[x.numel():] == 3.0).all())


def test_composition_path_same_bound():
    """``_ROPE_OURS = False`` and a head dim without the kernel (48) take ``rope_torch``: same bound."""
    from jumbo_mae_tpu_amd.ops import prims as P
    B, H, n_cls = 2, 3, 3
    pos = _pos("per-sample", B, 5)
    for hd, ours in ((64, False), (48, True)):
        table = _table(hd)
        for dtype in (torch.bfloat16, torch.float32):
            x = _input(B, n_cls + 5, H, hd, dtype, seed=hd)
            saved = P._ROPE_OURS
            try:
                P._ROPE_OURS = ours
                got = x.clone()
                assert P.rope_(got, H, n_cls, GW, table, pos) is got
            finally:
                P._ROPE_OURS = saved
            _check(got, x, H, n_cls, GW, table, pos, False)
    # and the switch left on runs the kernel: the same result within both bounds, v untouched
    x = _input(B, n_cls + 5, H, 64, torch.bfloat16, seed=64)
    got = P.rope_(x.clone(), H, n_cls, GW, _table(64), pos)
    _check(got, x, H, n_cls, GW, _table(64), pos, False)


def test_inverse_is_the_adjoint():
    """fp32 I/O: <R x, y> == <x, R^T y> in fp64 within 1e-5 relative -- the kernel's backward is the transpose."""
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    B, H, hd, n_cls = 2, 3, 64, 3
    table = _table(hd)
    pos = _pos("per-sample", B, 5)
    x = _input(B, n_cls + 5, H, hd, torch.float32, seed=1)
    y = _input(B, n_cls + 5, H, hd, torch.float32, seed=2)
    rx = ext.rope_apply(x.clone(), H, n_cls, GW, table, pos, False)
    rty = ext.rope_apply(y.clone(), H, n_cls, GW, table, pos, True)
    a = (rx.double() * y.double()).sum().item()
    b = (x.double() * rty.double()).sum().item()
    scale = (x.double().norm() * y.double().norm()).item()
    assert abs(a - b) <= 1e-5 * scale, (a, b, scale)
    back = ext.rope_apply(rx.clone(), H, n_cls, GW, table, pos, True)
    assert (back - x).abs().max().item() <= 1e-5


def test_bad_arguments_are_refused():
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    x = _input(2, 8, 3, 32, torch.bfloat16)
    with pytest.raises(RuntimeError, match="table"):
        ext.rope_apply(x, 3, 3, GW, _table(64), None, False)  # a table of another head dim
    with pytest.raises(RuntimeError, match="pos"):
        ext.rope_apply(x, 3, 3, GW, _table(32), torch.zeros(4, dtype=torch.int32, device=DEV), False)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ext.rope_apply(_input(2, 8, 3, 24, torch.bfloat16), 3, 3, GW, _table(24), None, False)
    with pytest.raises(RuntimeError, match="fewer positions"):
        ext.rope_apply(_input(1, 16, 3, 32, torch.bfloat16), 3, 0, GW, _table(32), None, False)  # 16 rows > 4 x 3


DEBUG_SCRIPT = textwrap.dedent("""
    import torch
    from jumbo_mae_tpu_amd.ops import _ext
    from jumbo_mae_tpu_amd.ops.rope import rope_table
    ext = _ext.load(True)
    assert ext.__name__.endswith("_C_debug") and ext.debug_build
    table = rope_table(4, 32, 100.0, "cuda")
    x = torch.randn(2, 8, 3 * 3 * 32, device="cuda").bfloat16()
    good = torch.tensor([0, 11, 5, 7, 2], dtype=torch.int32, device="cuda")
    ext.rope_apply(x.clone(), 3, 3, 3, table, good, False)
    assert ext.debug_lines() == {}, ext.debug_lines()
    for bad in (12, -1):                       # outside 0 <= p < G * gw = 12: reported, nothing traps
        pos = good.clone()
        pos[2] = bad
        y = ext.rope_apply(x.clone(), 3, 3, 3, table, pos, False)
        torch.cuda.synchronize()
        lines = ext.debug_lines()
        assert set(lines) == {"rope"} and lines["rope"] > 0, lines
        assert ext.debug_lines() == {}         # reading cleared it
        assert torch.isfinite(y.float()).all()
    print("ROPE_DEBUG_OK")
""")


def test_debug_build_reports_out_of_range_positions():
    so = [f for f in os.listdir(os.path.join(ROOT, "jumbo_mae_tpu_amd")) if f.startswith("_C_debug")]
    if not so:
        pytest.fail("debug extension not built: python -m jumbo_mae_tpu_amd.csrc.build --variant debug")
    env = dict(os.environ, JMAE_EXT="debug", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", DEBUG_SCRIPT], capture_output=True, text=True, timeout=110, env=env,
                       cwd=ROOT)
    assert r.returncode == 0 and "ROPE_DEBUG_OK" in r.stdout, (r.stdout[-3000:], r.stderr[-3000:])
