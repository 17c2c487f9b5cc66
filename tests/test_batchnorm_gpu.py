"""The fused BatchNorm kernels (csrc/batchnorm.hip) against the torch composition of parallel/syncbn.py
in fp64 on the CPU (tests/bn_ref.py).

Bound, per element of every fp32 output: max(2 x |fp32 composition - fp64 composition|, 1 fp32 ulp of the
value), computed here from the composition, never from the kernel.  A bf16 ``y`` is within 1 bf16
step of the fp64 ``y`` rounded to bf16.

What "the same inputs" are.  Three fp32 tensors travel between the passes and through the two
all-reduces: ``packed`` (mean, mean of squares), ``stats`` (mean, rstd), ``packed_g``.  They are part
of the op's interface, and their fp32 rounding is amplified by mean2 / var in everything computed
from them -- for the composition and for the kernels alike, each with its own rounding.  Against the
oracle evaluated from ``x`` alone, 3 - 5 % of the elements of ``y``, ``var``, ``dgamma`` and ``dx`` of an
implementation that is exact apart from those three roundings miss the bound above (CPU model of
such an implementation, B x J = 2 x 65 ... 2048 x 3072: worst error / bound 7 - 670 for ``y``, 2 - 13 for
``var``, 3 - 10 for ``dgamma``, 16 - 83 for ``dx``): where the composition's own error happens to be
small, the bound is smaller than what the interface permits.  So each pass is held to the bound
against the oracle evaluated on the inputs that pass reads (bn_ref.passes with ``packed`` / ``stats``
/ ``packed_g`` given): ``packed`` and ``dbeta`` from ``x`` / ``dy`` alone, ``y`` / ``stats`` / running
statistics from ``packed``, ``dgamma`` / ``packed_g`` from ``stats``, ``dx`` from ``stats`` and
``packed_g``; the bf16 step is counted from that oracle's ``y`` as well (where gamma xhat and beta cancel,
a y near 0 has steps far smaller than the interface's error: B = 2, J = 192 has an element 4 steps from
the oracle evaluated from ``x``).  End to end from ``x`` the tests assert the backstop |y - y64| <= 4e-5 (1 + |y64|)
on unit-scale inputs with B >= 65; the end-to-end error / bound ratios are printed with the others."""

import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.99
F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16


def _ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def _kernels(x, gamma, beta, dy, ydt, rm, rv, y_out=None, dx_out=None):
    """All five kernels once on GPU tensors (maybe views); the running statistics are updated on copies."""
    ext = _ext()
    rm, rv = rm.clone(), rv.clone()
    packed = ext.bn_stats(x)
    y, stats = ext.bn_apply(x, packed, gamma, beta, rm, rv, EPS, MOM, ydt, y_out)
    dgamma, dbeta, packed_g = ext.bn_bwd_reduce(dy, x, stats, gamma)
    dx = ext.bn_bwd_dx(dy, x, stats, gamma, packed_g, float(x.shape[0]), dx_out)
    return packed, y, stats, rm, rv, dgamma, dbeta, packed_g, dx


def _ratio(got, v32, v64):
    return ((got.cpu().double() - v64).abs() / R.bound(v32, v64)).max().item()


def _check(x, gamma, beta, dy, ydt, what, unit_scale=False, dev=None, y_out=None, dx_out=None):
    """The kernels on ``x`` / ``dy`` (CPU fp32 values; ``dev``: the GPU tensors to run on, maybe views, default
    plain copies; dy in ``ydt``) twice -- bit-identical -- and against the oracle.  Returns the outputs."""
    B, J = x.shape
    g = torch.Generator().manual_seed(B * 7919 + J)
    rm, rv = torch.randn(J, generator=g), 0.5 + torch.rand(J, generator=g)
    xd, dyd = dev if dev is not None else (x.cuda(), dy.to(ydt).cuda())
    args = (xd, gamma.cuda(), beta.cuda(), dyd, ydt, rm.cuda(), rv.cuda())
    out = _kernels(*args, y_out=y_out, dx_out=dx_out)
    again = _kernels(*args, y_out=y_out, dx_out=dx_out)
    torch.cuda.synchronize()
    assert _same(out, again), what
    packed, y, stats, rm1, rv1, dgamma, dbeta, packed_g, dx = (t.cpu() for t in out)
    assert y.dtype == ydt and dx.dtype == F32 and y.shape == dx.shape == (B, J) and stats.shape == (2, J)
    for t in (packed, y.float(), stats, rm1, rv1, dgamma, dbeta, packed_g, dx):
        assert torch.isfinite(t).all(), what

    dyv = dy.to(ydt).float()  # the values the kernels read
    worst = {}
    # from x / dy alone
    e64, e32 = R.passes(x, gamma, beta, dyv, F64), R.passes(x, gamma, beta, dyv, F32)
    worst["packed"] = _ratio(packed, e32[6], e64[6])
    worst["dbeta"] = _ratio(dbeta, e32[4], e64[4])
    # normalisation, from packed
    a64, a32 = R.passes(x, gamma, beta, dyv, F64, packed=packed), R.passes(x, gamma, beta, dyv, F32, packed=packed)
    worst["mean"] = _ratio(stats[0], a32[1], a64[1])
    worst["rstd"] = _ratio(stats[1], a32[7], a64[7])
    worst["running_mean"] = _ratio(rm1, R.running(rm, a32[1]), R.running(rm.double(), a64[1]))
    worst["running_var"] = _ratio(rv1, R.running(rv, a32[2]), R.running(rv.double(), a64[2]))
    if ydt == F32:
        worst["y"] = _ratio(y, a32[0], a64[0])
    else:
        # 1 bf16 step; where the fp32 bound itself is wider than that (a cancelling column), the bound plus a step
        steps = R.bf16_steps(y, a64[0].to(BF16))
        step = (a64[0].to(BF16).float().abs() * 2.0 ** -7).double()
        wide = (y.double() - a64[0]).abs() <= R.bound(a32[0], a64[0]) + step
        assert ((steps <= 1) | wide).all(), (what, steps.max().item())
    # end to end from x: the backstop
    if ydt == F32 and unit_scale and B >= 65:
        assert ((y.double() - e64[0]).abs() <= 4e-5 * (1 + e64[0].abs())).all(), what
    # backward reductions, from stats; dx, from stats and packed_g
    b64 = R.passes(x, gamma, beta, dyv, F64, stats=stats, packed_g=packed_g)
    b32 = R.passes(x, gamma, beta, dyv, F32, stats=stats, packed_g=packed_g)
    worst["dgamma"] = _ratio(dgamma, b32[3], b64[3])
    worst["packed_g"] = _ratio(packed_g, b32[8], b64[8])
    worst["dx"] = _ratio(dx, b32[5], b64[5])
    e2e = {k: _ratio(v, e32[i], e64[i]) for k, v, i in (("y", y.float(), 0), ("dgamma", dgamma, 3), ("dx", dx, 5))
           if not (k == "y" and ydt == BF16)}
    print(f"{what}: worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          " | from x alone (not asserted) " + " ".join(f"{k} {v:.2f}" for k, v in e2e.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return out


def test_tile_sizes_are_the_ones_the_edge_cases_straddle():
    assert _ext().bn_chunk_rows() == 64 and _ext().bn_block_cols() == 64


# chunk = block = 64: 63 / 64 / 65 are both sides of every boundary, 257 / 1000 several tiles with a partial last one
@pytest.mark.parametrize("J", [1, 63, 65, 192, 1000])
@pytest.mark.parametrize("B", [1, 2, 3, 63, 64, 65, 257])
def test_edges(B, J):
    gen = torch.Generator().manual_seed(1000 * B + J)
    x, gamma, beta, dy = R.inputs(B, J, gen)
    for ydt in (F32, BF16):
        _check(x, gamma, beta, dy, ydt, f"B={B} J={J} {str(ydt)[6:]}", unit_scale=True)


_PROD = {}


def _production():
    if not _PROD:
        _PROD["v"] = R.inputs(2048, 3072, torch.Generator().manual_seed(2048))
    return _PROD["v"]


@pytest.mark.parametrize("ydt", [BF16, F32])
def test_production_shape(ydt):
    """2048 x 3072 (the ln-*-vit-l16 presets): bf16 y and dy, fp32 y and dy."""
    _check(*_production(), ydt, f"2048x3072 {str(ydt)[6:]}", unit_scale=True)


@pytest.mark.parametrize("ydt", [BF16, F32])
def test_column_slices_with_poisoned_surroundings(ydt):
    """x, dy, y and dx as column slices of wider NaN-filled tensors: row stride > J, base 4 bytes (x, dx, fp32
    dy, fp32 y) or 2 bytes (bf16) past a 16-byte boundary.  No NaN reaches an output, the bytes around y
    and dx stay what they were, and the results equal those of contiguous tensors bit for bit."""
    B, J, W, off = 67, 130, 143, 2
    gen = torch.Generator().manual_seed(5)
    x, gamma, beta, dy = R.inputs(B, J, gen)

    def wide(v, dt):
        buf = torch.full((B + 2, W), float("nan"), dtype=dt, device="cuda")
        view = buf[1:B + 1, off:off + J]
        if v is not None:
            view.copy_(v.to(dt))
        assert view.stride(0) == W > J and view.data_ptr() % 16 == buf.element_size()  # 4 (fp32) / 2 (bf16) past
        return buf, view

    (_, xv), (_, dyv) = wide(x, F32), wide(dy, ydt)
    ybuf, yv = wide(None, ydt)
    dxbuf, dxv = wide(None, F32)
    out = _check(x, gamma, beta, dy, ydt, f"slices {str(ydt)[6:]}", unit_scale=True, dev=(xv, dyv), y_out=yv, dx_out=dxv)
    assert out[1].data_ptr() == yv.data_ptr() and out[8].data_ptr() == dxv.data_ptr()
    for buf, view in ((ybuf, yv), (dxbuf, dxv)):
        inside = torch.zeros_like(buf, dtype=torch.bool)
        inside[1:B + 1, off:off + J] = True
        assert torch.isnan(buf[~inside]).all() and torch.isfinite(buf[inside].float()).all()
    dense = _check(x, gamma, beta, dy, ydt, f"dense {str(ydt)[6:]}", unit_scale=True)
    assert _same(out, dense)


@pytest.mark.parametrize("B", [1, 64, 256, 1024])
def test_exact_statistics(B):
    """Integers in [-8, 8], B a power of two: packed is the exact mean and mean of squares; dyadic dy: dbeta exact."""
    gen = torch.Generator().manual_seed(B)
    J = 77
    x = torch.randint(-8, 9, (B, J), generator=gen).float()
    dy = torch.randint(-64, 65, (B, J), generator=gen).float() / 256.0
    ext = _ext()
    packed = ext.bn_stats(x.cuda())
    want = torch.cat([x.double().sum(0), (x.double() ** 2).sum(0)]) / B
    assert torch.equal(packed.cpu().double(), want)
    gamma = torch.ones(J).cuda()
    for dt in (F32, BF16):
        y, stats = ext.bn_apply(x.cuda(), packed, gamma, gamma, gamma.clone(), gamma.clone(), EPS, MOM, F32)
        _, dbeta, _ = ext.bn_bwd_reduce(dy.to(dt).cuda(), x.cuda(), stats, gamma)
        assert torch.equal(dbeta.cpu().double(), dy.double().sum(0))


def _structured(B, gen):
    x, gamma, beta, dy = R.inputs(B, 8, gen)
    x[:, 0] = 3.0                                            # constant: var exactly 0
    x[:, 1] = 0.1                                            # constant, its square not representable
    x[:, 2] = 1e3 + 1e-2 * torch.randn(B, generator=gen)     # cancellation in mean2 - mean^2
    x[:, 3] = -1e3 + 1e-2 * torch.randn(B, generator=gen)
    gamma[4] = 0.0
    gamma[5] = 1e-6
    return x, gamma, beta, dy


@pytest.mark.parametrize("B", [1, 2, 130])
def test_structured_columns(B):
    """Constant columns, mean 1e3 with std 1e-2, gamma 0 and 1e-6, B = 1: finite and within bound; a constant
    column and B = 1 have var exactly 0, rstd = 1 / sqrt(eps), y = beta."""
    x, gamma, beta, dy = _structured(B, torch.Generator().manual_seed(B))
    for ydt in (F32, BF16):
        out = _check(x, gamma, beta, dy, ydt, f"structured B={B} {str(ydt)[6:]}")
        packed, y, stats = out[0].cpu(), out[1].cpu(), out[2].cpu()
        const = [0, 1] if B > 1 else list(range(8))
        r0 = torch.rsqrt(torch.tensor(EPS, dtype=F64)).float()
        assert (stats[1, const] == r0).all(), stats[1]
        assert torch.equal(y[:, const].float(), beta[const].to(ydt).float().expand(B, -1))
        assert torch.equal(y[:, 4].float(), beta[4].to(ydt).float().expand(B))


def test_running_statistics_and_eval():
    """Three training calls move the running statistics as three steps of the fp64 recurrence (each step
    within the bound, from the packed and the running statistics it read); the inference pass from them matches the oracle's
    formula and leaves them untouched."""
    ext = _ext()
    B, J = 130, 97
    gen = torch.Generator().manual_seed(8)
    _, gamma, beta, _ = R.inputs(B, J, gen)
    rm, rv = torch.zeros(J).cuda(), torch.ones(J).cuda()
    for step in range(3):
        x = R.inputs(B, J, gen)[0] + step
        r64, r32 = [rm.cpu().double(), rv.cpu().double()], [rm.cpu(), rv.cpu()]  # what this step reads
        packed = ext.bn_stats(x.cuda())
        ext.bn_apply(x.cuda(), packed, gamma.cuda(), beta.cuda(), rm, rv, EPS, MOM, BF16)
        a64 = R.passes(x, gamma, beta, x, F64, packed=packed.cpu())
        a32 = R.passes(x, gamma, beta, x, F32, packed=packed.cpu())
        r64 = [R.running(r64[0], a64[1]), R.running(r64[1], a64[2])]
        r32 = [R.running(r32[0], a32[1]), R.running(r32[1], a32[2])]
        worst = max(_ratio(rm, r32[0], r64[0]), _ratio(rv, r32[1], r64[1]))
        print(f"running statistics after step {step + 1}: worst error / bound {worst:.3f}")
        assert worst <= 1.0
    assert (rm.cpu() != 0).all() and (rv.cpu() != 1).all()
    keep = (rm.clone(), rv.clone())
    x = R.inputs(B, J, gen)[0]
    for ydt in (F32, BF16):
        y = ext.bn_apply_eval(x.cuda(), rm, rv, gamma.cuda(), beta.cuda(), EPS, ydt)
        y2 = ext.bn_apply_eval(x.cuda(), rm, rv, gamma.cuda(), beta.cuda(), EPS, ydt)
        assert _same([y], [y2]) and y.dtype == ydt
        e64 = R.eval_formula(x, gamma, beta, rm.cpu(), rv.cpu(), F64)
        e32 = R.eval_formula(x, gamma, beta, rm.cpu(), rv.cpu(), F32)
        if ydt == F32:
            worst = _ratio(y, e32, e64)
            print(f"eval y: worst error / bound {worst:.3f}")
            assert worst <= 1.0
        else:
            assert R.bf16_steps(y.cpu(), e64.to(BF16)).max().item() <= 1
    assert _same((rm, rv), keep)


# ------------------------------------------------------------------------------------ the head
def _head(dtype=BF16, J=192, labels=1000):
    from jumbo_mae_tpu_amd.models.params import ParamStore
    from jumbo_mae_tpu_amd.models.vit import LinearCLS
    store = ParamStore()
    head = LinearCLS(store, ("head",), J, labels, batch_norm=True)
    store.finalize("cuda", dtype, torch.Generator().manual_seed(0))
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        head.bn_scale.master.copy_(1.0 + 0.5 * torch.randn(J, generator=gen))
        head.bn_bias.master.copy_(torch.randn(J, generator=gen))
        head.dense.k.master.copy_(torch.randn(head.dense.k.shape, generator=gen) / J ** 0.5)
    store.sync_shadow()
    head.init_stats("cuda")
    return store, head


def test_linear_cls_routes_to_the_kernels(monkeypatch):
    """LinearCLS(batch_norm=True) with the switch on against the switch off, same store contents.  The
    Dense gets a bf16 y either way: the fused y is within 1 bf16 step of the composition's cast y, so the
    logits differ by at most 2^-8 sum_k |y_k| |W_ck| plus their own bf16 rounding.  Both paths' fp32
    results are within about 1e-5 of the exact ones relative to the sums of magnitudes they are made
    of (the composition's measured worst: 8e-6 dgamma), so they agree within 4e-5 of those."""
    from jumbo_mae_tpu_amd.ops import prims as P
    from jumbo_mae_tpu_amd.parallel import syncbn
    B, J, L = 96, 192, 1000
    gen = torch.Generator().manual_seed(2)
    x = R.inputs(B, J, gen)[0].cuda()
    dlogits = (torch.randn(B, L, generator=gen) / B).cuda()
    res = {}
    for on in (True, False):
        monkeypatch.setattr(P, "_BN_OURS", on)
        store, head = _head()
        ready = []
        store.hooks.append(lambda h: ready.append(h))
        seen = []
        real = syncbn.sync_batch_norm

        def spy(*a, **k):
            seen.append(real(*a, **k))
            return seen[-1]

        monkeypatch.setattr(syncbn, "sync_batch_norm", spy)
        logits = head(x, det=False)
        monkeypatch.setattr(syncbn, "sync_batch_norm", real)
        y = seen[0]
        saved = [(tuple(t.shape), t.data_ptr()) for t in y.grad_fn.saved_tensors]
        logits.backward(dlogits)
        torch.cuda.synchronize()
        assert head.bn_scale in ready and head.bn_bias in ready
        res[on] = dict(logits=logits.detach(), y=y.detach(), fn=y.grad_fn, saved=saved, rm=head.running_mean.clone(),
                       rv=head.running_var.clone(), dg=head.bn_scale.grad.clone(), db=head.bn_bias.grad.clone(),
                       dk=head.dense.k.grad.clone(), W=head.dense.k.shadow.float().clone())
    on, off = res[True], res[False]
    # the kernel path: bf16 straight from the Function, and nothing of size B x J saved but x
    assert on["y"].dtype == BF16 and off["y"].dtype == F32
    assert type(on["fn"]).__name__.startswith("_SyncBNFused")
    assert [t[0] for t in on["saved"]] == [(B, J), (2, J)] and on["saved"][0][1] == x.data_ptr()
    assert R.bf16_steps(on["y"].cpu(), off["y"].to(BF16).cpu()).max().item() <= 1
    yabs, W = off["y"].abs().double(), on["W"].abs().double()
    tol = 2.0 ** -8 * (yabs @ W.t()) + 2.0 ** -7 * off["logits"].abs().double() + 1e-30
    assert ((on["logits"].double() - off["logits"].double()).abs() <= tol).all()
    xh = (x.double() - x.double().mean(0)) / x.double().std(0, unbiased=False)
    dy = (dlogits.double() @ on["W"].double()).abs()
    for k, scale in (("db", dy.sum(0)), ("dg", (dy * xh.abs()).sum(0)), ("rm", 0.01 * x.double().abs().mean(0)),
                     ("rv", 1.0 + 0.01 * (x.double() ** 2).mean(0))):
        d = (on[k].double() - off[k].double()).abs().cpu()
        print(f"routing {k}: worst difference / tolerance {(d / (4e-5 * scale.cpu())).max().item():.3f}")
        assert (d <= 4e-5 * scale.cpu()).all(), k
    # the Dense weight gradient: dlogits^T y, y differing by a bf16 step
    tol = 2.0 ** -8 * (dlogits.abs().double().t() @ yabs) + 1e-6 * off["dk"].abs().double() + 1e-30
    assert ((on["dk"].double() - off["dk"].double()).abs() <= tol).all()


def test_graph_replay_equals_eager_steps():
    """Forward, backward and running-statistics update captured in one graph on one stream and replayed
    twice: outputs, gradients and running statistics equal two eager steps bit for bit."""
    ext = _ext()
    B, J = 130, 192
    gen = torch.Generator().manual_seed(3)
    x, gamma, beta, dy = (t.cuda() for t in R.inputs(B, J, gen))
    dy = dy.to(BF16)

    def step(rm, rv):
        packed = ext.bn_stats(x)
        y, stats = ext.bn_apply(x, packed, gamma, beta, rm, rv, EPS, MOM, BF16)
        dgamma, dbeta, packed_g = ext.bn_bwd_reduce(dy, x, stats, gamma)
        dx = ext.bn_bwd_dx(dy, x, stats, gamma, packed_g, float(B))
        return y, stats, dgamma, dbeta, dx

    rm_e, rv_e = torch.zeros(J, device="cuda"), torch.ones(J, device="cuda")
    eager = [[t.clone() for t in step(rm_e, rv_e)] + [rm_e.clone(), rv_e.clone()] for _ in range(2)]
    rm_g, rv_g = torch.zeros(J, device="cuda"), torch.ones(J, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            outs = step(rm_g, rv_g)
    torch.cuda.current_stream().wait_stream(s)
    rm_g.zero_()
    rv_g.fill_(1.0)  # the capture itself runs nothing
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert _same(list(outs) + [rm_g, rv_g], eager[k]), k
