"""The fused BatchNorm without a GPU: the argument checks of its five bindings (they run before any
launch, so CPU tensors reach every message), the switch, and the CPU path of ``sync_batch_norm``, which
stays the torch composition bit for bit (tests/bn_ref.py)."""

import pytest
import torch

import bn_ref as R
from jumbo_mae_tpu_amd.models.params import ParamStore, ones_, zeros_
from jumbo_mae_tpu_amd.ops import prims as P
from jumbo_mae_tpu_amd.parallel.syncbn import sync_batch_norm

B, J = 5, 12


def _ext():
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(False)
    if ext is None:
        pytest.skip("extension not built (python -m jumbo_mae_tpu_amd.csrc.build)")
    return ext


def _good():
    g = torch.Generator().manual_seed(0)
    x, gamma, beta, dy = R.inputs(B, J, g)
    return dict(x=x, dy=dy, gamma=gamma, beta=beta, rm=torch.zeros(J), rv=torch.ones(J), packed=torch.zeros(2 * J),
                stats=torch.zeros(2, J), packed_g=torch.zeros(2 * J), out=torch.zeros(B, J))


def _calls(ext):
    """name -> (function of the argument dict, the names of the arguments it takes)"""
    f32 = torch.float32
    return {
        "bn_stats": (lambda a: ext.bn_stats(a["x"]), ["x"]),
        "bn_apply": (lambda a: ext.bn_apply(a["x"], a["packed"], a["gamma"], a["beta"], a["rm"], a["rv"], 1e-5, 0.99,
                                            f32, a["out"]), ["x", "packed", "gamma", "beta", "rm", "rv", "out"]),
        "bn_apply_eval": (lambda a: ext.bn_apply_eval(a["x"], a["rm"], a["rv"], a["gamma"], a["beta"], 1e-5, f32,
                                                      a["out"]), ["x", "rm", "rv", "gamma", "beta", "out"]),
        "bn_bwd_reduce": (lambda a: ext.bn_bwd_reduce(a["dy"], a["x"], a["stats"], a["gamma"], a["rm"], a["rv"]),
                          ["dy", "x", "stats", "gamma", "rm", "rv"]),
        "bn_bwd_dx": (lambda a: ext.bn_bwd_dx(a["dy"], a["x"], a["stats"], a["gamma"], a["packed_g"], float(B),
                                              a["out"]), ["dy", "x", "stats", "gamma", "packed_g", "out"]),
    }


MAT = ("x", "dy", "out")
# the message names its argument by the binding's word for it
WORD = {"rm": ("running_mean", "dgamma"), "rv": ("running_var", "dbeta")}


def _words(k):
    return WORD.get(k, (k,))


@pytest.mark.parametrize("name", ["bn_stats", "bn_apply", "bn_apply_eval", "bn_bwd_reduce", "bn_bwd_dx"])
def test_bindings_reject_bad_arguments_with_their_message(name):
    ext = _ext()
    fn, args = _calls(ext)[name]

    def raises(a, *needles):
        with pytest.raises(RuntimeError) as e:
            fn(a)
        msg = str(e.value)
        assert name + ":" in msg and any(n in msg for n in needles), (name, needles, msg)

    # everything well formed, on the CPU: the device check is the only one left, and it comes last
    raises(_good(), "must be a GPU tensor")
    for k in args:
        # a wrong dtype (fp64 everywhere; bf16 too where only fp32 is taken)
        a = _good()
        a[k] = a[k].double()
        raises(a, *[w + " must be" for w in _words(k)])
        if k in ("x",) or (k == "out" and name == "bn_bwd_dx"):
            a = _good()
            a[k] = a[k].bfloat16()
            raises(a, k + " must be fp32")
        if k in MAT:
            a = _good()
            a[k] = torch.zeros(J, B).t()  # column stride != 1
            raises(a, k + " must have a unit column stride")
            a = _good()
            a[k] = torch.zeros(B, 2 * J)[:, ::2]
            raises(a, k + " must have a unit column stride")
            a = _good()
            a[k] = torch.zeros(1, J).expand(B, J)  # row stride 0
            raises(a, k + " rows must not overlap")
            a = _good()
            a[k] = torch.as_strided(torch.zeros(B * J), (B, J), (J - 1, 1))
            raises(a, k + " rows must not overlap")
            a = _good()
            a[k] = torch.zeros(B, J)[0]  # not 2-D
            raises(a, k + " must be [B, J]")
            if k != "x":  # mismatched J / B against x
                a = _good()
                a[k] = torch.zeros(B, J + 1, dtype=a[k].dtype)
                raises(a, k + " must have the shape of x")
                a = _good()
                a[k] = torch.zeros(B + 1, J, dtype=a[k].dtype)
                raises(a, k + " must have the shape of x")
        else:
            ok = _good()[k]
            longer = torch.zeros(ok.shape[:-1] + (ok.shape[-1] + 1,))
            strided = torch.zeros(ok.shape[:-1] + (2 * ok.shape[-1],))[..., ::2]
            assert strided.shape == ok.shape and not strided.is_contiguous()
            for bad in (ok[..., :-1].contiguous(), longer, strided, ok[None], ok.reshape(-1)[:1]):
                a = _good()
                a[k] = bad  # wrong length (a packed of 2 J - 1, a gamma of another J), strided, wrong rank
                raises(a, *[w + " must be" for w in _words(k)])
    if "x" in args and len(args) > 1:  # x alone changes J: every vector is now of the wrong length
        a = _good()
        a["x"] = torch.zeros(B, J + 4)
        raises(a, "must be", "must have the shape of x")
    if name in ("bn_apply", "bn_apply_eval"):
        for dt in (torch.float16, torch.float64):
            with pytest.raises(RuntimeError, match="out_dtype must be bf16 or fp32"):
                (ext.bn_apply(*[_good()[k] for k in ("x", "packed", "gamma", "beta", "rm", "rv")], 1e-5, 0.99, dt)
                 if name == "bn_apply" else
                 ext.bn_apply_eval(*[_good()[k] for k in ("x", "rm", "rv", "gamma", "beta")], 1e-5, dt))
        a = _good()
        a["out"] = a["out"].bfloat16()  # out against out_dtype
        raises(a, "out must have out_dtype")
    if name == "bn_apply":
        g = _good()
        with pytest.raises(RuntimeError, match="eps > 0"):
            ext.bn_apply(g["x"], g["packed"], g["gamma"], g["beta"], g["rm"], g["rv"], 0.0, 0.99, torch.float32)
    if name == "bn_bwd_reduce":
        g = _good()
        with pytest.raises(RuntimeError, match="dgamma and dbeta come together"):
            ext.bn_bwd_reduce(g["dy"], g["x"], g["stats"], g["gamma"], g["rm"], None)
    if name == "bn_bwd_dx":
        g = _good()
        with pytest.raises(RuntimeError, match="n counts at least the local rows"):
            ext.bn_bwd_dx(g["dy"], g["x"], g["stats"], g["gamma"], g["packed_g"], float(B - 1))


def test_switch_exists_and_is_on():
    assert P._BN_OURS is True


def _handles(gamma, beta):
    store = ParamStore()
    hs = store.handle(store.add(("BatchNorm_0", "scale"), (gamma.numel(),), ones_))
    hb = store.handle(store.add(("BatchNorm_0", "bias"), (gamma.numel(),), zeros_))
    store.finalize("cpu")
    with torch.no_grad():
        hs.master.copy_(gamma)
        hb.master.copy_(beta)
    return store, hs, hb


@pytest.mark.parametrize("ours", [True, False])
@pytest.mark.parametrize("shape", [(1, 7), (2, 12), (65, 33)])
def test_cpu_path_is_the_composition_bit_for_bit(ours, shape, monkeypatch):
    """Outputs, gradients and running statistics of sync_batch_norm on CPU tensors, with the switch on or
    off, against bn_ref.composition in fp32; the inference branch against bn_ref.eval_formula."""
    monkeypatch.setattr(P, "_BN_OURS", ours)
    Bc, Jc = shape
    g = torch.Generator().manual_seed(Bc * 100 + Jc)
    x, gamma, beta, dy = R.inputs(Bc, Jc, g)
    store, hs, hb = _handles(gamma, beta)
    ready = []
    store.hooks.append(lambda h: ready.append(h))
    rm, rv = torch.randn(Jc, generator=g), 0.5 + torch.rand(Jc, generator=g)
    rm0, rv0 = rm.clone(), rv.clone()
    xin = x.clone().requires_grad_(True)
    y = sync_batch_norm(xin, hs, hb, rm, rv, training=True, out_dtype=torch.bfloat16)
    assert y.dtype == torch.float32  # the CPU path has no fused cast
    y.backward(dy)
    y32, mean, var, dgamma, dbeta, dx = R.composition(x, gamma, beta, dy, torch.float32)
    assert torch.equal(y.detach(), y32) and torch.equal(xin.grad, dx)
    assert torch.equal(hs.grad, dgamma) and torch.equal(hb.grad, dbeta)
    assert ready == [hs, hb]
    want_rm, want_rv = rm0.clone(), rv0.clone()
    want_rm.mul_(0.99).add_((1 - 0.99) * mean)
    want_rv.mul_(0.99).add_((1 - 0.99) * var)
    assert torch.equal(rm, want_rm) and torch.equal(rv, want_rv)
    ye = sync_batch_norm(x, hs, hb, rm, rv, training=False, out_dtype=torch.bfloat16)
    assert torch.equal(ye, R.eval_formula(x, gamma, beta, rm, rv, torch.float32))
    assert torch.equal(rm, want_rm) and torch.equal(rv, want_rv)


def test_oracle_helpers():
    v = torch.tensor([1.0, -3.0, 0.0], dtype=torch.float64)
    assert R.ulp32(v).tolist() == [2.0 ** -23, 2.0 ** -22, 2.0 ** -149]
    a = torch.tensor([1.0, -1.0, 0.0]).bfloat16()
    b = torch.tensor([1.0078125, -1.0, -0.0]).bfloat16()
    assert R.bf16_steps(a, b).tolist() == [1, 0, 0]
    r = torch.full((3,), 2.0, dtype=torch.float64)
    assert torch.equal(R.running(r, torch.ones(3)), r * 0.99 + (1 - 0.99) * torch.ones(3, dtype=torch.float64))
