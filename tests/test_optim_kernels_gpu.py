"""The optimizer kernels of csrc/optim.hip against a float64 reference, on hand-built chunk tables.

The raw bindings (``opt_sumsq``, ``opt_adamw``, ``opt_lamb_phase1``, ``opt_lars_norms``,
``opt_apply_trust``, ``opt_sgd``) run on flat buffers of ~70 k floats with the tables of
tests/optim_ref.py: ``runs64`` (runs of 1 / 257 / 600 / 1 / 256 / 1 / 3 chunks, so that
``chunk_sums_kernel``'s 256-strided walk wraps, starts at rows > 0 and ends at ``nchunks``; chunks of 7
and 1 elements for AdamW's scalar tail), ``prod`` (``flat.CHUNK`` rows) and ``partial`` (``runs64``
without every third row: norms over the covered part of a segment).  Each segment's p and g carry a
different power of ten, so a norm that leaks into a neighbouring run is off by orders of magnitude.
The reference (``optim_ref.ref_step``) is plain float64 over the same fp32 inputs; it never calls
``FlatOptimizer``.

What is asserted, and where each tolerance comes from (u = 2^-24, the fp32 unit roundoff; the build
has no fast-math flag, hipcc's fp32 division and sqrt are correctly rounded, and a contracted FMA
only removes a rounding, so every operation contributes at most u relative to its result):

updates   ``optim_ref.assert_updates``: p_new - p_old per segment, relative L2 < 1e-4, and per element
          within 2^-23 |p_new| + 1e-4 |ref|; ``hyper[0]`` per kind (LR below) makes every trainable
          segment's reference update >= 1e-2 of its parameter norm, which is asserted.
state     element by element |err| <= k u (sum of the magnitudes of the added terms), against float64
          from the fp32 values the kernel itself was given (its gnorm_sq, its norms, and for u its
          own stored mu / nu), with k the count of roundings on the worst term plus the final add:
            mu     b1 mu + (1 - b1) (g f):  f = c / sqrt(gs) 2, g f 1, 1 - b1 1, product 1, add 1   k = 6
            nu     b2 nu + ((1 - b2) (g f)) (g f):  g f 3 twice, 1 - b2 1, two products 2, add 1    k = 10
            u      (mu / bc1) / (sqrt(nu / bc2) + eps) + wd p:  division 1, denominator 0.5 + 1 + 1,
                   division 1, add 1 (the decay term: product 1, add 1)                             k = 6
            trace  LARS -lr tr (f g) + mom t:  tr = coef sqrt(pn2) / sqrt(un2) 4, lr tr 1, f g 3,
                   product 1, add 1 (the momentum term: product 1, add 1)                           k = 10
            trace  SGD f g + mom t:  f 2, product 1, add 1                                          k = 4
          plus 2^-126 where a result may be subnormal.  The moments of frozen segments are NOT
          compared: AdamW's kernel skips them while the torch path updates them.
norms     relative 1e-5 against float64: at most 32 serial fp32 adds per thread at CHUNK = 8192, then
          the wave, block and chunk trees: under 64 u = 4e-6.  Two more calls must return the same
          bits (fixed summation order), and the outputs start from non-zero values (``+=``, which
          ZeRO-1 relies on).
shadow    bit-equal to ``p_new.to(bfloat16)`` (round to nearest even) on covered elements; a run
          without shadow gives the same p bits.
uncovered every element outside the table's rows keeps its bits in p, mu, nu, trace, u and shadow
          (the gaps, the tail, the rows removed in ``partial``); g keeps its bits everywhere.
frozen    two segments with meta[3] = 0 (one single-chunk, one multi-chunk) keep the bits of p, shadow
          and trace in opt_adamw, opt_sgd and both opt_apply_trust modes.
clip      off (gnorm_sq = -1), norm below / above / exactly equal to clip (a gradient whose fp32 sum
          of squares is a perfect square: factor 1 whether the comparison is < or <=).  AdamW and LAMB
          are invariant to the factor in p; their moments show it.
trust     segments with p == 0, g == 0 and trust flag 0 must get ratio 1; LAMB has the flag off on
          two segments, LARS on everywhere.  opt_apply_trust mode 0 is called with a coefficient of
          0.25 that it has to ignore (the host passes 1).
steps     two consecutive steps (non-zero mu / nu / trace carry over): bias corrections for t = 1 and
          for t = 10000, where 1 - b2^t is within 5e-5 of 1.  The second gradient has fresh
          magnitudes and the first one's signs, so the terms added into mu and the trace do not
          cancel: the element bound on the update is relative to the update and presupposes that
          (``optim_ref.make_inputs``).
"""

import pytest
import torch

import optim_ref as R
from optim_ref import U

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -77.0  # exact in bf16
TINY = 2.0 ** -126
B1, B2, EPS, WD = 0.9, 0.999, 1e-8, 0.1
MOMENTUM, TRUST_COEF = 0.9, 1e-3
LR = R.LR  # hyper[0] by kind: every trainable segment's update is >= 1e-2 of its parameter norm
K_MU, K_NU, K_U, K_TRACE = 6, 10, 6, {"lars": 10, "sgd": 4}
KINDS = ("adamw", "lamb", "lars", "sgd")
CLIPS = ("off", "below", "above", "equal")


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


@pytest.fixture(scope="module")
def tables():
    from jumbo_mae_tpu_amd.optim import flat
    full = R.runs64()
    return {"runs64": full, "partial": R.partial(full), "prod": R.prod(flat.CHUNK)}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits(a, b, mask=None) -> bool:
    a, b = bits(a), bits(b)
    return bool(torch.equal(a, b) if mask is None else torch.equal(a[mask], b[mask]))


def make_hyper(kind: str, t: int, clip: float) -> torch.Tensor:
    wd = WD if kind in ("adamw", "lamb") else 0.0
    return torch.tensor([LR[kind], 1.0 - B1 ** t, 1.0 - B2 ** t, clip, B1, B2, EPS, wd], dtype=torch.float32)


def hip_step(ext, kind, tab, meta, hyper, st, g, clip_on, with_shadow=True):
    """One step through the raw bindings on device copies of ``st`` (dict of fp32 CPU tensors p, mu,
    nu, trace); returns CPU tensors: the new state, shadow, u, norms and the gnorm_sq handed on."""
    dv = lambda t: t.clone().to(DEV)
    rows, meta_d, hyper_d, g_d = dv(tab.rows), dv(meta), dv(hyper), dv(g)
    p, mu, nu, trace = (dv(st[k]) for k in ("p", "mu", "nu", "trace"))
    shadow = torch.full((tab.n,), SENTINEL, dtype=torch.bfloat16, device=DEV) if with_shadow else None
    u = torch.full((tab.n,), SENTINEL, dtype=torch.float32, device=DEV)
    norms = torch.zeros(tab.nseg, 2, dtype=torch.float32, device=DEV)
    gs = torch.zeros(1, dtype=torch.float32, device=DEV)
    if clip_on:
        ext.opt_sumsq(g_d, rows, gs)
    else:
        gs.fill_(-1.0)
    if kind == "adamw":
        ext.opt_adamw(p, g_d, mu, nu, shadow, rows, meta_d, hyper_d, gs)
    elif kind == "lamb":
        ext.opt_lamb_phase1(p, g_d, mu, nu, u, rows, meta_d, hyper_d, gs, norms)
        ext.opt_apply_trust(p, u, None, shadow, rows, meta_d, hyper_d, norms, gs, 0, 0.0, 0.25)
    elif kind == "lars":
        ext.opt_lars_norms(p, g_d, rows, hyper_d, gs, norms)
        ext.opt_apply_trust(p, g_d, trace, shadow, rows, meta_d, hyper_d, norms, gs, 1, MOMENTUM, TRUST_COEF)
    else:
        ext.opt_sgd(p, g_d, trace, shadow, rows, meta_d, hyper_d, gs, MOMENTUM)
    torch.cuda.synchronize()
    out = {"p": p, "mu": mu, "nu": nu, "trace": trace, "u": u, "norms": norms, "gs": gs, "g": g_d}
    if with_shadow:
        out["shadow"] = shadow
    return {k: v.cpu() for k, v in out.items()}


def assert_state(name, got, ref, mag, k, mask, tag):
    err = (got.double() - ref).abs()[mask]
    bound = (k * U * mag + TINY)[mask]
    worst = float((err / bound).max()) if err.numel() else 0.0
    print(f"OPTCHK {tag} {name} max err/bound {worst:.3f}")
    assert worst <= 1.0, f"{tag} {name}: {int((err > bound).sum())} element(s) beyond {k} u * magnitude, worst {worst:.2f}x"


def assert_norms(got, ref, tag):
    got, ref = got.double().flatten(), ref.flatten()
    rel = ((got - ref).abs() / ref.abs().clamp(min=1e-300)).where(ref != 0, got.abs())
    print(f"OPTCHK {tag} norms max rel {float(rel.max()):.3e}")
    assert float(rel.max()) <= 1e-5, f"{tag}: norms off by {rel.reshape(-1, 2).tolist()}"


def run_case(ext, kind, tab, clip, frozen):
    spec = R.spec_for(tab)
    meta = R.make_meta(kind, spec, frozen)
    cov = tab.covered
    sid = tab.seg_of.clamp(min=0)
    live = cov & (meta[sid, 3] != 0)
    dead = cov & ~live
    p0, _ = R.make_inputs(tab, spec, 10)
    zeros = torch.zeros(tab.n)
    st = {"p": p0, "mu": zeros.clone(), "nu": zeros.clone(), "trace": zeros.clone()}
    used = {"adamw": ("mu", "nu"), "lamb": ("mu", "nu"), "lars": ("trace",), "sgd": ("trace",)}[kind]
    g = None
    for step, t in enumerate((1, 10000)):
        tag = f"{kind}/{tab.name}/{clip}/step{step}"
        if clip == "equal":  # the second gradient takes the signs of the first (optim_ref.make_inputs)
            g, c = R.exact_norm_grad(tab, spec, 20 + step, g)
        else:
            _, g = R.make_inputs(tab, spec, 20 + step, g)
            gn = float(g.double()[cov].norm())
            c = R.f32({"off": 0.0, "below": 2.0 * gn, "above": 0.5 * gn}[clip])
        clip_on = clip != "off"
        hyper = make_hyper(kind, t, c)
        out = hip_step(ext, kind, tab, meta, hyper, st, g, clip_on)
        bare = hip_step(ext, kind, tab, meta, hyper, st, g, clip_on, with_shadow=False)
        # the whole step in float64 (updates), and stage by stage from the kernels' fp32 norms (state)
        ref = R.ref_step(kind, tab, meta, hyper, st["p"], g, st["mu"], st["nu"], st["trace"], clip_on=clip_on,
                         momentum=R.f32(MOMENTUM), trust_coef=R.f32(TRUST_COEF))
        gs_in = float(out["gs"]) if clip_on else None
        stage = R.ref_step(kind, tab, meta, hyper, st["p"], g, st["mu"], st["nu"], st["trace"], clip_on=clip_on,
                           gnorm_sq=gs_in, norms=out["norms"] if kind in ("lamb", "lars") else None,
                           momentum=R.f32(MOMENTUM), trust_coef=R.f32(TRUST_COEF))
        # ---- clip norm
        if clip_on:
            assert_norms(out["gs"], torch.tensor([ref["gnorm_sq"]], dtype=R.F64), tag + " gnorm_sq")
            if clip == "equal":
                assert float(out["gs"]) == c * c, f"{tag}: sum of squares {float(out['gs'])} is not exactly {c * c}"
                assert ref["f"] == 1.0 and stage["f"] == 1.0
            else:
                assert (ref["f"] == 1.0) == (clip == "below"), (tag, ref["f"])
        else:
            assert float(out["gs"]) == -1.0
        # ---- updates
        R.assert_updates(tab, meta, g, st["p"], out["p"], ref["p"], tag)
        # ---- state
        if kind in ("adamw", "lamb"):
            assert_state("mu", out["mu"], stage["mu"], stage["mu_mag"], K_MU, live, tag)
            assert_state("nu", out["nu"], stage["nu"], stage["nu_mag"], K_NU, live, tag)
        if kind == "lamb":
            u_ref, u_mag = R.ref_u(tab, meta, hyper, st["p"], out["mu"], out["nu"])
            assert_state("u", out["u"], u_ref, u_mag, K_U, cov, tag)
        if kind in ("lars", "sgd"):
            assert_state("trace", out["trace"], stage["trace"], stage["trace_mag"], K_TRACE[kind], live, tag)
        if kind in ("lamb", "lars"):
            assert_norms(out["norms"], ref["norms"], tag)
        # ---- shadow
        assert same_bits(out["shadow"], out["p"].to(torch.bfloat16), live), f"{tag}: shadow is not the RNE cast of p"
        assert same_bits(bare["p"], out["p"]), f"{tag}: p differs between the runs with and without shadow"
        for k in used:
            assert same_bits(bare[k], out[k]), f"{tag}: {k} differs between the runs with and without shadow"
        # ---- uncovered elements, frozen segments, the gradient
        for k in ("p", "mu", "nu", "trace"):
            assert same_bits(out[k], st[k], ~cov), f"{tag}: {k} written outside the table"
        for k in ("u", "shadow"):
            assert same_bits(out[k], torch.full_like(out[k], SENTINEL), ~cov), f"{tag}: {k} written outside the table"
        assert same_bits(out["g"], g), f"{tag}: g written"
        if bool(dead.any()):
            assert same_bits(out["p"], st["p"], dead), f"{tag}: p of a frozen segment written"
            assert same_bits(out["trace"], st["trace"], dead), f"{tag}: trace of a frozen segment written"
            assert same_bits(out["shadow"], torch.full_like(out["shadow"], SENTINEL), dead), \
                f"{tag}: shadow of a frozen segment written"
        st = {k: out[k] for k in ("p", "mu", "nu", "trace")}


@pytest.mark.parametrize("clip", CLIPS)
@pytest.mark.parametrize("table", ["runs64", "prod", "partial"])
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_match_fp64(ext, tables, kind, table, clip):
    """Two steps of one optimizer through the raw bindings, every segment trainable: updates, state,
    norms, shadow and untouched elements as laid out in the module docstring (k = 6 / 10 / 6 for mu /
    nu / u, 10 / 4 for the LARS / SGD trace; update floor 1e-2 asserted on the reference)."""
    run_case(ext, kind, tables[table], clip, ())


@pytest.mark.parametrize("table", ["runs64", "partial"])
@pytest.mark.parametrize("kind", KINDS)
def test_frozen_segments_keep_their_bits(ext, tables, kind, table):
    """Segments 0 (one chunk) and 2 (600 chunks) with meta[3] = 0, clip above the norm: p, shadow and
    trace of both keep their bits in opt_adamw, opt_sgd and opt_apply_trust modes 0 and 1, and every
    other segment still matches float64 (same k and bounds).  Nothing is asserted about the moments
    of the frozen segments: AdamW's kernel skips them, LAMB's phase 1 and the torch path update them."""
    run_case(ext, kind, tables[table], "above", (0, 2))


@pytest.mark.parametrize("table", ["runs64", "prod", "partial"])
def test_norm_entry_points_accumulate_in_fixed_order(ext, tables, table):
    """opt_sumsq, opt_lamb_phase1 and opt_lars_norms add into outputs that already hold non-zero
    values: old value + float64 sum within 1e-5 (under 64 u = 4e-6 from the fp32 accumulation, one
    more u for the ``+=``), and two more calls from the same inputs return the same bits."""
    tab = tables[table]
    spec = R.spec_for(tab)
    p, g = R.make_inputs(tab, spec, 30)
    gn = float(g.double()[tab.covered].norm())
    hyper = make_hyper("lamb", 1, R.f32(0.5 * gn))
    meta, meta_s = R.make_meta("lamb", spec), R.make_meta("lars", spec)
    mu0, nu0 = torch.randn(tab.n, generator=torch.Generator().manual_seed(31)) * g.abs(), g * g
    trace0 = torch.zeros(tab.n)
    gs64 = (g.double()[tab.covered] ** 2).sum().reshape(1)
    gs = gs64.to(torch.float32)
    # the norms from the fp32 gnorm_sq the kernels are handed (the clip factor enters LARS' |f g|)
    ref_l = R.ref_step("lamb", tab, meta, hyper, p, g, mu0, nu0, None, clip_on=True, gnorm_sq=float(gs))
    ref_s = R.ref_step("lars", tab, meta_s, hyper, p, g, None, None, trace0, clip_on=True, gnorm_sq=float(gs))
    # preloads of the order of the sums themselves (3 where the sum is 0), so neither hides the other
    pre = lambda ref: torch.where(ref != 0, 0.37 * ref, torch.full_like(ref, 3.0)).to(torch.float32)
    dv = lambda t: t.clone().to(DEV)
    rows, g_d, p_d, hyper_d, meta_d, gs_d = dv(tab.rows), dv(g), dv(p), dv(hyper), dv(meta), dv(gs)

    def sumsq():
        o = dv(pre(gs64))
        ext.opt_sumsq(g_d, rows, o)
        return o.cpu()

    def lamb():
        o, mu, nu, u = dv(pre(ref_l["norms"])), dv(mu0), dv(nu0), torch.empty(tab.n, device=DEV)
        ext.opt_lamb_phase1(p_d, g_d, mu, nu, u, rows, meta_d, hyper_d, gs_d, o)
        return o.cpu()

    def lars():
        o = dv(pre(ref_s["norms"]))
        ext.opt_lars_norms(p_d, g_d, rows, hyper_d, gs_d, o)
        return o.cpu()

    for name, fn, ref in (("sumsq", sumsq, gs64), ("lamb_phase1", lamb, ref_l["norms"]),
                          ("lars_norms", lars, ref_s["norms"])):
        a, b, c = fn(), fn(), fn()
        assert_norms(a, pre(ref).double() + ref, f"{name}/{table} accumulate")
        assert same_bits(a, b) and same_bits(a, c), f"{name}/{table}: three calls, different bits"


# ------------------------------------------------------------------ the real host path
HOST_LR = {"adamw": 0.05, "lamb": 0.05, "lars": 20.0, "sgd": 0.25}


@pytest.mark.parametrize("chunk", [64, None])
@pytest.mark.parametrize("clip", [0.0, 100.0])
@pytest.mark.parametrize("kind", KINDS)
def test_flat_optimizer_hip_matches_fp64(ext, monkeypatch, kind, clip, chunk):
    """``FlatOptimizer`` on the GPU (chunk table, meta and hyper built by the host) for the tiny
    pretrain model, two steps at a constant LR, against the float64 reference with
    ``assert_updates``'s bounds.  ``flat.CHUNK = 64`` turns the 147 k-element leaf into a run of more
    than 2000 chunks; ``None`` keeps the production value.  LR per kind: the smallest relative update
    is lr llrd (AdamW / LAMB on the unit LayerNorm scales), lr 1e-3 llrd (LARS) and lr llrd f with
    f = 100 / |g| ~ 0.2 (SGD, clipped), llrd >= 0.75^2: all >= 1e-2, asserted on the reference.  The
    clip of 100 is below the gradient norm (~500), so it is active."""
    from jumbo_mae_tpu_amd.config import DecoderConfig, ViTConfig
    from jumbo_mae_tpu_amd.models.mae import PretrainModel
    from jumbo_mae_tpu_amd.optim import flat

    if chunk is not None:
        monkeypatch.setattr(flat, "CHUNK", chunk)
    vc = ViTConfig(layers=2, dim=64, heads=4, labels=0, image_size=32, patch_size=8, posemb="sincos2d")
    dc = DecoderConfig(dec_layers=1, dec_dim=32, dec_heads=2, image_size=32, patch_size=8)
    m = PretrainModel(vc, dc).to(DEV, torch.bfloat16, seed=0)
    s = m.store
    lr = HOST_LR[kind]
    opt = flat.FlatOptimizer(s, kind, lambda count: lr, b1=B1, b2=0.95, eps=EPS, weight_decay=0.05, lr_decay=0.75,
                             num_layers=2, clip_grad=clip)
    tab = R.table_from_rows("host", opt.chunks.cpu(), s.total, opt.nseg)
    if chunk is not None:
        assert max(n for _, n in tab.runs()) > 2000
    assert int(tab.covered.sum()) == sum(sg.numel for sg in s.segments)
    meta = opt.meta.cpu()
    wd = 0.05 if kind in ("adamw", "lamb") else 0.0
    st = {k: torch.zeros(s.total) for k in ("mu", "nu", "trace")}
    gen = torch.Generator().manual_seed(1)
    g = None
    for step in range(2):
        t = step + 1
        g = R.like_signed(torch.randn(s.total, generator=gen), g)  # see optim_ref.make_inputs
        p_old = s.master.cpu()
        s.grad.copy_(g.to(DEV))
        opt.step()
        torch.cuda.synchronize()
        hyper = torch.tensor([lr, 1.0 - B1 ** t, 1.0 - 0.95 ** t, clip, B1, 0.95, EPS, wd], dtype=torch.float32)
        assert torch.equal(opt.hyper.cpu(), hyper)
        ref = R.ref_step(kind, tab, meta, hyper, p_old, g, st["mu"], st["nu"], st["trace"], clip_on=clip > 0,
                         momentum=R.f32(0.9), trust_coef=R.f32(1e-3))
        if clip > 0:
            assert ref["f"] < 1.0
        tag = f"host/{kind}/clip{clip}/chunk{chunk}/step{step}"
        R.assert_updates(tab, meta, g, p_old, s.master.cpu(), ref["p"], tag)
        assert same_bits(s.shadow, s.master.to(torch.bfloat16), tab.covered), f"{tag}: shadow is not the RNE cast"
        assert same_bits(s.master, p_old, ~tab.covered), f"{tag}: padding written"
        st = {k: (getattr(opt, k).cpu() if getattr(opt, k) is not None else st[k]) for k in st}
