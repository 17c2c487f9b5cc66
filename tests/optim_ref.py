"""fp64 reference of the flat optimizers, hand-built chunk tables and the shared assertions.

Used by tests/test_optim_kernels_gpu.py (the HIP kernels of csrc/optim.hip) and tests/test_optim.py
(the same reference against ``FlatOptimizer._step_torch`` on the CPU, which keeps it honest without a
GPU).  Nothing here calls ``FlatOptimizer``: ``ref_step`` restates the semantics of the optim/flat.py
docstring element by element in float64 over the fp32 inputs the kernels get --

  clip    f = c / gn where gn = sqrt(sum of g^2 over the covered elements) >= c, else 1
  adamw   mu' = b1 mu + (1 - b1) f g;  nu' = b2 nu + (1 - b2) (f g)^2
          u = (mu' / bc1) / (sqrt(nu' / bc2) + eps) + wd decay p;  p' = p - lr llrd u
  lamb    the same u;  p' = p - lr llrd tr u,  tr = |p| / |u| per segment where the trust flag is set
  lars    t' = -lr tr f g + momentum t,  tr = coef |p| / |f g| per segment;  p' = p + llrd t'
  sgd     t' = f g + momentum t;  p' = p - lr llrd t'
  tr = 1 where |p| = 0 or |u| = 0 or the flag is off; norms are sums over the covered elements of the
  segment (a ZeRO-1 table covers part of a segment); segments with trainable = 0 keep p and t.

``hyper = [lr, 1 - b1^t, 1 - b2^t, clip, b1, b2, eps, wd]`` and ``meta[seg] = [decay, llrd, trust,
trainable]`` are the kernels' own fp32 tensors, read here as float64.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import torch

F64 = torch.float64
U = 2.0 ** -24  # fp32 unit roundoff (round to nearest even)


def f32(x: float) -> float:
    """``x`` rounded to fp32, as a Python float (what a ``(float)`` cast in the bindings passes on)."""
    return float(torch.tensor(x, dtype=torch.float32))


# ------------------------------------------------------------------ chunk tables
@dataclass
class Table:
    name: str
    rows: torch.Tensor    # int32 [nchunks, 3] = (start, length, segment), sorted by segment
    n: int                # length of the flat buffers
    nseg: int
    seg_of: torch.Tensor  # int64 [n]: segment of every covered element, -1 elsewhere

    @property
    def covered(self) -> torch.Tensor:
        return self.seg_of >= 0

    def runs(self) -> list[tuple[int, int]]:
        """(segment, chunks) of every run of rows, in table order."""
        out: list[list[int]] = []
        for s in self.rows[:, 2].tolist():
            if out and out[-1][0] == s:
                out[-1][1] += 1
            else:
                out.append([s, 1])
        return [tuple(r) for r in out]


def table_from_rows(name: str, rows, n: int, nseg: int) -> Table:
    """Checked table: every row inside [0, n), no overlap, starts multiples of 4 (AdamW's 16-byte
    accesses), rows sorted by segment (chunk_sums_kernel's runs)."""
    rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1, 3)
    seg_of = torch.full((n,), -1, dtype=torch.int64)
    prev = -1
    for st, ln, sg in rows.tolist():
        assert 0 <= st and ln > 0 and st + ln <= n, (st, ln, n)
        assert st % 4 == 0, st
        assert prev <= sg < nseg, (prev, sg, nseg)
        assert bool((seg_of[st:st + ln] == -1).all()), f"rows overlap at {st}"
        seg_of[st:st + ln] = sg
        prev = sg
    return Table(name, rows.to(torch.int32), n, nseg, seg_of)


def build_table(name: str, numels: list[int], chunk: int, gaps: list[int], tail: int = 12) -> Table:
    """Segments of ``numels`` elements cut into rows of ``chunk``; ``gaps[k]`` unused elements after
    segment k, then up to the next multiple of 4; ``tail`` unused elements at the end of the buffer."""
    rows, pos = [], 0
    for k, ne in enumerate(numels):
        for st in range(0, ne, chunk):
            rows.append((pos + st, min(chunk, ne - st), k))
        pos = -(-(pos + ne + gaps[k]) // 4) * 4
    return table_from_rows(name, rows, pos + tail, len(numels))


RUNS64_CHUNKS = [(1, 64), (257, 64), (600, 64), (1, 7), (256, 64), (1, 1), (3, 64)]  # (chunks, chunk length)


def runs64() -> Table:
    """Chunk length 64: runs of 1, 257, 600 chunks, one chunk of 7 elements, exactly 256 chunks, one
    chunk of 1 element and a last run of 3 chunks that ends the table; gaps after segments 0, 2, 3,
    4 and 5."""
    return build_table("runs64", [c * ln for c, ln in RUNS64_CHUNKS], 64, [4, 0, 8, 0, 12, 0, 0])


def partial(full: Table | None = None) -> Table:
    """``runs64`` without every third row (rows 1, 4, 7, ...): the ZeRO-1 shape, rows covering part of
    a segment.  Every segment keeps at least one row and the last row stays the table's last."""
    full = full or runs64()
    keep = [i for i in range(full.rows.shape[0]) if i % 3 != 1]
    return table_from_rows("partial", full.rows[keep], full.n, full.nseg)


def prod(chunk: int) -> Table:
    """Production chunk length: one segment of 3 chunk + 5 elements (three full rows and one of 5)
    and one of 64."""
    return build_table("prod", [3 * chunk + 5, 64], chunk, [4, 0])


@dataclass
class Spec:
    """Per-segment flags and data scales of a table's test inputs."""
    decay: list[float]
    llrd: list[float]
    trust: list[float]    # LAMB's flag (kernels only); LARS sets 1 everywhere
    scale: list[float]    # p and g of segment k are N(0, 1) * scale[k]: a different power of ten each
    zero_p: tuple = ()    # segments with p == 0 everywhere (|p| = 0: ratio 1)
    zero_g: tuple = ()    # segments with g == 0 everywhere (|u| = 0 with decay 0: ratio 1)


def spec_for(tab: Table) -> Spec:
    if tab.nseg == 2:
        return Spec(decay=[1, 0], llrd=[1.0, 0.75], trust=[1, 0], scale=[1.0, 1e-2])
    assert tab.nseg == 7
    return Spec(decay=[0, 1, 1, 0, 0, 1, 0], llrd=[0.75 ** k for k in range(7)], trust=[0, 1, 1, 1, 1, 1, 0],
                scale=[1e-2, 1.0, 1e-1, 1e-3, 1e-4, 1e-5, 1e-6], zero_p=(5,), zero_g=(3,))


# hyper[0] by kind for the tables above.  The smallest relative update over the trainable segments is
# lr * llrd (LAMB with the flag; SGD, times a clip factor of 0.5), lr * coef * llrd (LARS, coef 1e-3)
# and lr * llrd / rms(p) (AdamW, rms(p) <= 1), with llrd >= 0.75^6 = 0.178: all >= 1e-2, which
# assert_updates asserts on the reference
LR = {"adamw": 0.05, "lamb": 0.1, "lars": 64.0, "sgd": 0.25}


def make_meta(kind: str, spec: Spec, frozen: tuple = ()) -> torch.Tensor:
    nseg = len(spec.decay)
    meta = torch.zeros(nseg, 4, dtype=torch.float32)
    for k in range(nseg):
        trust = 1.0 if kind == "lars" else float(spec.trust[k]) if kind == "lamb" else 0.0
        decay = float(spec.decay[k]) if kind in ("adamw", "lamb") else 0.0
        meta[k] = torch.tensor([decay, spec.llrd[k], trust, 0.0 if k in frozen else 1.0])
    return meta


def like_signed(g: torch.Tensor, sign_of: torch.Tensor | None) -> torch.Tensor:
    """``g`` with the sign of ``sign_of`` element by element (kept where ``sign_of`` is 0 or None)."""
    if sign_of is None:
        return g
    return torch.where(sign_of != 0, g.abs() * torch.sign(sign_of), g)


def make_inputs(tab: Table, spec: Spec, seed: int, sign_of: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """fp32 (p, g): N(0, 1) times the segment's scale (uncovered elements: scale 1, so that a write
    there shows), zeroed where the spec says so.

    ``sign_of``: the previous step's gradient; g takes its signs.  The terms added into mu and into
    the momentum trace then have one sign per element and never cancel.  The element bound of
    ``assert_updates`` is relative to the update, so it presupposes that: with independent signs about
    one element in 10^4 cancels to below 1e-2 of its terms, where the 1e-6 of error that the fp32
    norms may carry into one of the terms (1e-5 is allowed) already exceeds 1e-4 of the update."""
    gen = torch.Generator().manual_seed(seed)
    sc = torch.tensor(spec.scale + [1.0], dtype=torch.float32)[tab.seg_of]  # -1 -> the trailing 1.0
    p = torch.randn(tab.n, generator=gen) * sc
    g = like_signed(torch.randn(tab.n, generator=gen) * sc, sign_of)
    for k in spec.zero_p:
        p[tab.seg_of == k] = 0.0
    for k in spec.zero_g:
        g[tab.seg_of == k] = 0.0
    return p, g


def exact_norm_grad(tab: Table, spec: Spec, seed: int, sign_of: torch.Tensor | None = None) -> tuple[torch.Tensor, float]:
    """(g, c): an fp32 gradient whose sum of squares over the covered elements is c^2 EXACTLY in fp32,
    in any summation order.  Values are +-0.5, +-1, +-1.5, +-2: squares are multiples of 0.25 and the
    total stays below 2^24 * 0.25, so every partial sum is exact; a few elements are then lowered
    (1 -> 0.5 takes 3 quarter units off, 1.5 -> 1 takes 5) until the total is (m / 2)^2."""
    gen = torch.Generator().manual_seed(seed)
    h = torch.randint(1, 5, (tab.n,), generator=gen)                    # |g| in half units
    sign = torch.randint(0, 2, (tab.n,), generator=gen) * 2 - 1
    cov = tab.covered.clone()
    for k in spec.zero_g:
        h[tab.seg_of == k] = 0
    q = int((h[cov] ** 2).sum())
    assert q < 2 ** 24
    m = math.isqrt(q)
    if q - m * m in (1, 2, 4, 7):  # not of the form 3a + 5b
        m -= 1
    d = q - m * m
    b = {0: 0, 1: 2, 2: 1}[d % 3]
    a = (d - 5 * b) // 3
    ones = torch.nonzero(cov & (h == 2)).flatten()[:a]
    threes = torch.nonzero(cov & (h == 3)).flatten()[:b]
    assert ones.numel() == a and threes.numel() == b
    h[ones] = 1
    h[threes] = 2
    assert int((h[cov] ** 2).sum()) == m * m
    return like_signed((h * sign).to(torch.float32) * 0.5, sign_of), m / 2.0


# ------------------------------------------------------------------ fp64 reference
def _d(t) -> torch.Tensor:
    return t.detach().cpu().to(F64)


def clip_factor(hyper, g, tab: Table, clip_on: bool, gnorm_sq=None) -> tuple[float, float | None]:
    """(f, sum of g^2): clip by global norm over the covered elements, clipping at gn >= c.
    ``gnorm_sq`` given: the fp32 value a kernel was handed instead of the float64 sum."""
    if not clip_on:
        return 1.0, None
    c = float(_d(hyper)[3])
    gs = float((_d(g)[tab.covered] ** 2).sum()) if gnorm_sq is None else float(gnorm_sq)
    gn = math.sqrt(gs)
    return (c / gn if gn >= c else 1.0), gs


def ref_u(tab: Table, meta, hyper, p, mu_new, nu_new):
    """(u, magnitude): the LAMB phase-1 update from given new moments, and |adam term| + |decay term|."""
    _, bc1, bc2, _, _, _, eps, wd = _d(hyper).tolist()
    sid = tab.seg_of.clamp(min=0)
    a = (_d(mu_new) / bc1) / (torch.sqrt(_d(nu_new) / bc2) + eps)
    w = wd * _d(meta)[sid, 0] * _d(p)
    return a + w, a.abs() + w.abs()


def ref_step(kind: str, tab: Table, meta, hyper, p, g, mu=None, nu=None, trace=None, *, clip_on: bool,
             gnorm_sq=None, norms=None, momentum: float = 0.9, trust_coef: float = 1e-3) -> dict:
    """One optimizer step in float64 from fp32 inputs.  ``gnorm_sq`` / ``norms`` ([nseg, 2] sums of
    squares): use these fp32 kernel inputs instead of the float64 sums (the stage-by-stage state
    checks); by default everything is computed here.

    Returns float64 tensors: ``p`` and, by kind, ``mu`` ``nu`` ``u`` ``trace`` ``norms``, plus
    ``*_mag``, the sum of the magnitudes of the terms added into each state element (the scale of its
    fp32 rounding error).  Elements outside the table keep their values.  Frozen segments keep ``p``
    and ``trace`` (what the kernels do); their moments are updated as on the torch path and are
    compared nowhere."""
    lr, bc1, bc2, _, b1, b2, eps, wd = _d(hyper).tolist()
    cov = tab.covered
    sid = tab.seg_of.clamp(min=0)
    m = _d(meta)
    llrd = m[sid, 1]
    trust_on = m[:, 2] != 0
    live = cov & (m[sid, 3] != 0)
    P, G = _d(p), _d(g)
    f, gs = clip_factor(hyper, g, tab, clip_on, gnorm_sq)
    gg = G * f
    out = {"f": f, "gnorm_sq": gs}

    def seg_sums(x):
        return torch.zeros(tab.nseg, dtype=F64).index_add_(0, tab.seg_of[cov], x[cov])

    def ratio(n2, coef):
        pn, un = n2[:, 0].sqrt(), n2[:, 1].sqrt()
        ok = trust_on & (pn != 0) & (un != 0)
        return torch.where(ok, coef * pn / torch.where(un != 0, un, torch.ones_like(un)), torch.ones_like(pn))

    if kind in ("adamw", "lamb"):
        MU, NU = _d(mu), _d(nu)
        m1, m2 = b1 * MU, (1 - b1) * gg
        v1, v2 = b2 * NU, (1 - b2) * gg * gg
        out["mu"], out["mu_mag"] = torch.where(cov, m1 + m2, MU), m1.abs() + m2.abs()
        out["nu"], out["nu_mag"] = torch.where(cov, v1 + v2, NU), v1.abs() + v2.abs()
        u, out["u_mag"] = ref_u(tab, meta, hyper, p, out["mu"], out["nu"])
        out["u"] = u
        if kind == "lamb":
            n2 = torch.stack([seg_sums(P * P), seg_sums(u * u)], 1)
            out["norms"] = n2
            u = u * ratio(n2 if norms is None else _d(norms), 1.0)[sid]
        upd = -lr * llrd * u
    elif kind == "lars":
        T = _d(trace)
        n2 = torch.stack([seg_sums(P * P), seg_sums(gg * gg)], 1)
        out["norms"] = n2
        t1, t2 = -lr * ratio(n2 if norms is None else _d(norms), trust_coef)[sid] * gg, momentum * T
        out["trace"], out["trace_mag"] = torch.where(live, t1 + t2, T), t1.abs() + t2.abs()
        upd = llrd * (t1 + t2)
    else:
        assert kind == "sgd", kind
        T = _d(trace)
        t1, t2 = gg, momentum * T
        out["trace"], out["trace_mag"] = torch.where(live, t1 + t2, T), t1.abs() + t2.abs()
        upd = -lr * llrd * (t1 + t2)
    out["p"] = torch.where(live, P + upd, P)
    return out


# ------------------------------------------------------------------ shared assertions
UPDATE_FLOOR = 1e-2   # every trainable segment moves by at least this fraction of its parameter norm
UPDATE_REL = 1e-4     # per-segment relative L2 error allowed on the update


def assert_updates(tab: Table, meta, g, p_old, p_new, ref_p, tag: str = "") -> None:
    """The update p_new - p_old (float64 differences of the fp32 buffers) against the reference's,
    segment by segment over the covered elements.

    The learning rate of every case is chosen so that the REFERENCE update of each trainable segment
    with a non-zero gradient is at least UPDATE_FLOOR = 1e-2 of the segment's parameter norm (asserted
    here): a comparison of p itself would pass with no update at all.  Then

      * ||update - ref|| < 1e-4 ||ref|| per segment: rounding p_new to fp32 contributes at most
        2^-24 / 1e-2 = 6e-6, a wrong factor or a skipped chunk 1e-2 or more;
      * |update - ref| <= 2^-23 |p_new| + 1e-4 |ref| for every element: one fp32 ulp of the stored
        parameter plus the same relative slack, so that a few missed elements cannot hide in a norm.
    """
    P0, P1, R = _d(p_old), _d(p_new), _d(ref_p)
    m = _d(meta)
    G = _d(g)
    upd, ref = P1 - P0, R - P0
    err = (upd - ref).abs()
    bound = 2.0 ** -23 * P1.abs() + UPDATE_REL * ref.abs()
    for k in range(tab.nseg):
        sel = tab.seg_of == k
        if not bool(sel.any()):
            continue
        rn, pn, en = float(ref[sel].norm()), float(P0[sel].norm()), float((upd - ref)[sel].norm())
        if m[k, 3] != 0 and bool((G[sel] != 0).any()):
            assert rn >= UPDATE_FLOOR * pn, f"{tag} seg {k}: reference update {rn:.3e} < 1e-2 * |p| = {pn:.3e}"
        if rn == 0.0:
            assert en == 0.0, f"{tag} seg {k}: update {float(upd[sel].norm()):.3e}, reference has none"
        else:
            assert en < UPDATE_REL * rn, f"{tag} seg {k}: update error {en / rn:.3e} (relative L2)"
        bad = sel & (err > bound)
        if bool(bad.any()):
            i = int(torch.nonzero(bad)[0])
            raise AssertionError(f"{tag} seg {k}: {int(bad.sum())} element(s) off, first at {i}: update "
                                 f"{float(upd[i]):.9e} ref {float(ref[i]):.9e} bound {float(bound[i]):.3e}")
