"""The TN weight-gradient kernels of csrc/gemm_tn.hip, element by element, on exactly summable operands.

G [N, K] (+)= dy[M, N]^T x[M, K] with dy small integers and x (and G's initial contents) small integers
times 2**-s: every partial sum over any part of the M rows is an fp32 number, so the result does not
depend on the M split, the slice reduction or the order of the row blocks, and ``torch.equal`` holds
against float64.  dy and x are views into NaN-filled buffers (tests/gemm_ref.py ``poisoned_view``): a
row >= M read without its mask, or the padding of a row, shows as NaN.  Exactness: M a_max b_max + |G0|
< 2**24 units (``gemm_ref.check_exact`` with K = M).
"""

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

G0_MAX = 64  # |G0| in units of 2**-s


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


def plan(shapes, M):
    """Mirror of jm_gemm_tn_plan (csrc/gemm_tn.hip): the number of M splits of a launch."""
    NK = sum(n * k for n, k in shapes)
    tiles = sum((n // 256) * (k // 256) for n, k in shapes)
    cdiv = lambda a, b: -(-a // b)
    steps = cdiv(M, 32)
    best, best_S = 1e30, 1
    for S in range(1, 129):
        sps = cdiv(cdiv(steps, S), 4) * 4  # whole 128-row units
        s_eff = cdiv(steps, sps)
        waves = (tiles * s_eff + 255) // 256
        est = float(waves) * (sps + 12) + (s_eff * NK * 8.0 / 5.0e12 * 1e6 if s_eff > 1 else 0.0)
        if est < best:
            best, best_S = est, s_eff
    return best_S


def operands(M, N, K, seed, s, strided=True):
    """dy [M, N] integers in [-2, 2], x [M, K] integers in [-2, 2] times 2**-s (both bf16)."""
    R.check_exact(M, 2, 2, extra=G0_MAX)
    gen = torch.Generator().manual_seed(seed)
    dy = torch.randint(-2, 3, (M, N), generator=gen).to(torch.bfloat16).cuda()
    x = (torch.randint(-2, 3, (M, K), generator=gen).double() * 2.0 ** -s).to(torch.bfloat16).cuda()
    return (R.poisoned_view(dy), R.poisoned_view(x)) if strided else (dy, x)


def grid_g(N, K, seed, s):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randint(-G0_MAX, G0_MAX + 1, (N, K), generator=gen).double() * 2.0 ** -s).float().cuda()


def seed_of(*key):
    return R.seed_of("gemm_tn_exact", *key)


def prod64(dy, x):
    return dy.double().t() @ x.double()


@pytest.mark.parametrize("strided", [True, False], ids=["strided", "contig"])
@pytest.mark.parametrize("M", [200, 480, 128, 8192 + 32])
def test_gemm_tn_exact_plain(ext, M, strided):
    """The 4-phase kernel: ragged M against its 128-row unit, exactly one unit, and M split into slices
    + reduce; accumulate onto grid values and store over 1e4."""
    N = K = 256
    s = R.grid_scale(M, 2, 2)
    want_S = plan([(N, K)], M)
    # one unit: the kernel itself accumulates into / stores G; every other M: fp32 slices + the reduce
    assert want_S == {200: 2, 480: 4, 128: 1, 8224: 65}[M]
    for store in (False, True):
        dy, x = operands(M, N, K, seed_of("plain", M, strided, store), s, strided)
        g0 = grid_g(N, K, seed_of("g0", M, strided), s)
        g = torch.full((N, K), 1e4, device="cuda") if store else g0.clone()
        assert ext.gemm_tn_wgrad(dy, x, g, store) == want_S
        ref = prod64(dy, x) + (0.0 if store else g0.double())
        assert torch.equal(g.double(), ref), store


@pytest.mark.parametrize("shapes,stores", [([(256, 512), (512, 256)], [True, False]),
                                           ([(256, 512), (512, 256), (256, 256), (768, 256)],
                                            [False, True, True, False])])
def test_gemm_tn_exact_group(ext, shapes, stores):
    """Grouped launch: 2 and 4 problems of different (N, K) over the same ragged M, mixed store flags."""
    M = 1000
    s = R.grid_scale(M, 2, 2)
    ops = [operands(M, n, k, seed_of("group", len(shapes), i), s) for i, (n, k) in enumerate(shapes)]
    g0s = [grid_g(n, k, seed_of("group g0", len(shapes), i), s) for i, (n, k) in enumerate(shapes)]
    gs = [torch.full_like(g0, 1e4) if st else g0.clone() for g0, st in zip(g0s, stores)]
    S = ext.gemm_tn_wgrad_group([d for d, _ in ops], [x for _, x in ops], gs, stores)
    assert S == plan(shapes, M)
    for (dy, x), g0, g, st in zip(ops, g0s, gs, stores):
        assert torch.equal(g.double(), prod64(dy, x) + (0.0 if st else g0.double())), (g.shape, st)


@pytest.mark.parametrize("nb,rows", [(3, 128), (5, 96)], ids=["seg4phase", "seg32step"])
@pytest.mark.parametrize("store", [False, True], ids=["acc", "store"])
def test_gemm_tn_exact_segmented(ext, nb, rows, store):
    """Row blocks read in place: 3 blocks of 128 rows (the 4-phase kernel's segmented form) and 5 of 96
    (no multiple of 64: the 32-row-step kernel).  Every block is its own NaN-surrounded buffer."""
    N = K = 256
    M = nb * rows
    s = R.grid_scale(M, 2, 2)
    blocks = [operands(rows, N, K, seed_of("seg", nb, rows, store, i), s) for i in range(nb)]
    dys, xs = [d for d, _ in blocks], [x for _, x in blocks]
    g0 = grid_g(N, K, seed_of("seg g0", nb, rows, store), s)
    g = torch.full((N, K), 1e4, device="cuda") if store else g0.clone()
    assert ext.gemm_tn_wgrad_seg(dys, xs, g, store) == plan([(N, K)], M)
    ref = prod64(torch.cat(dys), torch.cat(xs)) + (0.0 if store else g0.double())
    assert torch.equal(g.double(), ref)


@pytest.mark.parametrize("nb,rows", [(3, 128), (5, 64)], ids=["128rows", "64rows"])
def test_gemm_tn_exact_segmented_group(ext, nb, rows):
    """Segmented and grouped: 2 problems of different (N, K), one stored and one accumulated (blocks of a
    multiple of 64 rows: the grouped launch has the 4-phase kernel only)."""
    shapes, stores = [(256, 512), (512, 256)], [True, False]
    M = nb * rows
    s = R.grid_scale(M, 2, 2)
    blocks = [[operands(rows, n, k, seed_of("sg", nb, rows, p, i), s) for i in range(nb)]
              for p, (n, k) in enumerate(shapes)]
    dys, xs = [[d for d, _ in b] for b in blocks], [[x for _, x in b] for b in blocks]
    g0s = [grid_g(n, k, seed_of("sg g0", nb, rows, p), s) for p, (n, k) in enumerate(shapes)]
    gs = [torch.full_like(g0, 1e4) if st else g0.clone() for g0, st in zip(g0s, stores)]
    assert ext.gemm_tn_wgrad_seg_group(dys, xs, gs, stores) == plan(shapes, M)
    for d, x, g0, g, st in zip(dys, xs, g0s, gs, stores):
        assert torch.equal(g.double(), prod64(torch.cat(d), torch.cat(x)) + (0.0 if st else g0.double())), st
