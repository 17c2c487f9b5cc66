"""The NT GEMM kernels of csrc/gemm.hip, element by element, on exactly summable operands.

tests/gemm_ref.py draws operands whose products and partial sums are all fp32 numbers, so the fp32 MFMA
accumulators are exact whatever the summation order, split or pipeline, and every stored element is a pure
function of the inputs:

  EPI_STORE, h of EPI_GELU, split-K, gemm_nt_f32   torch.equal with the float64 result cast to the output type
  GELU outputs (EPI_GELU / GELU_ONLY / GELU_D)     per element within (2^-8 + 2^-12) |gelu64(h_bf)| + 1e-30
  EPI_GELU_D codes                                 gemm_ref.gd_check against dgelu64(h_bf)
  EPI_DGELU / EPI_DMUL, pre-activation +-16        torch.equal(out, where(pre > 0, RNE_bf16(acc), 0)) and
                                                   torch.equal(dbias, dbias0 + column sums of out)
  EPI_DGELU / EPI_DMUL, random pre-activation      per element within (2^-8 + 2^-12) |ref| + 2e-6 |RNE_bf16(acc)|,
                                                   dbias within the fp32 summation bound of the kernel's own out

A and B are views into NaN-filled buffers (a consumed row >= M, column >= K or row padding shows as a NaN
in the output), every launch has its own seed (stale allocator contents cannot pass for the result), and
every case first asserts through gemm_nt_tiles / gemm_nt_tail_plan that it reaches the kernel family it
is named after.  Shapes are the smallest that exercise each edge: one row or eight columns in the last
tile, one K-tile, exactly the ring depth, a wrapping ring, an odd K-tile count, N % 8 != 0 (the register
epilogue), 10 row tiles x 3 column tiles for the tile order (a full group of 8 and one of 2; 30
workgroups over 8 XCDs).
"""

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

EPI = {"store": 0, "gelu": 1, "dgelu": 2, "partial": 3, "gelu_only": 4, "gelu_d": 6, "dmul": 7}
# family -> gemm_test_force(path, rows)
FAMS = {"narrow": (0, 0), "p4r256": (2, 256), "p4r224": (2, 224), "p4r192": (2, 192), "p4r160": (2, 160),
        "order": (2, 256), "nt64": (1, 0), "nt64shape": (0, 0)}
FWD = ["store", "gelu", "gelu_only", "gelu_d"]
BWD_SAT = ["dgelu_sat", "dmul_sat"]
BWD_RAND = ["dgelu_rand", "dmul_rand"]
NO_LDS = ["store", "gelu", "gelu_only"]  # what dispatches at N % 8 != 0


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


@pytest.fixture(autouse=True)
def _reset_gemm_variant(request):
    yield
    if "ext" in request.fixturenames:
        request.getfixturevalue("ext").gemm_test_force(0)


def cdiv(a, b):
    return -(-a // b)


def enter(ext, fam, M, N, K, epi, lda):
    """Force the family's kernel path and assert that this launch reaches it."""
    path, rows = FAMS[fam]
    ext.gemm_test_force(path, rows)
    tiles = ext.gemm_nt_tiles(M, N, K, epi, lda)
    big = cdiv(M, rows or 256) * cdiv(N, 256)
    if fam == "narrow":
        assert N % 8 == 0 and M < 4096
        assert tiles == cdiv(M, 128) * cdiv(N, 192) and tiles != cdiv(M, 256) * cdiv(N, 256), (fam, tiles)
    else:
        assert tiles == big, (fam, tiles, big)
    if fam.startswith("p4") or fam == "order":
        assert K % 128 == 0
    if fam == "nt64shape":  # no narrow tiles at N % 8 != 0, no 4-phase loop at K % 128 == 64
        assert K % 128 == 64 and N % 8 != 0
    assert ext.gemm_nt_tail_plan(M, N, K, epi, lda) == (0, 0)


def cases():
    out = []

    def add(fam, kinds, M, N, K, strided):
        for kind in kinds:
            out.append(pytest.param(fam, kind, M, N, K, strided,
                                    id=f"{fam}-{kind}-{M}x{N}x{K}-{'strided' if strided else 'contig'}"))

    main = FWD + BWD_SAT
    # narrow 128 x 192 tiles, ring of 3 64-deep K-tiles
    for K in (64, 192, 320, 256):
        add("narrow", main, 129, 200, K, True)
    add("narrow", BWD_RAND, 129, 200, 320, True)
    add("narrow", main, 257, 192, 192, False)
    add("narrow", main, 383, 392, 192, True)
    add("narrow", main, 129, 200, 192, False)
    # 4-phase kernels, every tile height
    for rows in (256, 224, 192, 160):
        fam = f"p4r{rows}"
        for K in (128, 256, 384):
            add(fam, main, 2 * rows + 1, 264, K, True)
        add(fam, BWD_RAND, 2 * rows + 1, 264, 384, True)
        add(fam, main, rows - 1, 264, 128, False)
        add(fam, NO_LDS, 2 * rows + 1, 260, 256, True)
        add(fam, NO_LDS, rows - 1, 260, 128, False)
    # tile order / XCD remap
    add("order", main + BWD_RAND, 2400, 520, 128, False)
    # 64-deep main loop: forced, and by shape
    for K in (64, 192, 320):
        add("nt64", main, 257, 264, K, True)
    add("nt64", BWD_RAND, 257, 264, 320, True)
    add("nt64", main, 513, 264, 64, False)
    add("nt64", NO_LDS, 513, 260, 128, True)
    for K in (64, 192, 320):
        add("nt64shape", NO_LDS, 257, 260, K, True)
    add("nt64shape", NO_LDS, 513, 260, 192, False)
    return out


def dev_seed(*key):
    return R.seed_of("gemm_exact", *key)


def run_fwd(ext, fam, kind, M, N, K, strided):
    op = R.exact_operands(M, K, N, dev_seed(fam, kind, M, N, K, strided), strided=strided, device="cuda")
    enter(ext, fam, M, N, K, EPI[kind], op.A.stride(0))
    h_bf = R.rne_bf16(op.h64())
    if kind == "store":
        (out,) = ext.gemm_nt(op.A, op.B, op.bias)
        assert torch.equal(out, h_bf)
    elif kind == "gelu":
        h, g = ext.gemm_nt(op.A, op.B, op.bias, True)
        assert torch.equal(h, h_bf)
        R.assert_gelu(g, h_bf, what=f"GELU {fam}")
    elif kind == "gelu_only":
        (g1,) = ext.gemm_nt(op.A, op.B, op.bias, True, True)
        R.assert_gelu(g1, h_bf, what=f"GELU_ONLY {fam}")
        enter(ext, fam, M, N, K, EPI["gelu"], op.A.stride(0))
        h, g = ext.gemm_nt(op.A, op.B, op.bias, True)  # g1 still alive: g is other memory
        assert torch.equal(h, h_bf) and torch.equal(g1, g)
    else:
        q, g = ext.gemm_nt(op.A, op.B, op.bias, True, False, True)
        R.assert_gelu(g, h_bf, what=f"GELU_D {fam}")
        R.gd_check(q, R.dgelu64(h_bf))


def run_bwd(ext, fam, kind, M, N, K, strided):
    sat, deriv = kind.endswith("_sat"), kind.startswith("dmul")
    seed = dev_seed(fam, kind, M, N, K, strided)
    # saturated: dy in {-1, 0, 1} so that the column sums over M rows stay exact as well
    op = R.exact_operands(M, K, N, seed, a_max=1 if sat else 2, colsum_rows=M if sat else 1, strided=strided,
                          device="cuda")
    enter(ext, fam, M, N, K, EPI["dmul" if deriv else "dgelu"], op.A.stride(0))
    a_bf = R.rne_bf16(op.acc64())
    db0 = op.grid((N,), seed + 1)
    db = db0.clone()
    gen = torch.Generator().manual_seed(seed + 2)
    if sat:
        pre = R.saturated_pre(M, N, seed + 2, device="cuda")
        aux = R.saturated_codes(pre) if deriv else pre
        out = ext.gemm_nt_dgelu(op.A, op.B, aux, db, deriv)
        assert torch.equal(out, torch.where(pre > 0, a_bf, torch.zeros_like(a_bf)))
        ref = db0.double() + out.double().sum(0)
        assert torch.equal(ref.float().double(), ref)
        assert torch.equal(db, ref.float())
        return
    if deriv:
        aux = torch.randint(1, 255, (M, N), generator=gen, dtype=torch.uint8).cuda()
        mul64 = (aux.double() - 34.0) / 195.0
    else:
        aux = (torch.randn(M, N, generator=gen) * 2).bfloat16().cuda()
        mul64 = R.dgelu64(aux)
    out = ext.gemm_nt_dgelu(op.A, op.B, aux, db, deriv)
    R.assert_dmul(out, a_bf, mul64, what=f"{kind} {fam}")
    R.assert_colsum(db, db0, out)


@pytest.mark.parametrize("fam,kind,M,N,K,strided", cases())
def test_gemm_nt_exact(ext, fam, kind, M, N, K, strided):
    (run_fwd if kind in FWD else run_bwd)(ext, fam, kind, M, N, K, strided)


@pytest.mark.parametrize("fam,M,N,K", [("narrow", 129, 200, 320), ("p4r224", 449, 264, 384), ("nt64", 257, 264, 192)])
def test_gemm_nt_exact_gelu_d_dropout(ext, fam, M, N, K):
    """FF hidden dropout inside EPI_GELU_D: dropped positions are exactly 0 / GD_Z, kept positions meet
    the GELU bound times 1 / keep and the code check."""
    from jumbo_mae_tpu_amd.ops import dropout as Dr
    from jumbo_mae_tpu_amd.ops import prims as P

    rate = 0.25
    op = R.exact_operands(M, K, N, dev_seed(fam, "drop", M, N, K), device="cuda")
    enter(ext, fam, M, N, K, EPI["gelu_d"], op.A.stride(0))
    h_bf = R.rne_bf16(op.h64())
    seed = torch.tensor([0x5EED + M], dtype=torch.int64, device="cuda")
    q, g = ext.gemm_nt(op.A, op.B, op.bias, True, False, True, seed, rate)
    keep = Dr.keep_mask(seed.cpu(), M * N, rate).view(M, N).cuda()
    assert 0.6 < float(keep.float().mean()) < 0.9
    assert bool((g[~keep] == 0).all()) and bool((q[~keep] == P.GD_Z).all())
    R.assert_gelu(g[keep], h_bf[keep], scale=1.0 / (1.0 - rate), what=f"GELU_D dropout {fam}")
    dref = R.dgelu64(h_bf)
    R.gd_check(torch.where(keep, q, P.gd_encode(dref)), dref)


SPLITK = [(fam, K, S) for fam in ("narrow", "p4r256", "nt64") for K, S in ((1024, 1), (1024, 3), (1024, 8))]
SPLITK.append(("nt64", 192, 3))


@pytest.mark.parametrize("out_kind", ["bf16_bias", "f32_add"])
@pytest.mark.parametrize("fam,K,S", SPLITK)
def test_gemm_nt_exact_splitk(ext, fam, K, S, out_kind):
    """EPI_PARTIAL on each family + the reduce: bf16 with bias, fp32 with bias and a row-strided fp32
    addend on the same grid (NaN between its rows)."""
    M, N = 300, 264
    op = R.exact_operands(M, K, N, dev_seed(fam, "splitk", K, S, out_kind), strided=False, device="cuda")
    R.check_exact(K, 2, 2, extra=R.BIAS_MAX + 64)
    enter(ext, fam, M, N, K, EPI["partial"], op.A.stride(0))
    h64 = op.h64()
    if out_kind == "bf16_bias":
        out = ext.gemm_nt_splitk(op.A, op.B, op.bias, S)
        assert out.dtype == torch.bfloat16 and torch.equal(out, R.rne_bf16(h64))
    else:
        add = R.poisoned_view(op.grid((M, N), dev_seed("add", fam, K, S)))
        out = ext.gemm_nt_splitk(op.A, op.B, op.bias, S, add)
        assert out.dtype == torch.float32 and torch.equal(out.double(), h64 + add.double())


@pytest.mark.parametrize("fam,K", [("narrow", 1024), ("p4r256", 1024), ("nt64", 1024), ("nt64", 192)])
def test_gemm_nt_exact_f32(ext, fam, K):
    """gemm_nt_f32: one fp32 split, the accumulators as they are."""
    M, N = 300, 264
    op = R.exact_operands(M, K, N, dev_seed(fam, "f32", K), strided=True, device="cuda")
    enter(ext, fam, M, N, K, EPI["partial"], op.A.stride(0))
    out = ext.gemm_nt_f32(op.A, op.B)
    assert out.dtype == torch.float32 and torch.equal(out.double(), op.acc64())


# ------------------------------------------------------------------ tail split
# The smallest shape (by outputs, K = 1024) whose path-0 launch still splits its tail on 256 CUs: 43 x 31 =
# 1333 tiles of 256 x 256 = 5 waves + 53 tiles, S = 2.  Below about five waves the 160-row tiles of
# tile_rows() fill the last wave more cheaply than 0.8 wave of split tail (4352 x 4096 x 1024, 272 tiles,
# runs 160-row tiles and no tail split), so nothing smaller reaches launch_tail / tail_finish_kernel.
TAIL_M, TAIL_N, TAIL_K = 11008, 7936, 1024
TAIL_PLAN, TAIL_TILES = (2, 53), 43 * 31


def tail_first_row(M, N, tail_tiles, group=8):
    """First row of the first row tile that holds a tail tile: tiles are numbered in groups of ``group``
    row tiles sweeping the column tiles (csrc/gemm.hip tile_coords), the tail is the last ``tail_tiles``."""
    nM, nN = cdiv(M, 256), cdiv(N, 256)
    rows = []
    for g in range(nM * nN - tail_tiles, nM * nN):
        first_m = g // (group * nN) * group
        rows.append(first_m + g % (group * nN) % min(nM - first_m, group))
    return min(rows) * 256


@pytest.fixture(scope="module")
def tail_ops():
    """Operands and float64 product of the tail-split shape, computed once and left unchanged; entries in
    {-1, 0, 1} so that the column sums over all M rows stay exact."""
    op = R.exact_operands(TAIL_M, TAIL_K, TAIL_N, dev_seed("tail"), a_max=1, b_max=1, colsum_rows=TAIL_M,
                          strided=False, device="cuda")
    return op, op.acc64()


@pytest.mark.parametrize("kind", ["store", "gelu", "gelu_only", "dgelu"])
def test_gemm_nt_exact_tail_split(ext, tail_ops, kind):
    """The last 53 of 1333 tiles run split-K 2 ways into a workspace and a finish kernel applies the
    epilogue.  Exact outputs equal the float64 result AND the plain 4-phase launch bit for bit.  The GELU
    outputs of both launches meet the GELU bound and are bit-equal too, first in every row tile without a
    tail tile (the same kernel) and then everywhere: the finish kernel evaluates gelu with gelu_tanh_f (exp)
    and the LDS epilogue with gelu_n (exp2 with log2(e) folded in) -- csrc/gemm.hip tail_finish_kernel vs
    epilogue_lds -- two fp32 values that could round to different bf16 neighbours but do not on the values
    of this grid."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus != 256:
        pytest.skip(f"tail-split plan assumes 256 CUs, this device has {cus}: on an MI355X this skip is a failure")
    M, N, K = TAIL_M, TAIL_N, TAIL_K
    op, acc64 = tail_ops
    epi = EPI[kind]
    ext.gemm_test_force(0)
    S, tail_tiles = ext.gemm_nt_tail_plan(M, N, K, epi, op.A.stride(0))
    assert S >= 2 and tail_tiles > 0 and (S, tail_tiles) == TAIL_PLAN
    assert ext.gemm_nt_tiles(M, N, K, epi, op.A.stride(0)) == TAIL_TILES
    main_rows = tail_first_row(M, N, tail_tiles)
    assert main_rows == 40 * 256

    def launch(seed):
        if kind == "dgelu":
            pre = R.saturated_pre(M, N, seed, device="cuda")
            db0 = op.grid((N,), seed + 1)
            db = db0.clone()
            return pre, db0, (ext.gemm_nt_dgelu(op.A, op.B, pre, db), db)
        return None, None, tuple(ext.gemm_nt(op.A, op.B, op.bias, kind != "store", kind == "gelu_only"))

    seed = dev_seed("tail", kind)
    pre, db0, tail = launch(seed)
    ext.gemm_test_force(2, 256)
    assert ext.gemm_nt_tail_plan(M, N, K, epi, op.A.stride(0)) == (0, 0)
    _, _, plain = launch(seed)  # the tail launch's outputs stay alive: these are other memory
    ext.gemm_test_force(0)
    if kind == "dgelu":
        a_bf = R.rne_bf16(acc64)
        want = torch.where(pre > 0, a_bf, torch.zeros_like(a_bf))
        ref = db0.double() + want.double().sum(0)
        assert torch.equal(ref.float().double(), ref)
        for out, db in (tail, plain):
            assert torch.equal(out, want)
            assert torch.equal(db, ref.float())
        return
    h_bf = R.rne_bf16(acc64 + op.bias.double())
    for outs, name in ((tail, "tail split"), (plain, "plain")):
        if kind != "gelu_only":
            assert torch.equal(outs[0], h_bf), name
        if kind != "store":
            R.assert_gelu(outs[-1], h_bf, what=f"{kind} {name}")
    if kind != "store":
        assert torch.equal(tail[-1][:main_rows], plain[-1][:main_rows])
        # h_bf lies on the 2**-s grid, a few hundred distinct values: on every one of them the two forms
        # round to the same bf16, so here the launches agree bit for bit in the tail tiles as well
        assert torch.equal(tail[-1], plain[-1])
