// The launch plan of the NT GEMM kernels (gemm.hip): which kernel family and tile shape a launch takes,
// its grid, its tail split and the sizes of the buffers it writes -- decided once per launch by
// gemm_nt_plan, obeyed by jm_gemm_nt and read by bindings.cpp to size the tail workspace and the
// column-sum buffer.  Plain host C++: nothing from HIP or torch, no globals, no device
// (tests/gemm_plan_driver.cpp compiles it alone).
#pragma once
#include <initializer_list>

// NT GEMM epilogues (template parameter of the kernels, the epi argument of the plan).
// EPI_STORE: out = acc (+bias); EPI_GELU: out = acc (+bias), out2 = gelu(out);
// EPI_DGELU: out = bf16(acc) * gelu'(aux) -- the data gradient through the FF GELU -- with the
// following Dense's bias gradient (column sums of out) as per-tile partials.
// EPI_PARTIAL: split-K -- each (tile, split) workgroup stores its fp32 partial tile; the sum (+bias,
// bf16) is taken by jm_splitk_reduce_bf16.  For small-M, long-K GEMMs (the jumbo MLP: 512 rows,
// K = 12288) whose 24 output tiles would otherwise occupy 24 of 256 CUs.
// EPI_GELU_ONLY: out = gelu(bf16(acc + bias)) alone -- inference (no backward needs the
// pre-activation), half the epilogue bytes of EPI_GELU.
// EPI_TAIL: split-K partial tile of a tail-split launch, stored compact in ep.tail (see GemmEpi).
// EPI_GELU_D: dq = gelu'(h) as 8-bit codes (common.h gd_code), out2 = gelu(h) for h = bf16(acc + bias):
// the FF1 forward saves the GELU derivative for the backward instead of h (one shared exp here, no
// transcendental in the backward epilogue), in 1 byte per element instead of 2.
// EPI_DMUL: out = bf16(acc) * gelu'(h) decoded from dqa, + column partials as EPI_DGELU.
enum { EPI_STORE = 0, EPI_GELU = 1, EPI_DGELU = 2, EPI_PARTIAL = 3, EPI_GELU_ONLY = 4, EPI_TAIL = 5, EPI_GELU_D = 6,
       EPI_DMUL = 7 };

// kernel families
enum { GEMM_NARROW = 0,  // 128 x 192 tiles, 64-deep ring (gemm_narrow_kernel)
       GEMM_P4 = 1,      // 256 / 224 / 192 / 160 x 256 tiles, 4-phase 128-deep loop (gemm_p4_kernel)
       GEMM_NT64 = 2 };  // 256 x 256 tiles, 64-deep loop, nontemporal epilogue stores (gemm_nt64_kernel)

// tile sizes of the kernels (gemm.hip BM / BN / NBM / NBN, which static_asserts that they agree)
constexpr int GEMM_PLAN_BM = 256, GEMM_PLAN_BN = 256, GEMM_PLAN_NBM = 128, GEMM_PLAN_NBN = 192;
// column-sum rows that the tail finish kernel writes per tail tile (one per 32-row band)
constexpr int GEMM_PLAN_TAIL_BANDS = 8;

// the epilogues whose launch may split its tail (they have a tail_finish_kernel)
constexpr bool gemm_tail_epi(int epi) {
  return epi == EPI_STORE || epi == EPI_GELU || epi == EPI_DGELU || epi == EPI_GELU_ONLY;
}

struct GemmPlan {
  int status;  // 0, or jm_gemm_nt's result for a launch that cannot run: -1 shape, -2 operand of 4 GiB or
               // more, -3 epilogue (unknown, or EPI_DGELU / EPI_DMUL at N % 8 != 0), -4 split count
  int M, N, K, epi, splits;  // the launch the plan was made for
  long lda;
  int family;                // GEMM_NARROW / GEMM_P4 / GEMM_NT64
  int tile_rows, tile_cols;  // output tile
  int row_tiles, col_tiles, tiles;
  int grid;  // workgroups of the main launch: tiles x splits (EPI_PARTIAL), tiles - tail_r with a tail split
  // tail split: the last, partly filled wave of 256 x 256 output tiles (tail_r of them) runs split-K tail_S
  // ways into a compact fp32 workspace and a finish kernel applies the epilogue.  tail_S 0: none
  int tail_S, tail_r;
  long tail_floats;  // floats of that workspace, [tail_S][tail_r][256][256]
  // column sums of EPI_DGELU / EPI_DMUL (GemmEpi::colpart): one row per row tile, then the finish kernel's
  // 8 rows per tail tile.  With a tail split the buffer must start zeroed: the tail tiles' entries of the
  // per-row-tile rows are never written
  bool colpart;  // the launch writes them; a caller that passes no buffer clears this
  int colpart_rows;
  bool colpart_zero;
};

// Relative cost per tile row of the short-row 4-phase tiles vs 256 rows (the same B panel feeds
// fewer MFMAs; measured per full wave, profiles/r3_gemm_tile_rows.txt)
// (160 rows: 1.20 -- ViT-B / finetune N = 768 GEMMs 5-6 % faster than 192 rows, the decoder's N = 512
// ones 2 % slower than 224: profiles/r5_gemm_tile160.txt)
inline float gemm_rows_cost(int tr) { return tr == 256 ? 1.f : (tr == 224 ? 1.05f : (tr == 192 ? 1.10f : 1.20f)); }

// Cost per output element of the 128 x 192 narrow tile relative to the 4-phase 256-row tile: its
// smaller tile re-reads operands 1.5-1.7x as often per FLOP (MFMA busy 35 vs 43-57 %, r4_gemm_pmc)
constexpr float GEMM_NARROW_COST = 1.45f;

constexpr int GEMM_NARROW_MAX_M = 4096;  // M below this: 128 x 192 tiles are a candidate

// ncu: the device's compute units; force_path / force_rows: jm_gemm_test_force (numerics tests only;
// 0 = by shape).  Every field is filled whatever the status.
inline GemmPlan gemm_nt_plan(int M, int N, int K, int epi, long lda, int splits, int ncu, int force_path,
                             int force_rows) {
  constexpr int BM = GEMM_PLAN_BM, BN = GEMM_PLAN_BN, NBM = GEMM_PLAN_NBM, NBN = GEMM_PLAN_NBN;
  GemmPlan p{};
  p.M = M, p.N = N, p.K = K, p.epi = epi, p.splits = splits, p.lda = lda;
  if (ncu < 1) ncu = 1;
  const auto cdiv = [](long a, long b) { return (a + b - 1) / b; };
  const bool splitk = epi == EPI_PARTIAL || epi == EPI_TAIL;
  const bool colsum = epi == EPI_DGELU || epi == EPI_DMUL;
  const bool known = epi == EPI_STORE || epi == EPI_GELU || epi == EPI_GELU_ONLY || epi == EPI_GELU_D ||
                     epi == EPI_PARTIAL || colsum;
  if (K % 64 || N % 4 || M <= 0 || N <= 0) p.status = -1;
  else if ((long)M * lda * 2 >= (1L << 32)) p.status = -2;  // (B's rows: jm_gemm_nt, which is given ldb)
  else if (epi == EPI_PARTIAL && (splits < 1 || K / 64 < splits)) p.status = -4;
  else if (!known || (colsum && N % 8)) p.status = -3;

  // K in 128-deep units -> the 4-phase loop, else the 64-deep one
  const bool deep = force_path != 1 && K % 128 == 0;
  const int nN = (int)cdiv(N, BN);
  const long t256 = cdiv(M, BM) * nN;

  // M < GEMM_NARROW_MAX_M: the narrow tiles unless a 4-phase launch fills the chip's waves better --
  // waves x tile outputs x per-output cost.  The jumbo MLP at a 2048-row micro-batch: N = 12288
  // runs 1.9 waves of 224-row tiles (16-20 % faster than 4 waves of narrow tiles), N = 3072 one
  // full wave of narrow tiles (a 224-row launch would leave half the chip idle); at 512 rows every
  // jumbo GEMM stays narrow (profiles/r4z_jumbo_routing.txt).  Split-K (EPI_PARTIAL) keeps the
  // narrow tiles: the jumbo MLP's K = 12288 GEMMs run 4 splits of 128 x 192 tiles instead of 10 of
  // 256 x 256 -- the GEMM alone is ~4 us slower (r3e_summary_vitl_b512_fused_reductions.txt) but the
  // fp32 partials shrink 2.5x (profiles/r3_narrow_splitk.txt: ViT-L step -0.41 ms in-process).
  bool narrow = force_path == 0 && M < GEMM_NARROW_MAX_M && N % 8 == 0;
  if (narrow && !splitk && deep) {
    const long tn = cdiv(M, NBM) * cdiv(N, NBN);
    const float c_narrow = (float)cdiv(tn, ncu) * NBM * NBN * GEMM_NARROW_COST;
    for (int tr : {256, 224, 192}) {
      const long t = cdiv(M, tr) * nN;
      if ((float)cdiv(t, ncu) * tr * BN * gemm_rows_cost(tr) < c_narrow) narrow = false;
    }
  }

  // Tail split: the last wave of output tiles (tiles % CUs of them) fills only part of the chip; when
  // it is at most a quarter wave, those tiles run split-K S ways (compact fp32 partials) and a finish
  // kernel applies the epilogue.
  // ViT-B FF2 fwd 127 -> 109 us (profiles/r2_gemm_tail_p4.txt).
  int S = 0, r = 0;
  if (force_path == 0 && gemm_tail_epi(epi) && N % 8 == 0 && K % 128 == 0 && !narrow && t256 >= ncu) {
    r = (int)(t256 % ncu);
    // (half a wave of tail tiles split 2 ways lost: ViT-L Wo 201 -> 224 us, step +5 ms)
    if (r > ncu / 4) r = 0;
    if (r) S = ncu / r;
    // every split keeps >= 8 64-deep K steps (r1: splits of 1-2 steps lost to the partial round trip,
    // profiles/r1_gemm_tail_split.txt)
    if (S > K / 512) S = K / 512;
    if (S > 8) S = 8;
    if (S < 2) S = 0, r = 0;
  }

  // Tile height of a 4-phase launch: the candidate whose launch spans the fewest tile rows per CU,
  // waves x rows x rows_cost (a last wave that fills part of the chip costs a full wave; 256-row
  // launches may split a tail of at most a quarter wave instead, counted as 0.8 wave: the split
  // tail and its finish kernel lost to 224 / 192-row tiles on every measured shape).  Split-K,
  // tail-split and 64-deep launches and operands of >= 2 GB (the short tiles' unused a1 rows load
  // from offset 2^31, which must be out of range) keep 256.
  int rows = BM;
  if (!narrow && deep && !splitk && (long)M * lda * 2 < (1L << 31) - (1L << 20)) {
    if (force_rows) {
      rows = force_rows;
    } else {
      float best_c = S ? (t256 / ncu + 0.8f) * BM : (float)cdiv(t256, ncu) * BM;
      for (int tr : {224, 192, 160}) {
        const float c = (float)cdiv(cdiv(M, tr) * nN, ncu) * tr * gemm_rows_cost(tr);
        if (c < best_c) best_c = c, rows = tr;
      }
    }
  }
  if (rows != BM) S = 0, r = 0;  // short-row tiles fill the last wave instead

  // narrow tiles for M < 4096; K in 128-deep units (split-K: per split) -> p4, else the 64-deep kernel
  p.family = narrow ? GEMM_NARROW : (deep && (epi != EPI_PARTIAL || K / 128 >= splits) ? GEMM_P4 : GEMM_NT64);
  p.tile_rows = narrow ? NBM : rows;
  p.tile_cols = narrow ? NBN : BN;
  p.row_tiles = (int)cdiv(M, p.tile_rows);
  p.col_tiles = (int)cdiv(N, p.tile_cols);
  p.tiles = p.row_tiles * p.col_tiles;
  p.grid = epi == EPI_PARTIAL ? p.tiles * splits : p.tiles - r;
  p.tail_S = S, p.tail_r = r;
  p.tail_floats = (long)S * r * BM * BN;
  p.colpart = colsum;
  p.colpart_rows = p.row_tiles + GEMM_PLAN_TAIL_BANDS * r;
  p.colpart_zero = r > 0;
  return p;
}
