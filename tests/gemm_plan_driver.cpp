// Stand-alone driver of csrc/gemm_plan.h for tests/test_gemm_plan.py (built with the address and
// undefined-behaviour sanitizers): reads "M N K epi lda splits ncu force_path force_rows" lines from
// standard input and prints one line of plan fields per input line, in the order of FIELDS there.
#include <cstdio>

#include "gemm_plan.h"

int main() {
  long M, N, K, epi, lda, splits, ncu, path, rows;
  while (std::scanf("%ld %ld %ld %ld %ld %ld %ld %ld %ld", &M, &N, &K, &epi, &lda, &splits, &ncu, &path, &rows) == 9) {
    const GemmPlan p = gemm_nt_plan((int)M, (int)N, (int)K, (int)epi, lda, (int)splits, (int)ncu, (int)path, (int)rows);
    std::printf("%d %d %d %d %d %d %d %d %d %d %ld %d %d %d\n", p.status, p.family, p.tile_rows, p.tile_cols,
                p.row_tiles, p.col_tiles, p.tiles, p.grid, p.tail_S, p.tail_r, p.tail_floats, (int)p.colpart,
                p.colpart_rows, (int)p.colpart_zero);
  }
  return 0;
}
