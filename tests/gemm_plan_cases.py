"""Cases and recorder of tests/test_gemm_plan.py and tests/test_gemm_plan_gpu.py: the launch plan of the NT
GEMM kernels (csrc/gemm_plan.h) must give the output tiles and tail splits recorded in
tests/golden/gemm_nt_plans.json.

Every case ``(M, N, K, lda)`` is planned for every epilogue of ``EPIS`` under every ``gemm_test_force``
setting of ``FORCES``; the golden file keeps ``[tiles, tail S, tail tiles]`` per combination, in
``combos()`` order, and the CU count of the device they were planned for.

The golden file is written from the tree of the commit BEFORE a change to the launch code:
    python tests/gemm_plan_cases.py --tree DIR --write FILE
(``DIR``, the root of a built tree, is put first on sys.path).  Recording launches no kernels.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / "golden" / "gemm_nt_plans.json"
EPIS = (0, 1, 2, 3, 4, 6, 7)
FORCES = ((0, 0), (1, 0), (2, 0), (2, 256), (2, 224), (2, 192), (2, 160))

# (M, N, K, lda)
CASES = [
    # the shapes that tests/test_kernels_gpu.py names
    (25088, 4096, 1024, 1024), (26624, 3072, 1024, 1024), (512, 12288, 3072, 3072), (512, 3072, 12288, 12288),
    (128, 9216, 2304, 2304),
    # the jumbo MLP at a 2048-row micro-batch
    (2048, 12288, 3072, 3072), (2048, 3072, 12288, 12288),
    # tail split: the case of tests/test_gemm_exact_gpu.py (53 tail tiles of 256 CUs), exactly a quarter wave (64)
    # and just over it (65)
    (11008, 7936, 1024, 1024), (6656, 8192, 1024, 1024), (12544, 4352, 1024, 1024),
    # ViT-B FF2 (N = 768, K = 3072): MAE encoder rows of a 512 batch, full sequences of a 256 batch
    (25600, 768, 3072, 3072), (50432, 768, 3072, 3072),
    # tail limits: K / 512 < 2, K / 512 = 3, more than 8 splits possible
    (11008, 7936, 512, 512), (11008, 7936, 1536, 1536), (8192, 4128, 8192, 8192),
    # the edge shapes of tests/test_gemm_exact_gpu.py cases(), one per family (strided and contiguous rows)
    (129, 200, 192, 256), (383, 392, 192, 256), (513, 264, 256, 320), (449, 264, 384, 448), (385, 264, 128, 192),
    (321, 264, 256, 320), (159, 264, 128, 128), (2400, 520, 128, 128), (257, 264, 320, 384), (513, 264, 64, 64),
    # N % 8 != 0 (no narrow tiles, no tail split), K % 128 == 64 (no 4-phase loop)
    (257, 260, 192, 256), (513, 260, 128, 192), (11008, 7932, 1024, 1024), (2048, 3072, 1088, 1088),
    (25088, 4096, 1088, 1088),
    # M around NARROW_MAX_M
    (4095, 768, 768, 768), (4096, 768, 768, 768), (4095, 3072, 768, 768), (4096, 3072, 768, 768),
    # M lda 2 bytes just below and at 2^31 - 2^20 (short tiles end), and at 2^32 (no launch)
    (1048063, 512, 1024, 1024), (1048064, 512, 1024, 1024), (2097152, 256, 128, 1024),
]


def case_id(case) -> str:
    M, N, K, lda = case
    return f"{M}x{N}x{K}-lda{lda}"


def combos():
    """(epilogue, (force path, force rows)) in the order of a case's golden rows."""
    return [(e, f) for e in EPIS for f in FORCES]


def record(ext) -> dict:
    import torch

    cases = {}
    try:
        for case in CASES:
            M, N, K, lda = case
            rows = []
            for epi, (path, frows) in combos():
                ext.gemm_test_force(path, frows)
                S, r = ext.gemm_nt_tail_plan(M, N, K, epi, lda)
                rows.append([ext.gemm_nt_tiles(M, N, K, epi, lda), S, r])
            cases[case_id(case)] = rows
    finally:
        ext.gemm_test_force(0)
    return {"cus": torch.cuda.get_device_properties(0).multi_processor_count, "epis": list(EPIS),
            "forces": [list(f) for f in FORCES], "cases": cases}


# fields of a plan, in the order tests/gemm_plan_driver.cpp prints them (= the keys of ext.gemm_nt_plan)
FIELDS = ("status", "family", "tile_rows", "tile_cols", "row_tiles", "col_tiles", "tiles", "grid", "tail_S",
          "tail_r", "tail_floats", "colpart", "colpart_rows", "colpart_zero")
NARROW, P4, NT64 = 0, 1, 2
PARTIAL_SPLITS = (1, 4)  # EPI_PARTIAL is planned at each of these split counts, the others at 1


def check_plan(plan: dict, want, case, epi: int, splits: int):
    """``plan`` (FIELDS -> value) against the golden ``[tiles, S, r]`` of the parent and against itself."""
    M, N, K, lda = case
    tiles, S, r = want
    what = (case, epi, splits, plan)
    assert plan["tiles"] == tiles and (plan["tail_S"], plan["tail_r"]) == (S, r), (what, want)
    assert plan["row_tiles"] == -(-M // plan["tile_rows"]) and plan["col_tiles"] == -(-N // plan["tile_cols"]), what
    assert plan["tiles"] == plan["row_tiles"] * plan["col_tiles"], what
    assert plan["colpart_rows"] == plan["row_tiles"] + 8 * r, what
    assert plan["tail_floats"] == S * r * 256 * 256, what
    assert plan["grid"] == (tiles * splits if epi == 3 else tiles - r), what
    assert bool(plan["colpart"]) == (epi in (2, 7)) and bool(plan["colpart_zero"]) == (r > 0), what
    assert (S >= 2 and 0 < r <= tiles) or (S, r) == (0, 0), what
    if plan["family"] == NARROW:
        assert (plan["tile_rows"], plan["tile_cols"]) == (128, 192) and r == 0, what
    else:
        assert plan["family"] in (P4, NT64) and plan["tile_cols"] == 256, what
        assert plan["tile_rows"] in ((256, 224, 192, 160) if plan["family"] == P4 else (256,)), what
        assert r == 0 or (plan["family"], plan["tile_rows"]) == (P4, 256), what
    assert plan["family"] != P4 or K % 128 == 0, what
    if M * lda * 2 >= 2 ** 32:
        assert plan["status"] == -2, what
    elif epi == 3 and K // 64 < splits:
        assert plan["status"] == -4, what
    elif epi in (2, 7) and N % 8:
        assert plan["status"] == -3, what
    else:
        assert plan["status"] == 0, what


def load_golden() -> dict:
    g = json.loads(GOLDEN.read_text())
    assert g["epis"] == list(EPIS) and g["forces"] == [list(f) for f in FORCES], "golden file of another case list"
    assert sorted(g["cases"]) == sorted(case_id(c) for c in CASES), "golden file of another case list"
    return g


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--tree", required=True, help="root of the built tree whose plans are recorded")
    ap.add_argument("--write", required=True, help="JSON file to write")
    a = ap.parse_args(argv)
    sys.path.insert(0, str(Path(a.tree).resolve()))
    from jumbo_mae_tpu_amd.ops import _ext
    ext = _ext.load(True)
    print("extension:", ext.__file__)
    res = record(ext)
    Path(a.write).parent.mkdir(parents=True, exist_ok=True)
    body = ",\n".join(f'  "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in res["cases"].items())
    head = {k: v for k, v in res.items() if k != "cases"}
    Path(a.write).write_text(json.dumps(head)[:-1] + ', "cases": {\n' + body + "\n}}\n")
    print(f"wrote {len(res['cases'])} cases x {len(combos())} combinations ({res['cus']} CUs) to {a.write}")


if __name__ == "__main__":
    sys.exit(main())
