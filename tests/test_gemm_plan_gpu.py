"""The launch plan of the NT GEMM kernels as the extension makes it on the device (ext.gemm_nt_plan: csrc/gemm_plan.h
at the device's CU count under gemm_test_force) against tests/golden/gemm_nt_plans.json, which was recorded through
gemm_nt_tiles / gemm_nt_tail_plan before the launch code was gathered into one plan.  No kernel is launched."""

import pytest
import torch

import gemm_plan_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    e = _ext.load(True)
    yield e
    e.gemm_test_force(0)


def test_gemm_plan_matches_golden_on_device(ext):
    g = C.load_golden()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == g["cus"], f"the golden plans are those of {g['cus']} CUs, this device has {cus}"
    for case in C.CASES:
        M, N, K, lda = case
        for (epi, (path, rows)), want in zip(C.combos(), g["cases"][C.case_id(case)], strict=True):
            ext.gemm_test_force(path, rows)
            for splits in (C.PARTIAL_SPLITS if epi == 3 else (1,)):
                plan = ext.gemm_nt_plan(M, N, K, epi, lda, splits)
                assert tuple(plan) == C.FIELDS
                C.check_plan(plan, want, case, epi, splits)
            # the two views of the plan that tests and tools read
            assert ext.gemm_nt_tiles(M, N, K, epi, lda) == plan["tiles"] == want[0]
            assert ext.gemm_nt_tail_plan(M, N, K, epi, lda) == (plan["tail_S"], plan["tail_r"]) == tuple(want[1:])
