"""csrc/gemm_plan.h on the CPU: tests/gemm_plan_driver.cpp, built with the address and undefined-behaviour
sanitizers, plans every case of tests/gemm_plan_cases.py at the recorded CU count; the plans must give the
tiles and tail splits of tests/golden/gemm_nt_plans.json and be consistent in themselves (check_plan)."""

import shutil
import subprocess
from pathlib import Path

import pytest

import gemm_plan_cases as C

HERE = Path(__file__).resolve().parent
CSRC = HERE.parent / "jumbo_mae_tpu_amd" / "csrc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tests/gemm_plan_driver.cpp")
    exe = tmp_path_factory.mktemp("gemm_plan") / "driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I" + str(CSRC), str(HERE / "gemm_plan_driver.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def plan_all(driver, requests):
    """requests: (M, N, K, epi, lda, splits, ncu, path, rows) -> one FIELDS dict each."""
    text = "".join(" ".join(str(v) for v in q) + "\n" for q in requests)
    r = subprocess.run([str(driver)], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(requests)
    return [dict(zip(C.FIELDS, map(int, ln.split()))) for ln in lines]


def test_gemm_plan_matches_golden(driver):
    g = C.load_golden()
    todo = []
    for case in C.CASES:
        M, N, K, lda = case
        for (epi, (path, rows)), want in zip(C.combos(), g["cases"][C.case_id(case)], strict=True):
            for splits in (C.PARTIAL_SPLITS if epi == 3 else (1,)):
                todo.append((case, epi, splits, want, (M, N, K, epi, lda, splits, g["cus"], path, rows)))
    plans = plan_all(driver, [t[4] for t in todo])
    for (case, epi, splits, want, _), plan in zip(todo, plans, strict=True):
        C.check_plan(plan, want, case, epi, splits)


def test_gemm_plan_odd_arguments(driver):
    """Arguments that jm_gemm_nt refuses, and a device of one CU: a status, no trap under the sanitizers."""
    reqs = [(0, 256, 128, 0, 128, 1, 256, 0, 0), (256, 0, 128, 0, 128, 1, 256, 0, 0), (256, 256, 96, 0, 96, 1, 256, 0, 0),
            (256, 258, 128, 0, 128, 1, 256, 0, 0), (256, 256, 128, 5, 128, 1, 256, 0, 0),
            (256, 256, 128, 9, 128, 1, 256, 0, 0), (256, 256, 128, 3, 128, 0, 256, 0, 0),
            (2 ** 31 - 1, 4, 64, 0, 2 ** 30, 1, 1, 0, 0), (11008, 7936, 1024, 0, 1024, 1, 0, 0, 0)]
    plans = plan_all(driver, reqs)
    assert [p["status"] for p in plans] == [-1, -1, -1, -1, -3, -3, -4, -2, 0]
