"""The whole-sequence attention kernels of csrc/attention.hip (S <= 224, head dims 32 / 64) bit for bit
against digests recorded from the commit before their launchers and dispatch were refactored: the guard
for any later change that must leave their results as they are (tests/attn_bits.py has the cases and how
the golden file is written) (MI355X)."""

import json

import pytest
import torch

import attn_bits as A

pytestmark = pytest.mark.gpu

IDS = [A.case_id(s) for s in A.CASES]


@pytest.fixture(scope="module")
def ext():
    from jumbo_mae_tpu_amd.ops import _ext
    return _ext.load(True)


@pytest.fixture(scope="module")
def golden():
    return json.loads(A.GOLDEN.read_text())


def test_golden_lists_the_cases(golden):
    assert sorted(golden) == sorted(IDS)


@pytest.mark.parametrize("shape", A.CASES, ids=IDS)
def test_whole_seq_bits(ext, golden, shape):
    want = golden[A.case_id(shape)]
    got = {}
    for mode in ("nodrop", "drop"):
        got[mode] = A.run_case(ext, shape, mode == "drop")
        # the inputs first: a change in the host's random stream is that, not a kernel difference
        for k in A.INPUTS:
            assert got[mode][k] == want[mode][k], f"{mode}: the host generator gave other inputs ({k})"
    for mode in ("nodrop", "drop"):
        for k in A.OUTPUTS:
            assert got[mode][k] == want[mode][k], f"{mode}: {k} differs from the recorded bits"
    # the dropout mask is live and no output is a constant (lse is that of the undropped P: equal by design)
    for k in ("o", "dqkv", "dbias"):
        assert got["drop"][k] != got["nodrop"][k], k
    assert got["drop"]["lse"] == got["nodrop"]["lse"]
