"""csrc/build.py names every object after a hash of what it is compiled from.  jm_api.h is the
interface between bindings.cpp and the kernel files (by-value structs, default arguments), so an
edit to a header must rename the bindings object as well as every kernel object -- a cached object
with the old struct layouts would otherwise be linked against the rebuilt kernels.  No compiler
runs here: ``plan`` only returns the objects and their commands."""

import shutil

import pytest

from jumbo_mae_tpu_amd.csrc import build as B


@pytest.fixture()
def csrc(tmp_path):
    src = tmp_path / "csrc"
    src.mkdir()
    for f in B.HERE.iterdir():
        if f.suffix in (".hip", ".h", ".cpp"):
            shutil.copy(f, src / f.name)
    return src


def _objects(src, tmp_path, variant="release"):
    """{source file name: object file name} of the plan for the copy at ``src``"""
    jobs = B.plan(variant, src_dir=src, out_dir=tmp_path / "obj")
    out = {}
    for obj, cmd in jobs:
        assert obj.parent == tmp_path / "obj" and cmd[-1] == str(obj)
        source = cmd[cmd.index("-c") + 1]
        assert source.startswith(str(src))
        out[source[len(str(src)) + 1:]] = obj.name
    return out


def _flip_first_byte(path):
    data = bytearray(path.read_bytes())
    data[0] ^= 1
    path.write_bytes(bytes(data))


def test_plan_covers_every_translation_unit(csrc, tmp_path):
    objs = _objects(csrc, tmp_path)
    assert sorted(objs) == sorted(B.KERNELS + ["bindings.cpp"])
    assert len(set(objs.values())) == len(objs)
    assert _objects(csrc, tmp_path) == objs  # a pure function of the files
    assert not (tmp_path / "obj").exists()   # and of nothing else: it ran nothing


@pytest.mark.parametrize("variant", ["release", "debug"])
def test_header_edit_renames_every_object(csrc, tmp_path, variant):
    before = _objects(csrc, tmp_path, variant)
    _flip_first_byte(csrc / "jm_api.h")
    after = _objects(csrc, tmp_path, variant)
    assert before.keys() == after.keys()
    same = [k for k in before if before[k] == after[k]]
    assert same == [], f"objects that a jm_api.h edit would not rebuild: {same}"


def test_kernel_edit_renames_only_its_object(csrc, tmp_path):
    before = _objects(csrc, tmp_path)
    _flip_first_byte(csrc / "gemm_tn.hip")
    after = _objects(csrc, tmp_path)
    changed = [k for k in before if before[k] != after[k]]
    assert changed == ["gemm_tn.hip"]
    _flip_first_byte(csrc / "bindings.cpp")
    last = _objects(csrc, tmp_path)
    assert [k for k in after if after[k] != last[k]] == ["bindings.cpp"]


def test_variants_do_not_share_objects(csrc, tmp_path):
    rel, dbg = _objects(csrc, tmp_path, "release"), _objects(csrc, tmp_path, "debug")
    assert all(rel[k] != dbg[k] for k in rel)
