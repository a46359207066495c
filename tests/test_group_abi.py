"""msha_group_digests_device in the C ABI (include/mirsha.h "Digests grouped by value on
the GPU"): the new symbols declared, exported and bound, MSHA_HAS_GROUP_DEVICE, the ABI
version still 10, the two struct mirrors laid out as the header's, the build lists naming
the three new files, a null context rejected without a GPU, and
Engine.group_digests_device refusing bad tensors before anything reaches C. No compute
calls here (CPU suite)."""
import ctypes
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_group_digests_device", "msha_get_group_stats"]
NEW_FILES = ["group.hpp", "group.hip", "group.cpp"]


def test_group_symbols_declared_exported_and_bound():
    declared = set(L.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = L.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in L.SIGNATURES and hasattr(lib, s), s
    assert len(L.SIGNATURES["msha_group_digests_device"][1]) == 12


def test_header_constants_and_abi_version():
    text = open(L.HEADER_PATH).read()
    assert re.search(r"^#define MSHA_HAS_GROUP_DEVICE 1\s*$", text, re.M) and L.MSHA_HAS_GROUP_DEVICE == 1
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    assert ctypes.sizeof(L.MshaStats) == 192
    # the reference sites the contract cites
    for site in ("sequence.go:73-74, 271-277, 331-340", "checkpoints.go:264-290",
                 "client_hash_disseminator.go:346-349, 415-504", "batch_tracker.go:20, 85-91",
                 "epoch_change.go:23, 42-50"):
        assert site in text, site


def test_struct_mirrors_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(msha_group_result),\n'
                   '       offsetof(msha_group_result, n), offsetof(msha_group_result, groups),\n'
                   '       offsetof(msha_group_result, listed), offsetof(msha_group_result, max_count),\n'
                   '       offsetof(msha_group_result, max_group));\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(msha_group_stats),\n'
                   '       offsetof(msha_group_stats, calls), offsetof(msha_group_stats, digests),\n'
                   '       offsetof(msha_group_stats, launches), offsetof(msha_group_stats, table_slots),\n'
                   '       offsetof(msha_group_stats, last_kernel_ms));\n'
                   'printf("%zu %zu %zu\\n", sizeof(msha_verify_result), sizeof(msha_verify_stats), sizeof(msha_stats));\n'
                   'return MSHA_HAS_GROUP_DEVICE == 1 ? 0 : 1;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    res, st, old = (list(map(int, ln.split())) for ln in
                    subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [f for f, _ in L.MshaGroupResult._fields_] == ["n", "groups", "listed", "max_count", "max_group"]
    assert res == [40, 0, 8, 16, 24, 32] == [ctypes.sizeof(L.MshaGroupResult)] + [
        getattr(L.MshaGroupResult, f).offset for f, _ in L.MshaGroupResult._fields_]
    assert [f for f, _ in L.MshaGroupStats._fields_] == ["calls", "digests", "launches", "table_slots",
                                                         "last_kernel_ms"]
    assert st == [40, 0, 8, 16, 24, 32] == [ctypes.sizeof(L.MshaGroupStats)] + [
        getattr(L.MshaGroupStats, f).offset for f, _ in L.MshaGroupStats._fields_]
    assert L.MshaGroupStats._fields_[-1][1] is ctypes.c_double
    # the older structs are as they were
    assert old == [40, 40, 192] == [ctypes.sizeof(L.MshaVerifyResult), ctypes.sizeof(L.MshaVerifyStats),
                                    ctypes.sizeof(L.MshaStats)]


def test_build_lists_name_the_new_files():
    """The Makefile's SRCS and _lib._SRC_FILES name the same files in the same order
    (msha_build_id depends on it), the three new ones included, and the library is the
    tree's build."""
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*?)\n(?!\s)", text, re.M | re.S).group(1).replace("\\\n", " ").split()
    assert srcs == [f.replace(os.sep, "/") for f in L._SRC_FILES]
    for f in NEW_FILES:
        assert srcs.count(f) == 1 and os.path.exists(os.path.join(ROOT, "mirbft_amd", "csrc", f)), f
    assert "group_kernels.o" in text and "$(BUILD)/group.o" in text
    assert L.build_id()["matches_tree"]


def test_bad_args_rejected_without_gpu():
    """A null context is refused whatever else is passed. (With a context each refusal
    has its own message: tests/test_gpu_group.py.)"""
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    f = lib.msha_group_digests_device
    assert f(None, None, 1, None, None, None, None, None, None, 0, None, None) == bad
    assert f(None, None, 0, None, None, None, None, None, None, 0, None, None) == bad
    assert f(None, None, (1 << 30) + 1, None, None, None, None, None, None, 4, None, None) == bad
    assert lib.msha_get_group_stats(None, None) == bad
    s = L.MshaGroupStats()
    assert lib.msha_get_group_stats(None, ctypes.byref(s)) == bad


@pytest.fixture
def eng_no_call():
    from mirbft_amd.engine import Engine
    eng = Engine.__new__(Engine)      # no context needed: validation runs first
    eng._dev_index = 0
    eng._ctx = None

    class NoCall:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    eng._lib = NoCall()
    return eng


def _good(n=70):
    import torch
    digests = torch.zeros(32 * n, dtype=torch.uint8)
    assert digests.data_ptr() % 16 == 0
    return digests, torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32), torch.zeros(5, dtype=torch.int64)


def test_group_rejects_a_wrong_device(eng_no_call):
    with pytest.raises(ValueError, match="cuda:0"):
        eng_no_call.group_digests_device(*_good())            # host tensors


def test_group_validates_tensors_before_the_call(eng_no_call, monkeypatch):
    """Wrong dtype or length, rows that are not 32 bytes, one group array without the
    other, a misaligned table: each raises before the C call. There is no GPU here, so
    host tensors are made to report the context's device; every other property checked
    is their own."""
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    eng = eng_no_call
    dig, first, group, res = _good()
    called = "msha_group_digests_device called"
    i32 = lambda k: torch.zeros(k, dtype=torch.int32)                      # noqa: E731
    with pytest.raises(AssertionError, match=called):
        eng.group_digests_device(dig, first, group, res)      # the good calls are the only ones that get through
    with pytest.raises(AssertionError, match=called):
        eng.group_digests_device(dig, first, group, res, scope=i32(70), members=i32(70), group_first=i32(8),
                                 group_count=i32(8))
    with pytest.raises(ValueError, match="digests must hold 1-byte"):
        eng.group_digests_device(dig.view(torch.int32), first, group, res)
    with pytest.raises(ValueError, match="first must hold 4-byte"):
        eng.group_digests_device(dig, first.long(), group, res)
    with pytest.raises(ValueError, match="scope must hold 4-byte"):
        eng.group_digests_device(dig, first, group, res, scope=torch.zeros(70, dtype=torch.int64))
    with pytest.raises(ValueError, match="result must hold 8-byte"):
        eng.group_digests_device(dig, first, group, res.int())
    with pytest.raises(ValueError, match="result must hold 5 words"):
        eng.group_digests_device(dig, first, group, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="32-byte rows"):
        eng.group_digests_device(dig[:-1], first, group, res)
    with pytest.raises(ValueError, match="group has 69 entries, expected 70"):
        eng.group_digests_device(dig, first, group[:69], res)
    with pytest.raises(ValueError, match="scope has 71 entries"):
        eng.group_digests_device(dig, first, group, res, scope=i32(71))
    with pytest.raises(ValueError, match="members has 1 entries"):
        eng.group_digests_device(dig, first, group, res, members=i32(1))
    with pytest.raises(ValueError, match="both or neither"):
        eng.group_digests_device(dig, first, group, res, group_first=i32(8))
    with pytest.raises(ValueError, match="group_count has 7 entries, group_first 8"):
        eng.group_digests_device(dig, first, group, res, group_first=i32(8), group_count=i32(7))
    with pytest.raises(ValueError, match="contiguous"):
        eng.group_digests_device(torch.zeros((70, 64), dtype=torch.uint8)[:, :32], first, group, res)
    with pytest.raises(ValueError, match="digests must start on a 16-byte boundary"):
        eng.group_digests_device(torch.zeros(32 * 70 + 8, dtype=torch.uint8)[8:], first, group, res)


def test_engine_and_package_have_the_entry():
    import mirbft_amd
    from mirbft_amd.engine import Engine
    assert callable(Engine.group_digests_device) and callable(Engine.group_stats)
    for name in ("tally_digests_device", "dedupe_digests_device"):
        assert callable(getattr(mirbft_amd, name)) and name in mirbft_amd.__all__
