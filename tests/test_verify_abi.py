"""msha_verify_digests_device in the C ABI (include/mirsha.h "Digests verified on the
GPU"): the new symbols declared, exported and bound, MSHA_HAS_VERIFY_DEVICE, the ABI
version still 10, the two struct mirrors laid out as the header's, the build lists
naming the three new files, a null context rejected without a GPU, and
Engine.verify_digests_device refusing bad tensors before anything reaches C. No compute
calls here (CPU suite)."""
import ctypes
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_verify_digests_device", "msha_get_verify_stats"]
NEW_FILES = ["verify.hpp", "verify.hip", "verify.cpp"]


def test_verify_symbols_declared_exported_and_bound():
    declared = set(L.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = L.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in L.SIGNATURES and hasattr(lib, s), s


def test_header_constants_and_abi_version():
    text = open(L.HEADER_PATH).read()
    assert re.search(r"^#define MSHA_HAS_VERIFY_DEVICE 1\s*$", text, re.M) and L.MSHA_HAS_VERIFY_DEVICE == 1
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    assert ctypes.sizeof(L.MshaStats) == 192
    # the three reference sites the contract cites
    for site in ("batch_tracker.go:167-195", "clients.go:152-177", "epoch_target.go:486-528"):
        assert site in text, site


def test_struct_mirrors_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(msha_verify_result),\n'
                   '       offsetof(msha_verify_result, n), offsetof(msha_verify_result, bad),\n'
                   '       offsetof(msha_verify_result, first_bad), offsetof(msha_verify_result, listed),\n'
                   '       offsetof(msha_verify_result, bad_index));\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(msha_verify_stats),\n'
                   '       offsetof(msha_verify_stats, calls), offsetof(msha_verify_stats, digests),\n'
                   '       offsetof(msha_verify_stats, launches), offsetof(msha_verify_stats, scan_words),\n'
                   '       offsetof(msha_verify_stats, last_kernel_ms));\n'
                   'printf("%zu %zu\\n", sizeof(msha_concat_stats), sizeof(msha_stats));\n'
                   'return MSHA_HAS_VERIFY_DEVICE == 1 ? 0 : 1;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    res, st, old = (list(map(int, ln.split())) for ln in
                    subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [f for f, _ in L.MshaVerifyResult._fields_] == ["n", "bad", "first_bad", "listed", "bad_index"]
    assert res == [40, 0, 8, 16, 24, 32] == [ctypes.sizeof(L.MshaVerifyResult)] + [
        getattr(L.MshaVerifyResult, f).offset for f, _ in L.MshaVerifyResult._fields_]
    assert [f for f, _ in L.MshaVerifyStats._fields_] == ["calls", "digests", "launches", "scan_words",
                                                          "last_kernel_ms"]
    assert st == [40, 0, 8, 16, 24, 32] == [ctypes.sizeof(L.MshaVerifyStats)] + [
        getattr(L.MshaVerifyStats, f).offset for f, _ in L.MshaVerifyStats._fields_]
    assert L.MshaVerifyStats._fields_[-1][1] is ctypes.c_double
    # the older counters are as they were
    assert old == [40, 192] == [ctypes.sizeof(L.MshaConcatStats), ctypes.sizeof(L.MshaStats)]


def test_build_lists_name_the_new_files():
    """The Makefile's SRCS and _lib._SRC_FILES name the same files in the same order
    (msha_build_id depends on it), the three new ones included, and the library is the
    tree's build."""
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*?)\n(?!\s)", text, re.M | re.S).group(1).replace("\\\n", " ").split()
    assert srcs == [f.replace(os.sep, "/") for f in L._SRC_FILES]
    for f in NEW_FILES:
        assert srcs.count(f) == 1 and os.path.exists(os.path.join(ROOT, "mirbft_amd", "csrc", f)), f
    assert "verify_kernels.o" in text and "$(BUILD)/verify.o" in text
    assert L.build_id()["matches_tree"]


def test_bad_args_rejected_without_gpu():
    """A null context is refused whatever else is passed. (With a context each refusal
    has its own message: tests/test_gpu_verify.py.)"""
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    f = lib.msha_verify_digests_device
    assert f(None, None, 1, None, 1, None, None, None, 0, None, None) == bad
    assert f(None, None, 0, None, 0, None, None, None, 0, None, None) == bad
    assert f(None, None, 0xFFFFFFFF, None, 1, None, None, None, 4, None, None) == bad
    assert lib.msha_get_verify_stats(None, None) == bad
    s = L.MshaVerifyStats()
    assert lib.msha_get_verify_stats(None, ctypes.byref(s)) == bad


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
    got = torch.zeros(32 * n, dtype=torch.uint8)
    exp = torch.zeros(32 * n, dtype=torch.uint8)
    assert got.data_ptr() % 16 == 0 and exp.data_ptr() % 16 == 0
    return got, exp, torch.zeros((n + 63) // 64, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)


def test_verify_rejects_a_wrong_device(eng_no_call):
    with pytest.raises(ValueError, match="cuda:0"):
        eng_no_call.verify_digests_device(*_good())           # host tensors


def test_verify_validates_tensors_before_the_call(eng_no_call, monkeypatch):
    """Wrong dtype or length, rows that are not 32 bytes, a short mask, a misaligned
    table: each raises before the C call. There is no GPU here, so host tensors are made
    to report the context's device; every other property checked is their own."""
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    eng = eng_no_call
    got, exp, mask, res = _good()
    called = "msha_verify_digests_device called"
    with pytest.raises(AssertionError, match=called):
        eng.verify_digests_device(got, exp, mask, res)        # the good calls are the only ones that get through
    idx = torch.zeros(70, dtype=torch.int32)
    lst = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(AssertionError, match=called):
        eng.verify_digests_device(got, exp[:64], mask, res, expected_idx=idx, bad_list=lst)
    with pytest.raises(ValueError, match="mask must hold 8-byte"):
        eng.verify_digests_device(got, exp, mask.int(), res)
    with pytest.raises(ValueError, match="result must hold 8-byte"):
        eng.verify_digests_device(got, exp, mask, res.int())
    with pytest.raises(ValueError, match="result must hold 5 words"):
        eng.verify_digests_device(got, exp, mask, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="got must hold 1-byte"):
        eng.verify_digests_device(got.view(torch.int32), exp, mask, res)
    with pytest.raises(ValueError, match="expected_idx must hold 4-byte"):
        eng.verify_digests_device(got, exp, mask, res, expected_idx=torch.zeros(70, dtype=torch.int64))
    with pytest.raises(ValueError, match="bad_list must hold 4-byte"):
        eng.verify_digests_device(got, exp, mask, res, bad_list=torch.zeros(8, dtype=torch.int64))
    with pytest.raises(ValueError, match="32-byte rows"):
        eng.verify_digests_device(got[:-1], exp, mask, res)
    with pytest.raises(ValueError, match="as many rows as got"):
        eng.verify_digests_device(got, exp[:64], mask, res)
    with pytest.raises(ValueError, match="expected_idx has 69 entries"):
        eng.verify_digests_device(got, exp, mask, res, expected_idx=idx[:69])
    with pytest.raises(ValueError, match="mask holds 1 words, needs 2"):
        eng.verify_digests_device(got, exp, mask[:1], res)
    with pytest.raises(ValueError, match="contiguous"):
        eng.verify_digests_device(torch.zeros((70, 64), dtype=torch.uint8)[:, :32], exp, mask, res)
    with pytest.raises(ValueError, match="expected must start on a 16-byte boundary"):
        eng.verify_digests_device(got, torch.zeros(32 * 70 + 8, dtype=torch.uint8)[8:], mask, res)
    with pytest.raises(ValueError, match="got must start on a 16-byte boundary"):
        eng.verify_digests_device(torch.zeros(32 * 70 + 8, dtype=torch.uint8)[8:], exp, mask, res)


def test_engine_and_package_have_the_entry():
    import mirbft_amd
    from mirbft_amd.engine import Engine
    assert callable(Engine.verify_digests_device) and callable(Engine.verify_stats)
    assert callable(mirbft_amd.verify_batches_device) and "verify_batches_device" in mirbft_amd.__all__
