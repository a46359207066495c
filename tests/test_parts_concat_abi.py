"""msha_concat_lists_device in the C ABI (include/mirsha.h "Part lists flattened on the
GPU"): the new symbols declared, exported and bound, MSHA_HAS_PARTS_CONCAT, the ABI
version still 10, msha_stats and the other counters unchanged, the msha_concat_stats
mirror laid out as the header's struct, bad arguments rejected without a GPU, and
Engine.concat_lists_device refusing bad tensors before anything reaches C. No compute
calls here (CPU suite)."""
import ctypes
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_concat_lists_device", "msha_get_concat_stats"]


def test_concat_symbols_declared_exported_and_bound():
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
    assert re.search(r"^#define MSHA_HAS_PARTS_CONCAT 1\s*$", text, re.M) and L.MSHA_HAS_PARTS_CONCAT == 1
    assert re.search(r"^#define MSHA_HAS_PARTS_PLANNED 1\s*$", text, re.M)
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    assert ctypes.sizeof(L.MshaStats) == 192


def test_stats_mirror_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(msha_concat_stats),\n'
                   '       offsetof(msha_concat_stats, last_bytes), offsetof(msha_concat_stats, last_kernel_ms),\n'
                   '       sizeof(msha_parts_plan_stats), sizeof(msha_parts_stats), sizeof(msha_stats));\n'
                   'return MSHA_HAS_PARTS_CONCAT == 1 ? 0 : 1;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, lbytes, lms, plan, parts, stats = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                                                    check=True).stdout.split())
    assert ctypes.sizeof(L.MshaConcatStats) == size == 40
    assert [f for f, _ in L.MshaConcatStats._fields_] == ["calls", "lists", "launches", "last_bytes",
                                                          "last_kernel_ms"]
    assert L.MshaConcatStats.last_bytes.offset == lbytes == 24
    assert L.MshaConcatStats.last_kernel_ms.offset == lms == 32
    # the older counters are as they were
    assert ctypes.sizeof(L.MshaPartsPlanStats) == plan == 72 and ctypes.sizeof(L.MshaPartsStats) == parts == 40
    assert stats == 192 == ctypes.sizeof(L.MshaStats)


def test_build_lists_agree():
    """The Makefile's SRCS and _lib._SRC_FILES name the same files in the same order
    (msha_build_id depends on it), the new ones included."""
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*?)\n(?!\s)", text, re.M | re.S).group(1).replace("\\\n", " ").split()
    assert srcs == [f.replace(os.sep, "/") for f in L._SRC_FILES]
    assert srcs[-3:] == ["parts_concat.hpp", "parts_concat.hip", "parts_concat.cpp"]
    assert L.build_id()["matches_tree"]


def test_bad_args_rejected_without_gpu():
    """A null context is refused whatever else is passed. (With a context each refusal
    has its own message: tests/test_gpu_parts_concat.py.)"""
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    f = lib.msha_concat_lists_device
    assert f(None, None, None, None, None, 1, None, 1, None, 0, None, None, None) == bad
    assert f(None, None, None, None, None, 0, None, 0, None, 0, None, None, None) == bad
    assert f(None, None, None, None, None, 2, None, 1, None, 0, None, None, None) == bad
    assert f(None, None, None, None, None, 0xFFFFFFFF, None, 0xFFFFFFFF, None, 0, None, None, None) == bad
    assert lib.msha_get_concat_stats(None, None) == bad
    s = L.MshaConcatStats()
    assert lib.msha_get_concat_stats(None, ctypes.byref(s)) == bad


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


def _good():
    import torch
    arena = torch.zeros(256, dtype=torch.uint8)
    dst = torch.zeros(512, dtype=torch.uint8)
    assert arena.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    po = torch.zeros(3, dtype=torch.int64)
    begin = torch.tensor([0, 1, 3], dtype=torch.int64)
    return arena, po, po.clone(), begin, dst, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)


def test_concat_rejects_a_wrong_device(eng_no_call):
    with pytest.raises(ValueError, match="cuda:0"):
        eng_no_call.concat_lists_device(*_good())             # host tensors


def test_concat_validates_tensors_before_the_call(eng_no_call, monkeypatch):
    """Wrong dtype, wrong msg_off / msg_len length, non-contiguous input, misaligned
    arena or dst: each raises before the C call. There is no GPU here, so host tensors
    are made to report the context's device; every other property checked is their own."""
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    eng = eng_no_call
    arena, po, pl, begin, dst, mo, ml = _good()
    called = "msha_concat_lists_device called"
    with pytest.raises(AssertionError, match=called):
        eng.concat_lists_device(arena, po, pl, begin, dst, mo, ml)          # the good calls are the only ones that get through
    sel = torch.tensor([1, 0, 1], dtype=torch.int32)
    three = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(AssertionError, match=called):
        eng.concat_lists_device(arena, po, pl, begin, dst, three, three.clone(), select=sel)
    with pytest.raises(ValueError, match="part_off must hold 8-byte"):
        eng.concat_lists_device(arena, po.int(), pl, begin, dst, mo, ml)
    with pytest.raises(ValueError, match="list_begin must hold 8-byte"):
        eng.concat_lists_device(arena, po, pl, begin.int(), dst, mo, ml)
    with pytest.raises(ValueError, match="msg_off must hold 8-byte"):
        eng.concat_lists_device(arena, po, pl, begin, dst, mo.int(), ml)
    with pytest.raises(ValueError, match="msg_len must hold 8-byte"):
        eng.concat_lists_device(arena, po, pl, begin, dst, mo, ml.double())
    with pytest.raises(ValueError, match="dst must hold 1-byte"):
        eng.concat_lists_device(arena, po, pl, begin, dst.view(torch.int32), mo, ml)
    with pytest.raises(ValueError, match="select must hold 4-byte"):
        eng.concat_lists_device(arena, po, pl, begin, dst, mo, ml, select=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="entries, expected 2"):
        eng.concat_lists_device(arena, po, pl, begin, dst, three, ml)
    with pytest.raises(ValueError, match="entries, expected 3"):
        eng.concat_lists_device(arena, po, pl, begin, dst, mo, ml, select=sel)
    with pytest.raises(ValueError, match="part_len has 2 entries"):
        eng.concat_lists_device(arena, po, pl[:2], begin, dst, mo, ml)
    with pytest.raises(ValueError, match="contiguous"):
        eng.concat_lists_device(arena, po, pl, begin, torch.zeros((8, 64), dtype=torch.uint8)[:, :32], mo, ml)
    with pytest.raises(ValueError, match="arena must start on a 16-byte boundary"):
        eng.concat_lists_device(arena[1:], po, pl, begin, dst, mo, ml)
    with pytest.raises(ValueError, match="dst must start on a 16-byte boundary"):
        eng.concat_lists_device(arena, po, pl, begin, dst[8:], mo, ml)


def test_engine_has_the_methods():
    from mirbft_amd.engine import Engine
    assert callable(Engine.concat_lists_device) and callable(Engine.concat_stats)
