"""msha_hash_actions_device_planned in the C ABI (include/mirsha.h "Multi-part actions
through part LISTS"): the new symbols declared, exported and bound,
MSHA_HAS_PARTS_PLANNED, the ABI version, msha_stats and msha_parts_stats unchanged, the
msha_parts_plan_stats mirror laid out as the header's struct, bad arguments rejected
without a GPU, Engine.hash_actions_device_planned refusing bad tensors before anything
reaches C, and the block-count -> class-key function (mirbft_amd/csrc/parts_plan.hpp)
under AddressSanitizer + UBSan as a stand-alone program. No compute calls here (CPU
suite)."""
import ctypes
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_hash_actions_device_planned", "msha_get_parts_plan_stats", "msha_parts_plan_read_order"]


def test_planned_symbols_declared_exported_and_bound():
    declared = set(L.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = L.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in L.SIGNATURES and hasattr(lib, s), s


def test_header_constants_abi_version_and_stats_size():
    text = open(L.HEADER_PATH).read()
    assert re.search(r"^#define MSHA_HAS_PARTS_PLANNED 1\s*$", text, re.M)
    assert re.search(r"^enum \{ MSHA_PARTS_FOLD = 1u \};", text, re.M) and L.MSHA_PARTS_FOLD == 1
    assert re.search(r"^#define MSHA_HAS_PARTS_DEVICE 1\s*$", text, re.M)
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    assert ctypes.sizeof(L.MshaStats) == 192


def test_stats_mirrors_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu\\n", sizeof(msha_parts_plan_stats),\n'
                   '       offsetof(msha_parts_plan_stats, last_kernel_ms), sizeof(msha_parts_stats),\n'
                   '       offsetof(msha_parts_stats, last_kernel_ms), sizeof(msha_stats));\n'
                   'return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, last, psize, plast, stats = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                                              check=True).stdout.split())
    assert ctypes.sizeof(L.MshaPartsPlanStats) == size == 72
    assert [f for f, _ in L.MshaPartsPlanStats._fields_] == [
        "calls", "actions", "lists", "last_lanes", "last_blocks", "launches_plan", "launches_hash",
        "launches_fill", "last_kernel_ms"]
    assert L.MshaPartsPlanStats.last_kernel_ms.offset == last == 64
    # msha_parts_stats and msha_stats are as they were
    assert ctypes.sizeof(L.MshaPartsStats) == psize == 40 and L.MshaPartsStats.last_kernel_ms.offset == plast == 32
    assert [f for f, _ in L.MshaPartsStats._fields_] == ["calls", "actions", "launches", "last_lanes",
                                                         "last_kernel_ms"]
    assert stats == 192 == ctypes.sizeof(L.MshaStats)


def test_bad_args_rejected_without_gpu():
    """No context can exist here, and a null context is refused whatever else is passed:
    null pointers, an unknown flag, counts that disagree or are out of range, zero
    actions. (With a context each has its own message: tests/test_gpu_parts_planned.py.)"""
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    f = lib.msha_hash_actions_device_planned
    assert f(None, None, None, None, None, 1, None, 1, 0, None, None) == bad
    assert f(None, None, None, None, None, 0, None, 0, 0, None, None) == bad
    assert f(None, None, None, None, None, 1, None, 1, 2, None, None) == bad          # an unknown flag
    assert f(None, None, None, None, None, 2, None, 1, 0, None, None) == bad          # n_actions != n_lists
    assert f(None, None, None, None, None, 0xFFFFFFFF, None, 0xFFFFFFFF, 0, None, None) == bad
    assert lib.msha_get_parts_plan_stats(None, None) == bad
    s = L.MshaPartsPlanStats()
    assert lib.msha_get_parts_plan_stats(None, ctypes.byref(s)) == bad
    n = ctypes.c_uint64(7)
    assert lib.msha_parts_plan_read_order(None, None, 0, ctypes.byref(n)) == bad
    assert lib.msha_parts_plan_read_order(None, None, 0, None) == bad


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
    assert arena.data_ptr() % 16 == 0
    po = torch.zeros(3, dtype=torch.int64)
    begin = torch.tensor([0, 1, 3], dtype=torch.int64)
    out = torch.zeros((2, 32), dtype=torch.uint8)
    return arena, po, po.clone(), begin, out


def test_planned_rejects_a_wrong_device(eng_no_call):
    arena, po, pl, begin, out = _good()           # host tensors
    with pytest.raises(ValueError, match="cuda:0"):
        eng_no_call.hash_actions_device_planned(arena, po, pl, begin, out)


def test_planned_validates_tensors_before_the_call(eng_no_call, monkeypatch):
    """Wrong dtype, wrong list_begin or action_list length, short out, non-contiguous
    input, misaligned arena: each raises before the C call. There is no GPU here, so
    host tensors are made to report the context's device; every other property checked
    is their own."""
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    eng = eng_no_call
    arena, po, pl, begin, out = _good()
    called = "msha_hash_actions_device_planned called"
    with pytest.raises(AssertionError, match=called):
        eng.hash_actions_device_planned(arena, po, pl, begin, out)      # the good calls are the only ones that get through
    al = torch.tensor([1, 0, 1, 1], dtype=torch.int32)
    with pytest.raises(AssertionError, match=called):
        eng.hash_actions_device_planned(arena, po, pl, begin, torch.zeros((4, 32), dtype=torch.uint8), action_list=al)
    with pytest.raises(ValueError, match="part_off must hold 8-byte"):
        eng.hash_actions_device_planned(arena, po.int(), pl, begin, out)
    with pytest.raises(ValueError, match="part_len must hold 8-byte"):
        eng.hash_actions_device_planned(arena, po, pl.double(), begin, out)
    with pytest.raises(ValueError, match="list_begin must hold 8-byte"):
        eng.hash_actions_device_planned(arena, po, pl, begin.int(), out)
    with pytest.raises(ValueError, match="arena must hold 1-byte"):
        eng.hash_actions_device_planned(arena.view(torch.int32), po, pl, begin, out)
    with pytest.raises(ValueError, match="action_list must hold 4-byte"):
        eng.hash_actions_device_planned(arena, po, pl, begin, out, action_list=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="action_list must hold 4-byte"):
        eng.hash_actions_device_planned(arena, po, pl, begin, out, action_list=torch.zeros(2, dtype=torch.float32))
    with pytest.raises(ValueError, match="action_list has 3 entries, expected 2"):
        eng.hash_actions_device_planned(arena, po, pl, begin, out, action_list=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="list_begin has 4 entries, expected 3"):
        eng.hash_actions_device_planned(arena, po, pl, torch.tensor([0, 1, 2, 3]), out)
    with pytest.raises(ValueError, match="list_begin has 3 entries, expected 2"):
        eng.hash_actions_device_planned(arena, po, pl, begin, out[:1])
    with pytest.raises(ValueError, match="not a multiple of 32"):
        eng.hash_actions_device_planned(arena, po, pl, begin, out.view(-1)[:63])
    with pytest.raises(ValueError, match="part_len has 2 entries"):
        eng.hash_actions_device_planned(arena, po, pl[:2], begin, out)
    with pytest.raises(ValueError, match="contiguous"):
        eng.hash_actions_device_planned(arena, po, pl, begin, torch.zeros((2, 64), dtype=torch.uint8)[:, :32])
    with pytest.raises(ValueError, match="16-byte boundary"):
        eng.hash_actions_device_planned(arena[1:], po, pl, begin, out)


def test_engine_has_the_methods():
    from mirbft_amd.engine import Engine
    assert callable(Engine.hash_actions_device_planned) and callable(Engine.parts_plan_stats)
    assert callable(Engine.parts_plan_order)


def _key(blocks: int) -> int:
    """The rule restated: the exact block count below 4,096 blocks, floor(log2) from
    there up; keys are descending classes, 52 power-of-two classes first."""
    if blocks < 4096:
        return 52 + 4095 - blocks
    return 63 - (blocks.bit_length() - 1)


def test_class_key_under_asan_ubsan(tmp_path):
    counts = [0, 1, 4095, 4096, 4097]
    for k in range(1, 33):
        counts += [c for c in ((1 << k) - 1, 1 << k, (1 << k) + 1) if c <= (1 << 32) - 1]
    counts = sorted(set(counts))
    assert counts[-1] == (1 << 32) - 1 and {8191, 8192, 8193} <= set(counts)
    exe = tmp_path / "parts_plan_key_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "parts_plan_key_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + [str(c) for c in counts], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "parts_plan keys ok: %d block counts" % len(counts) in r.stdout
    got = dict(tuple(map(int, ln.split())) for ln in r.stdout.splitlines() if re.fullmatch(r"\d+ \d+", ln))
    assert got == {c: _key(c) for c in counts}
    keys = [got[c] for c in counts]
    assert keys == sorted(keys, reverse=True) and keys[0] == 4147 and min(keys) == 63 - 31
