"""msha_hash_actions_device in the C ABI (include/mirsha.h "ProcessHashActions from
HBM"): the new symbols exported and bound, MSHA_HAS_PARTS_DEVICE, the ABI version and
msha_stats unchanged, the msha_parts_stats mirror laid out as the header's struct, null
arguments rejected without a GPU, and Engine.hash_actions_device refusing bad tensors
before anything reaches C. No compute calls here (CPU suite)."""
import ctypes
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_hash_actions_device", "msha_get_parts_stats"]


def test_parts_symbols_declared_exported_and_bound():
    declared = set(L.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = L.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in L.SIGNATURES and hasattr(lib, s), s


def test_header_constant_abi_version_and_stats_size():
    text = open(L.HEADER_PATH).read()
    assert re.search(r"^#define MSHA_HAS_PARTS_DEVICE 1\s*$", text, re.M)
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    assert ctypes.sizeof(L.MshaStats) == 192


def test_parts_stats_mirror_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu\\n", sizeof(msha_parts_stats), offsetof(msha_parts_stats, last_kernel_ms),\n'
                   '       sizeof(msha_stats));\n'
                   'return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, last, stats = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                                check=True).stdout.split())
    assert ctypes.sizeof(L.MshaPartsStats) == size
    assert L.MshaPartsStats._fields_[-1][0] == "last_kernel_ms" and L.MshaPartsStats.last_kernel_ms.offset == last
    assert stats == 192 == ctypes.sizeof(L.MshaStats)      # msha_stats did not grow


def test_null_args_rejected_without_gpu():
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    assert lib.msha_hash_actions_device(None, None, None, None, None, None, 1, None, None) == bad
    assert lib.msha_hash_actions_device(None, None, None, None, None, None, 0, None, None) == bad
    assert lib.msha_get_parts_stats(None, None) == bad
    s = L.MshaPartsStats()
    assert lib.msha_get_parts_stats(None, ctypes.byref(s)) == bad


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


def test_hash_actions_device_rejects_a_wrong_device(eng_no_call):
    arena, po, pl, begin, out = _good()           # host tensors
    with pytest.raises(ValueError, match="cuda:0"):
        eng_no_call.hash_actions_device(arena, po, pl, begin, out)


def test_hash_actions_device_validates_tensors_before_the_call(eng_no_call, monkeypatch):
    """Wrong dtype, wrong begin length, short out, non-contiguous input, misaligned
    arena: each raises before the C call. There is no GPU here, so host tensors are made
    to report the context's device; every other property checked is their own."""
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    eng = eng_no_call
    arena, po, pl, begin, out = _good()
    with pytest.raises(AssertionError, match="msha_hash_actions_device called"):
        eng.hash_actions_device(arena, po, pl, begin, out)      # the good call is the only one that gets through
    with pytest.raises(ValueError, match="part_off must hold 8-byte"):
        eng.hash_actions_device(arena, po.int(), pl, begin, out)
    with pytest.raises(ValueError, match="part_len must hold 8-byte"):
        eng.hash_actions_device(arena, po, pl.double(), begin, out)
    with pytest.raises(ValueError, match="begin must hold 8-byte"):
        eng.hash_actions_device(arena, po, pl, begin.int(), out)
    with pytest.raises(ValueError, match="arena must hold 1-byte"):
        eng.hash_actions_device(arena.view(torch.int32), po, pl, begin, out)
    with pytest.raises(ValueError, match="order must hold 4-byte"):
        eng.hash_actions_device(arena, po, pl, begin, out, order=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="order has 3 entries"):
        eng.hash_actions_device(arena, po, pl, begin, out, order=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="begin has 4 entries, expected 3"):
        eng.hash_actions_device(arena, po, pl, torch.tensor([0, 1, 2, 3]), out)
    with pytest.raises(ValueError, match="begin has 3 entries, expected 2"):
        eng.hash_actions_device(arena, po, pl, begin, out[:1])
    with pytest.raises(ValueError, match="not a multiple of 32"):
        eng.hash_actions_device(arena, po, pl, begin, out.view(-1)[:63])
    with pytest.raises(ValueError, match="part_len has 2 entries"):
        eng.hash_actions_device(arena, po, pl[:2], begin, out)
    with pytest.raises(ValueError, match="contiguous"):
        eng.hash_actions_device(arena, po, pl, begin, torch.zeros((2, 64), dtype=torch.uint8)[:, :32])
    with pytest.raises(ValueError, match="16-byte boundary"):
        eng.hash_actions_device(arena[1:], po, pl, begin, out)


def test_engine_has_the_methods():
    from mirbft_amd.engine import Engine
    assert callable(Engine.hash_actions_device) and callable(Engine.parts_stats)
