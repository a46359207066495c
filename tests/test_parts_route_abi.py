"""msha_hash_actions_device_routed in the C ABI (include/mirsha.h "Part lists with their
long lists routed to the chains"): the header compiles as C, the new symbols are
declared, exported and bound, MSHA_HAS_PARTS_ROUTED is defined, the ctypes mirrors are
laid out as the header's structs, the older stat structs keep their sizes, a null
context is refused, and Engine.hash_actions_device_routed refuses bad arguments before
anything reaches C. No compute calls here (CPU suite)."""
import ctypes
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_hash_actions_device_routed", "msha_get_parts_route_stats", "msha_parts_route_read",
               "msha_parts_route_read_order"]


def test_routed_symbols_declared_exported_and_bound():
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
    assert re.search(r"^#define MSHA_HAS_PARTS_ROUTED 1\s*$", text, re.M) and L.MSHA_HAS_PARTS_ROUTED == 1
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    m = re.search(r"^#define MSHA_ROUTE_LONG_BLOCKS_DEFAULT (\d+)u\s*$", text, re.M)
    assert m and int(m.group(1)) == L.MSHA_ROUTE_LONG_BLOCKS_DEFAULT
    m = re.search(r"^#define MSHA_ROUTE_LONG_BYTES_DEFAULT \((\d+)ull << (\d+)\)\s*$", text, re.M)
    assert m and int(m.group(1)) << int(m.group(2)) == L.MSHA_ROUTE_LONG_BYTES_DEFAULT
    for name in ("MSHA_HAS_PARTS_PLANNED", "MSHA_HAS_PARTS_CONCAT", "MSHA_HAS_PARTS_DEVICE"):
        assert re.search(r"^#define %s 1\s*$" % name, text, re.M)


def test_mirrors_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\n'
                   '#if !defined(MSHA_HAS_PARTS_ROUTED) || MSHA_HAS_PARTS_ROUTED != 1\n#error not defined\n#endif\n'
                   'int main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(msha_route_opts),\n'
                   '       offsetof(msha_route_opts, long_bytes), sizeof(msha_parts_route_stats),\n'
                   '       offsetof(msha_parts_route_stats, last_kernel_ms), sizeof(msha_parts_plan_stats),\n'
                   '       sizeof(msha_concat_stats), sizeof(msha_parts_stats), sizeof(msha_stats));\n'
                   'return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(exe)], check=True)
    osize, olast, size, last, plan, concat, parts, stats = map(
        int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(L.MshaRouteOpts) == osize == 16 and L.MshaRouteOpts.long_bytes.offset == olast == 8
    assert [f for f, _ in L.MshaRouteOpts._fields_] == ["long_blocks", "max_long", "long_bytes"]
    assert ctypes.sizeof(L.MshaPartsRouteStats) == size == 104
    assert L.MshaPartsRouteStats.last_kernel_ms.offset == last == 96
    assert [f for f, _ in L.MshaPartsRouteStats._fields_] == [
        "calls", "actions", "lists", "launches_plan", "launches_copy", "launches_chain", "launches_hash",
        "launches_fill", "last_lanes", "last_blocks", "last_routed", "last_routed_bytes", "last_kernel_ms"]
    # the structs that were there are as they were
    assert (plan, concat, parts, stats) == (72, 40, 40, 192)
    assert ctypes.sizeof(L.MshaPartsPlanStats) == 72 and ctypes.sizeof(L.MshaConcatStats) == 40
    assert ctypes.sizeof(L.MshaStats) == 192


def test_bad_args_rejected_without_gpu():
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    f = lib.msha_hash_actions_device_routed
    assert f(None, None, None, None, None, 1, None, 1, None, None, None) == bad
    assert f(None, None, None, None, None, 0, None, 0, None, None, None) == bad
    o = L.MshaRouteOpts(4, 1, 79)
    assert f(None, None, None, None, None, 1, None, 1, ctypes.byref(o), None, None) == bad
    assert lib.msha_get_parts_route_stats(None, None) == bad
    s = L.MshaPartsRouteStats()
    assert lib.msha_get_parts_route_stats(None, ctypes.byref(s)) == bad
    n, b = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert lib.msha_parts_route_read(None, None, 0, ctypes.byref(n), ctypes.byref(b)) == bad
    assert lib.msha_parts_route_read(None, None, 0, None, None) == bad
    assert lib.msha_parts_route_read_order(None, None, 0, ctypes.byref(n)) == bad
    assert lib.msha_parts_route_read_order(None, None, 0, None) == bad


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


def test_routed_rejects_a_wrong_device(eng_no_call):
    arena, po, pl, begin, out = _good()           # host tensors
    with pytest.raises(ValueError, match="cuda:0"):
        eng_no_call.hash_actions_device_routed(arena, po, pl, begin, out)


def test_routed_validates_before_the_call(eng_no_call, monkeypatch):
    """The argument checks of hash_actions_device_planned, and the three options' ranges.
    There is no GPU here, so host tensors are made to report the context's device."""
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    eng = eng_no_call
    arena, po, pl, begin, out = _good()
    called = "msha_hash_actions_device_routed called"
    with pytest.raises(AssertionError, match=called):
        eng.hash_actions_device_routed(arena, po, pl, begin, out)       # the good calls are the only ones that get through
    al = torch.tensor([1, 0, 1, 1], dtype=torch.int32)
    with pytest.raises(AssertionError, match=called):
        eng.hash_actions_device_routed(arena, po, pl, begin, torch.zeros((4, 32), dtype=torch.uint8), action_list=al,
                                       long_blocks=4, max_long=2, long_bytes=4096)
    with pytest.raises(ValueError, match="part_off must hold 8-byte"):
        eng.hash_actions_device_routed(arena, po.int(), pl, begin, out)
    with pytest.raises(ValueError, match="list_begin must hold 8-byte"):
        eng.hash_actions_device_routed(arena, po, pl, begin.int(), out)
    with pytest.raises(ValueError, match="action_list must hold 4-byte"):
        eng.hash_actions_device_routed(arena, po, pl, begin, out, action_list=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="action_list has 3 entries, expected 2"):
        eng.hash_actions_device_routed(arena, po, pl, begin, out, action_list=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="list_begin has 4 entries, expected 3"):
        eng.hash_actions_device_routed(arena, po, pl, torch.tensor([0, 1, 2, 3]), out)
    with pytest.raises(ValueError, match="not a multiple of 32"):
        eng.hash_actions_device_routed(arena, po, pl, begin, out.view(-1)[:63])
    with pytest.raises(ValueError, match="part_len has 2 entries"):
        eng.hash_actions_device_routed(arena, po, pl[:2], begin, out)
    with pytest.raises(ValueError, match="contiguous"):
        eng.hash_actions_device_routed(arena, po, pl, begin, torch.zeros((2, 64), dtype=torch.uint8)[:, :32])
    with pytest.raises(ValueError, match="16-byte boundary"):
        eng.hash_actions_device_routed(arena[1:], po, pl, begin, out)
    with pytest.raises(ValueError, match="long_blocks must be in"):
        eng.hash_actions_device_routed(arena, po, pl, begin, out, long_blocks=-1)
    with pytest.raises(ValueError, match="max_long must be in"):
        eng.hash_actions_device_routed(arena, po, pl, begin, out, max_long=1 << 32)
    with pytest.raises(ValueError, match="long_bytes must be in"):
        eng.hash_actions_device_routed(arena, po, pl, begin, out, long_bytes=1 << 64)


def test_engine_has_the_methods():
    from mirbft_amd.engine import Engine
    assert callable(Engine.hash_actions_device_routed) and callable(Engine.parts_route_stats)
    assert callable(Engine.parts_route_lists) and callable(Engine.parts_route_order)
