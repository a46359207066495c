"""The device digest maps in the C ABI (include/mirsha.h "Device digest maps"): the new
symbols declared, exported and bound, MSHA_HAS_DIGEST_MAP, the ABI version still 10, the
two struct mirrors laid out as the header's, the build lists naming the three new files,
null handles rejected without a GPU, and DeviceDigestMap refusing bad tensors before
anything reaches C. No compute calls here (CPU suite)."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_dmap_create", "msha_dmap_destroy", "msha_dmap_add_device", "msha_dmap_find_device",
               "msha_dmap_clear_device", "msha_dmap_size", "msha_dmap_read", "msha_dmap_get_stats"]
NEW_FILES = ["dmap.hpp", "dmap.hip", "dmap.cpp"]
RESULT_FIELDS = ["n", "entries", "added", "full", "crossed", "listed", "max_count", "max_id"]
STATS_FIELDS = ["adds", "finds", "clears", "digests", "launches", "capacity", "last_kernel_ms"]


def test_dmap_symbols_declared_exported_and_bound():
    declared = set(L.header_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    lib = L.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in exported, s
        assert s in L.SIGNATURES and hasattr(lib, s), s
    assert len(L.SIGNATURES["msha_dmap_add_device"][1]) == 12
    assert len(L.SIGNATURES["msha_dmap_find_device"][1]) == 7
    assert len(L.SIGNATURES["msha_dmap_read"][1]) == 6


def test_header_constants_and_abi_version():
    text = open(L.HEADER_PATH).read()
    assert re.search(r"^#define MSHA_HAS_DIGEST_MAP 1\s*$", text, re.M) and L.MSHA_HAS_DIGEST_MAP == 1
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    # the reference sites the contract cites, and what it rules out
    section = text[text.index("Device digest maps (ABI 10"):text.index("#define MSHA_HAS_DIGEST_MAP")]
    for site in ("sequence.go:73-74, 271-277, 331-340", "checkpoints.go:264-290",
                 "client_hash_disseminator.go:346-349, 415-504"):
        assert site in section, site
    for word in ("no erase", "tombstones", "FULL: ALL OR NOTHING", "CANONICAL", "MSHA_DMAP_SEED", "MSHA_DMAP_FORCE_HOME"):
        assert word in section, word


def test_struct_mirrors_match_the_header(tmp_path):
    src = tmp_path / "layout.c"
    res_off = ", ".join("offsetof(msha_dmap_result, %s)" % f for f in RESULT_FIELDS)
    st_off = ", ".join("offsetof(msha_dmap_stats, %s)" % f for f in STATS_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'size_t a[] = {sizeof(msha_dmap_result), %s};\n'
                   'size_t b[] = {sizeof(msha_dmap_stats), %s};\n'
                   'for (unsigned i = 0; i < sizeof a / sizeof *a; ++i) printf("%%zu ", a[i]);\nprintf("\\n");\n'
                   'for (unsigned i = 0; i < sizeof b / sizeof *b; ++i) printf("%%zu ", b[i]);\nprintf("\\n");\n'
                   'printf("%%zu %%zu %%zu\\n", sizeof(msha_group_result), sizeof(msha_group_stats), sizeof(msha_stats));\n'
                   'return MSHA_HAS_DIGEST_MAP == 1 ? 0 : 1;\n}\n' % (res_off, st_off))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    res, st, old = (list(map(int, ln.split())) for ln in
                    subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [f for f, _ in L.MshaDmapResult._fields_] == RESULT_FIELDS
    assert res == [64] + list(range(0, 64, 8)) == [ctypes.sizeof(L.MshaDmapResult)] + [
        getattr(L.MshaDmapResult, f).offset for f in RESULT_FIELDS]
    assert all(t is ctypes.c_uint64 for _, t in L.MshaDmapResult._fields_)
    assert [f for f, _ in L.MshaDmapStats._fields_] == STATS_FIELDS
    assert st == [56] + list(range(0, 56, 8)) == [ctypes.sizeof(L.MshaDmapStats)] + [
        getattr(L.MshaDmapStats, f).offset for f in STATS_FIELDS]
    assert L.MshaDmapStats._fields_[-1][1] is ctypes.c_double
    # the older structs are as they were
    assert old == [40, 40, 192] == [ctypes.sizeof(L.MshaGroupResult), ctypes.sizeof(L.MshaGroupStats),
                                    ctypes.sizeof(L.MshaStats)]


def test_build_lists_name_the_new_files():
    """The Makefile's SRCS and _lib._SRC_FILES name the same files in the same order
    (msha_build_id depends on it), the three new ones included, DmapArgs is in
    kernels.hpp, and the library is the tree's build."""
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*?)\n(?!\s)", text, re.M | re.S).group(1).replace("\\\n", " ").split()
    assert srcs == [f.replace(os.sep, "/") for f in L._SRC_FILES]
    for f in NEW_FILES:
        assert srcs.count(f) == 1 and os.path.exists(os.path.join(ROOT, "mirbft_amd", "csrc", f)), f
    assert "$(BUILD)/dmap_kernels.o" in text and "$(BUILD)/dmap.o" in text
    assert "struct DmapArgs {" in open(os.path.join(ROOT, "mirbft_amd", "csrc", "kernels.hpp")).read()
    assert L.build_id()["matches_tree"]


def test_bad_args_rejected_without_gpu():
    """A null context or a null map is refused whatever else is passed. (With a map each
    refusal has its own message: tests/test_gpu_dmap.py.)"""
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    assert lib.msha_dmap_create(None, 16, ctypes.byref(h)) == bad and not h.value
    assert lib.msha_dmap_create(None, 16, None) == bad
    assert lib.msha_dmap_add_device(None, None, 1, None, 0, None, None, None, None, 0, None, None) == bad
    assert lib.msha_dmap_add_device(None, None, 0, None, 0, None, None, None, None, 0, None, None) == bad
    assert lib.msha_dmap_find_device(None, None, 1, None, None, None, None) == bad
    assert lib.msha_dmap_clear_device(None, None) == bad
    e = ctypes.c_uint64(7)
    assert lib.msha_dmap_size(None, ctypes.byref(e)) == bad and e.value == 7
    assert lib.msha_dmap_read(None, 0, 0, None, None, None) == bad
    s = L.MshaDmapStats()
    assert lib.msha_dmap_get_stats(None, ctypes.byref(s)) == bad
    lib.msha_dmap_destroy(None)                               # as free(NULL)


@pytest.fixture
def map_no_call():
    """A DeviceDigestMap with no context behind it: validation runs before any C call."""
    from mirbft_amd.digest_map import DeviceDigestMap
    from mirbft_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng._dev_index = 0
    eng._ctx = None

    class NoCall:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    eng._lib = NoCall()
    m = DeviceDigestMap.__new__(DeviceDigestMap)
    m._engine, m._lib, m.max_keys, m._h = eng, eng._lib, 16, ctypes.c_void_p(1)
    yield m
    m._h = None


def _good(n=70):
    import torch
    digests = torch.zeros(32 * n, dtype=torch.uint8)
    assert digests.data_ptr() % 16 == 0
    return digests, torch.zeros(n, dtype=torch.int32), torch.zeros(8, dtype=torch.int64)


def test_map_rejects_a_wrong_device(map_no_call):
    dig, ids, res = _good()
    with pytest.raises(ValueError, match="cuda:0"):
        map_no_call.add_device(dig, ids, res)                # host tensors
    with pytest.raises(ValueError, match="cuda:0"):
        map_no_call.find_device(dig, ids)


def test_map_validates_tensors_before_the_call(map_no_call, monkeypatch):
    """Wrong dtype or length, rows that are not 32 bytes, a short result, a misaligned
    table: each raises before the C call. There is no GPU here, so host tensors are made
    to report the context's device; every other property checked is their own."""
    import torch
    monkeypatch.setattr(torch.Tensor, "device", property(lambda self: torch.device("cuda", 0)), raising=False)
    m = map_no_call
    dig, ids, res = _good()
    i32 = lambda k: torch.zeros(k, dtype=torch.int32)                      # noqa: E731
    with pytest.raises(AssertionError, match="msha_dmap_add_device called"):
        m.add_device(dig, ids, res)                          # the good calls are the only ones that get through
    with pytest.raises(AssertionError, match="msha_dmap_add_device called"):
        m.add_device(dig, ids, res, scope=i32(70), threshold=3, before=i32(70), after=i32(70), crossed_slots=i32(4))
    with pytest.raises(AssertionError, match="msha_dmap_find_device called"):
        m.find_device(dig, ids, scope=i32(70), count=i32(70))
    with pytest.raises(AssertionError, match="msha_dmap_clear_device called"):
        m.clear_device()
    m.add_device(dig[:0], ids[:0], res)                      # nothing to add: no call
    m.find_device(dig[:0], ids[:0])
    with pytest.raises(ValueError, match="digests must hold 1-byte"):
        m.add_device(dig.view(torch.int32), ids, res)
    with pytest.raises(ValueError, match="ids must hold 4-byte"):
        m.add_device(dig, ids.long(), res)
    with pytest.raises(ValueError, match="scope must hold 4-byte"):
        m.add_device(dig, ids, res, scope=torch.zeros(70, dtype=torch.int64))
    with pytest.raises(ValueError, match="before must hold 4-byte"):
        m.add_device(dig, ids, res, before=torch.zeros(70, dtype=torch.float32))
    with pytest.raises(ValueError, match="result must hold 8-byte"):
        m.add_device(dig, ids, res.int())
    with pytest.raises(ValueError, match="result must hold 8 words"):
        m.add_device(dig, ids, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="32-byte rows"):
        m.add_device(dig[:-1], ids, res)
    with pytest.raises(ValueError, match="ids has 69 entries, expected 70"):
        m.add_device(dig, ids[:69], res)
    with pytest.raises(ValueError, match="scope has 71 entries"):
        m.add_device(dig, ids, res, scope=i32(71))
    with pytest.raises(ValueError, match="after has 1 entries"):
        m.add_device(dig, ids, res, after=i32(1))
    with pytest.raises(ValueError, match="threshold must fit 32 bits"):
        m.add_device(dig, ids, res, threshold=1 << 32)
    with pytest.raises(ValueError, match="contiguous"):
        m.add_device(torch.zeros((70, 64), dtype=torch.uint8)[:, :32], ids, res)
    with pytest.raises(ValueError, match="crossed_slots must be contiguous"):
        m.add_device(dig, ids, res, crossed_slots=i32(8)[::2])
    with pytest.raises(ValueError, match="digests must start on a 16-byte boundary"):
        m.add_device(torch.zeros(32 * 70 + 8, dtype=torch.uint8)[8:], ids, res)
    with pytest.raises(ValueError, match="count has 3 entries, expected 70"):
        m.find_device(dig, ids, count=i32(3))
    with pytest.raises(ValueError, match="count must hold 4-byte"):
        m.find_device(dig, ids, count=torch.zeros(70, dtype=torch.int16))
    with pytest.raises(ValueError, match="digests must start on a 16-byte boundary"):
        m.find_device(torch.zeros(32 * 70 + 8, dtype=torch.uint8)[8:], ids)
    from mirbft_amd import MshaError
    m._h = None
    with pytest.raises(MshaError, match="device digest map is closed"):
        m.add_device(dig, ids, res)


def test_package_has_the_map():
    import mirbft_amd
    from mirbft_amd import DeviceDigestMap, GPUHasher, tally_into_map_device
    assert "DeviceDigestMap" in mirbft_amd.__all__ and "tally_into_map_device" in mirbft_amd.__all__
    for name in ("add_device", "find_device", "clear_device", "size", "read", "stats", "close"):
        assert callable(getattr(DeviceDigestMap, name)), name
    assert list(inspect.signature(GPUHasher.new_device_digest_map).parameters) == ["self", "max_keys"]
    sig = inspect.signature(tally_into_map_device)
    assert list(sig.parameters) == ["dmap", "digests", "scope", "quorum", "crossed_cap", "stream"]
    assert (sig.parameters["quorum"].default, sig.parameters["crossed_cap"].default) == (0, 64)
