"""The stream-set additions to the C ABI (include/mirsha.h "Stream sets"): every new
symbol exported and bound, the exported-state size, the ABI version unchanged, the
msha_streams_stats mirror laid out as the header's struct, and null arguments
rejected without a GPU. No compute calls here (CPU suite)."""
import ctypes
import os
import re
import subprocess

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["msha_streams_create", "msha_streams_destroy", "msha_streams_write", "msha_streams_sum",
               "msha_streams_reset", "msha_streams_length", "msha_streams_export", "msha_streams_import",
               "msha_streams_get_stats", "msha_absorb_device", "msha_finish_device"]


def test_stream_symbols_declared_exported_and_bound():
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
    assert re.search(r"^#define MSHA_HAS_STREAMS 1\s*$", text, re.M)
    m = re.search(r"^#define MSHA_STREAM_STATE_BYTES (\d+)u\s*$", text, re.M)
    assert m and int(m.group(1)) == 108 == L.MSHA_STREAM_STATE_BYTES
    assert 4 + 8 * 4 + 64 + 8 == 108      # magic, state words, buffer, length
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10


def test_streams_stats_mirror_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %u\\n", sizeof(msha_streams_stats), offsetof(msha_streams_stats, last_kernel_ms),\n'
                   '       offsetof(msha_streams_stats, last_load_mode), (unsigned)MSHA_STREAM_STATE_BYTES);\n'
                   'return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    size, last, mode, state = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                                      check=True).stdout.split())
    assert ctypes.sizeof(L.MshaStreamsStats) == size
    assert L.MshaStreamsStats.last_kernel_ms.offset == last
    assert L.MshaStreamsStats.last_load_mode.offset == mode
    assert state == 108
    # the existing structs keep their layout (tests/test_abi.py pins them too)
    assert ctypes.sizeof(L.MshaStats) == 8 * 24 and ctypes.sizeof(L.MshaShardStats) == 8 * 15


def test_null_args_rejected_without_gpu():
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    assert lib.msha_streams_create(None, 4, 0, ctypes.byref(h)) == bad and h.value is None
    assert lib.msha_streams_create(None, 4, 0, None) == bad
    lib.msha_streams_destroy(None)                      # a no-op
    assert lib.msha_streams_write(None, None, 0, None, None, None, 0) == bad
    assert lib.msha_streams_sum(None, None, 0, None) == bad
    assert lib.msha_streams_reset(None, None, 0) == bad
    assert lib.msha_streams_length(None, None, 0, None) == bad
    assert lib.msha_streams_export(None, None, 0, None) == bad
    assert lib.msha_streams_import(None, None, 0, None) == bad
    assert lib.msha_streams_get_stats(None, None) == bad
    assert lib.msha_absorb_device(None, None, None, None, None, 1, None) == bad
    assert lib.msha_finish_device(None, None, None, None, None, None, 1, None, None) == bad


def test_engine_device_forms_validate_tensors_before_the_call():
    """absorb_device / finish_device take raw device pointers: a tensor off the GPU
    raises before anything reaches the C ABI (as the other *_device calls do)."""
    import pytest
    import torch
    from mirbft_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng._dev_index = 0
    eng._ctx = None

    class NoCall:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")
    eng._lib = NoCall()
    arena = torch.zeros(128, dtype=torch.uint8)
    off = torch.zeros(2, dtype=torch.int64)
    state = torch.zeros((2, 8), dtype=torch.int32)
    out = torch.zeros((2, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda:0"):
        eng.absorb_device(state, arena, off, off)
    with pytest.raises(ValueError, match="cuda:0"):
        eng.finish_device(None, None, arena, off, off, out)


def test_package_exports_stream_set():
    import mirbft_amd
    assert "StreamSet" in mirbft_amd.__all__ and hasattr(mirbft_amd.GPUHasher, "new_streams")
    assert mirbft_amd.StreamSet.stream and mirbft_amd.StreamSet.write_packed
