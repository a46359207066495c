"""The C ABI and the Python surface of the device stream sets (msha_dstreams_*), as far
as they can be checked without a GPU: exports, argument checks that come before any
device work, the stats struct's layout, and DeviceStreamSet's tensor validation."""
import ctypes
import os
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["msha_dstreams_create", "msha_dstreams_destroy", "msha_dstreams_write_device", "msha_dstreams_sum_device",
           "msha_dstreams_snap_device", "msha_dstreams_reset_device", "msha_dstreams_length", "msha_dstreams_export",
           "msha_dstreams_import", "msha_dstreams_get_stats"]


def test_symbols_declared_bound_and_exported():
    assert L.MSHA_HAS_STREAMS_DEVICE == 1 and L.ABI_VERSION == 10
    header = open(L.HEADER_PATH).read()
    assert "#define MSHA_HAS_STREAMS_DEVICE 1" in header
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = set(L.header_symbols())
    for s in SYMBOLS:
        assert s in declared and s in L.SIGNATURES and s in exported, s
        assert hasattr(L.lib(), s), s


def test_null_and_bad_arguments_rejected_without_a_gpu():
    lib = L.lib()
    h = ctypes.c_void_p(1234)
    assert lib.msha_dstreams_create(None, 4, ctypes.byref(h)) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_create(None, 4, None) == L.MSHA_ERR_INVALID_ARG
    lib.msha_dstreams_destroy(None)                                          # a no-op
    assert lib.msha_dstreams_write_device(None, None, None, None, None, None, 1, None) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_sum_device(None, None, 1, None, None) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_snap_device(None, None, 1, None, None) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_reset_device(None, None, 1, None) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_length(None, None, 0, None) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_export(None, None, 0, None) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_import(None, None, 0, None) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_get_stats(None, None) == L.MSHA_ERR_INVALID_ARG


def test_stats_struct_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    fields = [name for name, _ in L.MshaDstreamsStats._fields_]
    body = 'printf("size %zu\\n", sizeof(msha_dstreams_stats));\n' + "".join(
        'printf("%s %%zu\\n", offsetof(msha_dstreams_stats, %s));\n' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n%s return 0;\n}\n'
                   % body)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines() if line)
    assert ctypes.sizeof(L.MshaDstreamsStats) == int(got.pop("size")) == 56
    assert list(got) == fields
    for f in fields:
        assert getattr(L.MshaDstreamsStats, f).offset == int(got[f]), f


def _unopened_set():
    """A DeviceStreamSet with no context behind it: validation runs before any C call."""
    from mirbft_amd.engine import Engine
    from mirbft_amd.streams_device import DeviceStreamSet

    class NoCall:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")

    eng = Engine.__new__(Engine)
    eng._dev_index = 0
    eng._ctx = None
    eng._lib = NoCall()
    s = DeviceStreamSet.__new__(DeviceStreamSet)
    s._engine, s._lib, s.n, s._h = eng, eng._lib, 2, None
    return s


def test_device_stream_set_validates_tensors_before_the_call():
    import torch
    s = _unopened_set()
    arena = torch.zeros(128, dtype=torch.uint8)
    i64 = torch.zeros(3, dtype=torch.int64)
    out = torch.zeros((2, 32), dtype=torch.uint8)
    with pytest.raises(ValueError, match="cuda:0"):                          # wrong device
        s.write_device(arena, i64, i64, i64)
    with pytest.raises(ValueError, match="cuda:0"):
        s.sum_device(out)
    with pytest.raises(ValueError, match="cuda:0"):
        s.snap_device(out)
    with pytest.raises(ValueError, match="cuda:0"):
        s.reset_device(rows=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="cuda:0"):                          # not a tensor at all
        s.sum_device(bytearray(64))

    # the remaining checks, with the device check satisfied by tensors that claim cuda:0
    class Dev:
        type, index = "cuda", 0

    class Fake(torch.Tensor):
        @property
        def device(self):
            return Dev

    def fake(t):
        return t.as_subclass(Fake)

    good = dict(arena=fake(arena), part_off=fake(i64), part_len=fake(i64), row_part_begin=fake(i64))
    with pytest.raises(ValueError, match="part_off must hold 8-byte integers"):
        s.write_device(**{**good, "part_off": fake(i64.int())})
    with pytest.raises(ValueError, match="part_len must hold 8-byte integers"):
        s.write_device(**{**good, "part_len": fake(i64.double())})
    with pytest.raises(ValueError, match="rows must hold 4-byte integers"):
        s.write_device(**good, rows=fake(torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError, match="arena must hold 1-byte integers"):
        s.write_device(**{**good, "arena": fake(i64)})
    with pytest.raises(ValueError, match="row_part_begin must be contiguous"):
        s.write_device(**{**good, "row_part_begin": fake(torch.zeros(6, dtype=torch.int64)[::2])})
    with pytest.raises(ValueError, match="row_part_begin has 4 entries, expected 3"):
        s.write_device(**{**good, "row_part_begin": fake(torch.zeros(4, dtype=torch.int64))})
    with pytest.raises(ValueError, match="row_part_begin has 3 entries, expected 2"):
        s.write_device(**good, rows=fake(torch.zeros(1, dtype=torch.int32)))
    with pytest.raises(ValueError, match="part_len has 2 entries, part_off 3"):
        s.write_device(**{**good, "part_len": fake(i64[:2])})
    with pytest.raises(ValueError, match="16-byte boundary"):
        s.write_device(**{**good, "arena": fake(torch.zeros(256, dtype=torch.uint8)[1:])})
    with pytest.raises(ValueError, match="out holds 32 bytes, needs 64"):
        s.sum_device(fake(out[:1]))
    with pytest.raises(ValueError, match="out must be contiguous"):
        s.snap_device(fake(torch.zeros((2, 64), dtype=torch.uint8)[:, :32]))
    with pytest.raises(ValueError, match="out must hold 1-byte integers"):
        s.sum_device(fake(torch.zeros(64, dtype=torch.int16)))
