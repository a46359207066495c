"""The C ABI and the Python surface of msha_dstreams_write_jobs_device, as far as they can
be checked without a GPU: exports, argument checks that come before any device work,
the stats struct's layout, and DeviceStreamSet's tensor validation."""
import ctypes
import os
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["msha_dstreams_write_jobs_device", "msha_dstreams_get_jobs_stats", "msha_dstreams_jobs_read_order"]


def test_symbols_declared_bound_and_exported():
    assert L.MSHA_HAS_STREAMS_DEVICE_JOBS == 1 and L.ABI_VERSION == 10
    header = open(L.HEADER_PATH).read()
    assert "#define MSHA_HAS_STREAMS_DEVICE_JOBS 1" in header and "#define MSHA_ABI_VERSION 10u" in header
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = set(L.header_symbols())
    for s in SYMBOLS:
        assert s in declared and s in L.SIGNATURES and s in exported, s
        assert hasattr(L.lib(), s), s


def test_sources_are_in_both_build_lists():
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "Makefile")).read()
    for f in ("stream_jobs.hpp", "stream_jobs.hip"):
        assert f in L._SRC_FILES and f in text.split("SRC_ID")[0]
    assert "stream_jobs_kernels.o" in text.split("$(OUT):")[1]


def test_null_and_bad_arguments_rejected_without_a_gpu():
    lib = L.lib()
    assert lib.msha_dstreams_write_jobs_device(None, None, None, None, None, 1, None) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_write_jobs_device(None, None, None, None, None, 0, None) == L.MSHA_ERR_INVALID_ARG
    st = L.MshaDstreamsJobsStats()
    assert lib.msha_dstreams_get_jobs_stats(None, ctypes.byref(st)) == L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_get_jobs_stats(None, None) == L.MSHA_ERR_INVALID_ARG
    n = ctypes.c_uint64(7)
    assert lib.msha_dstreams_jobs_read_order(None, None, 0, ctypes.byref(n), ctypes.byref(n)) == L.MSHA_ERR_INVALID_ARG
    assert n.value == 7


def test_stats_struct_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    fields = [name for name, _ in L.MshaDstreamsJobsStats._fields_]
    assert fields == ["calls", "jobs", "launches_sort", "launches_rows", "launches_write", "last_passes", "last_jobs",
                      "tile_jobs", "last_kernel_ms"]
    body = ('printf("size %zu\\n", sizeof(msha_dstreams_jobs_stats));\n'
            'printf("old %zu\\n", sizeof(msha_dstreams_stats));\n') + "".join(
        'printf("%s %%zu\\n", offsetof(msha_dstreams_jobs_stats, %s));\n' % (f, f) for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n%s return 0;\n}\n'
                   % body)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines() if line)
    assert ctypes.sizeof(L.MshaDstreamsJobsStats) == int(got.pop("size")) == 72
    assert int(got.pop("old")) == ctypes.sizeof(L.MshaDstreamsStats) == 56      # the older counters are as they were
    assert list(got) == fields
    for f in fields:
        assert getattr(L.MshaDstreamsJobsStats, f).offset == int(got[f]), f


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


def test_write_jobs_device_validates_tensors_before_the_call():
    import torch
    s = _unopened_set()
    arena = torch.zeros(128, dtype=torch.uint8)
    i32 = torch.zeros(3, dtype=torch.int32)
    i64 = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="cuda:0"):                          # wrong device
        s.write_jobs_device(arena, i32, i64, i64)
    with pytest.raises(ValueError, match="cuda:0"):                          # not a tensor at all
        s.write_jobs_device(arena, [0, 1, 0], i64, i64)

    class Dev:
        type, index = "cuda", 0

    class Fake(torch.Tensor):
        @property
        def device(self):
            return Dev

    def fake(t):
        return t.as_subclass(Fake)

    good = dict(arena=fake(arena), job_stream=fake(i32), job_off=fake(i64), job_len=fake(i64))
    with pytest.raises(ValueError, match="job_stream must hold 4-byte integers"):
        s.write_jobs_device(**{**good, "job_stream": fake(i64)})
    with pytest.raises(ValueError, match="job_stream must hold 4-byte integers"):
        s.write_jobs_device(**{**good, "job_stream": fake(i32.float())})
    with pytest.raises(ValueError, match="job_off must hold 8-byte integers"):
        s.write_jobs_device(**{**good, "job_off": fake(i32)})
    with pytest.raises(ValueError, match="job_len must hold 8-byte integers"):
        s.write_jobs_device(**{**good, "job_len": fake(i64.double())})
    with pytest.raises(ValueError, match="arena must hold 1-byte integers"):
        s.write_jobs_device(**{**good, "arena": fake(i64)})
    with pytest.raises(ValueError, match="job_off must be contiguous"):
        s.write_jobs_device(**{**good, "job_off": fake(torch.zeros(6, dtype=torch.int64)[::2])})
    with pytest.raises(ValueError, match="job_stream has 3 entries, job_off 2, job_len 3"):
        s.write_jobs_device(**{**good, "job_off": fake(i64[:2])})
    with pytest.raises(ValueError, match="job_stream has 3 entries, job_off 3, job_len 4"):
        s.write_jobs_device(**{**good, "job_len": fake(torch.zeros(4, dtype=torch.int64))})
    with pytest.raises(ValueError, match="16-byte boundary"):
        s.write_jobs_device(**{**good, "arena": fake(torch.zeros(256, dtype=torch.uint8)[1:])})
    # no jobs: nothing is called (the set has no library behind it)
    s.write_jobs_device(fake(arena), fake(i32[:0]), fake(i64[:0]), fake(i64[:0]))
