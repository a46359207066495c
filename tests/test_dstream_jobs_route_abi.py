"""The C ABI and the Python surface of msha_dstreams_write_jobs_routed_device, as far as
they can be checked without a GPU: the define, exports and bindings, argument checks that
come before any device work, the new stats struct's layout against a compiled C program,
every older struct's size, DeviceStreamSet's validation, and the new header in both build
lists."""
import ctypes
import inspect
import os
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["msha_dstreams_write_jobs_routed_device", "msha_dstreams_get_jobs_route_stats",
           "msha_dstreams_jobs_route_read"]
FIELDS = ["calls", "jobs", "launches_sort", "launches_rows", "launches_route", "launches_copy", "launches_chain",
          "launches_tail", "launches_write", "last_passes", "last_jobs", "last_routed", "last_routed_bytes",
          "last_kernel_ms"]


def test_symbols_declared_bound_and_exported():
    assert L.MSHA_HAS_STREAMS_DEVICE_JOBS_ROUTED == 1 and L.ABI_VERSION == 10
    header = open(L.HEADER_PATH).read()
    assert "#define MSHA_HAS_STREAMS_DEVICE_JOBS_ROUTED 1" in header
    assert "#define MSHA_ABI_VERSION 10u" in header and L.lib().msha_abi_version() == 10
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = set(L.header_symbols())
    for s in SYMBOLS:
        assert s in declared and s in L.SIGNATURES and s in exported, s
        assert hasattr(L.lib(), s), s
    # the jobs entry's arguments with the routed write's opts before the stream
    jobs, routed = L.SIGNATURES["msha_dstreams_write_jobs_device"], L.SIGNATURES["msha_dstreams_write_routed_device"]
    new = L.SIGNATURES["msha_dstreams_write_jobs_routed_device"]
    assert new[0] == jobs[0] and new[1] == jobs[1][:-1] + routed[1][-2:]


def test_the_new_header_is_in_both_build_lists():
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "Makefile")).read()
    assert "stream_jobs_route.hpp" in L._SRC_FILES and "stream_jobs_route.hpp" in text.split("SRC_ID")[0]
    # stream_device.o is rebuilt when the header changes: the compiler lists each object's
    # headers beside it (-MMD), the Makefile includes those lists, and the one the build
    # left for stream_device.o names the header
    assert "-MMD" in text.split("$(BUILD)/%.o: %.cpp")[1].split("\n\n")[0]
    assert "-include $(wildcard $(BUILD)/*.d)" in text
    assert "stream_jobs_route.hpp" in open(os.path.join(ROOT, "mirbft_amd", "csrc", "stream_device.d")).read()
    assert os.path.exists(os.path.join(ROOT, "mirbft_amd", "csrc", "stream_jobs_route.hpp"))
    # the Makefile's order is the binding's: the build id is a hash over the files in it
    srcs = text.split("SRCS :=")[1].split("SRC_ID")[0].replace("\\", " ").split()
    assert [os.path.basename(f) for f in srcs] == [os.path.basename(f) for f in L._SRC_FILES]


def test_null_and_bad_arguments_rejected_without_a_gpu():
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    assert lib.msha_dstreams_write_jobs_routed_device(None, None, None, None, None, 1, None, None) == bad
    assert lib.msha_dstreams_write_jobs_routed_device(None, None, None, None, None, 0, None, None) == bad
    opts = L.MshaRouteOpts(2, 4, 4096)
    assert lib.msha_dstreams_write_jobs_routed_device(None, None, None, None, None, 1, ctypes.byref(opts), None) == bad
    st = L.MshaDstreamsJobsRouteStats()
    assert lib.msha_dstreams_get_jobs_route_stats(None, ctypes.byref(st)) == bad
    assert lib.msha_dstreams_get_jobs_route_stats(None, None) == bad
    n = ctypes.c_uint64(7)
    p = ctypes.byref(n)
    assert lib.msha_dstreams_jobs_route_read(None, None, 0, p, p, None, 0, p, p) == bad
    assert n.value == 7


def test_stats_struct_matches_the_header(tmp_path):
    assert [name for name, _ in L.MshaDstreamsJobsRouteStats._fields_] == FIELDS
    olds = {"msha_dstreams_stats": L.MshaDstreamsStats, "msha_dstreams_jobs_stats": L.MshaDstreamsJobsStats,
            "msha_dstreams_route_stats": L.MshaDstreamsRouteStats, "msha_stats": L.MshaStats,
            "msha_parts_route_stats": L.MshaPartsRouteStats, "msha_route_opts": L.MshaRouteOpts,
            "msha_streams_stats": L.MshaStreamsStats, "msha_parts_stats": L.MshaPartsStats,
            "msha_parts_plan_stats": L.MshaPartsPlanStats, "msha_concat_stats": L.MshaConcatStats}
    body = 'printf("size %zu\\n", sizeof(msha_dstreams_jobs_route_stats));\n'
    body += "".join('printf("old_%s %%zu\\n", sizeof(%s));\n' % (k, k) for k in olds)
    body += "".join('printf("%s %%zu\\n", offsetof(msha_dstreams_jobs_route_stats, %s));\n' % (f, f) for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n%s return 0;\n}\n'
                   % body)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines() if line)
    assert ctypes.sizeof(L.MshaDstreamsJobsRouteStats) == int(got.pop("size")) == 112       # thirteen u64 and a double
    want_old = {"msha_dstreams_stats": 56, "msha_dstreams_jobs_stats": 72, "msha_dstreams_route_stats": 80,
                "msha_stats": 192, "msha_parts_route_stats": 104, "msha_route_opts": 16, "msha_streams_stats": 88,
                "msha_parts_stats": 40, "msha_parts_plan_stats": 72, "msha_concat_stats": 40}
    for k, cls in olds.items():
        assert int(got.pop("old_" + k)) == ctypes.sizeof(cls) == want_old[k], k      # the older structs are as they were
    assert list(got) == FIELDS
    for i, f in enumerate(FIELDS):
        assert getattr(L.MshaDstreamsJobsRouteStats, f).offset == int(got[f]) == 8 * i, f


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


def test_write_jobs_routed_device_validates_before_the_call():
    import torch
    from mirbft_amd.streams_device import DeviceStreamSet
    sig = inspect.signature(DeviceStreamSet.write_jobs_routed_device)
    assert list(sig.parameters) == ["self", "arena", "job_stream", "job_off", "job_len", "stream", "long_blocks",
                                    "max_long", "long_bytes"]
    assert [sig.parameters[p].default for p in ("stream", "long_blocks", "max_long", "long_bytes")] == [None, 0, 0, 0]
    assert hasattr(DeviceStreamSet, "jobs_route_stats") and hasattr(DeviceStreamSet, "jobs_route_read")
    s = _unopened_set()
    arena = torch.zeros(128, dtype=torch.uint8)
    i32 = torch.zeros(3, dtype=torch.int32)
    i64 = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="cuda:0"):                          # wrong device
        s.write_jobs_routed_device(arena, i32, i64, i64)
    with pytest.raises(ValueError, match="cuda:0"):                          # not a tensor at all
        s.write_jobs_routed_device(arena, [0, 1, 0], i64, i64)

    class Dev:
        type, index = "cuda", 0

    class Fake(torch.Tensor):
        @property
        def device(self):
            return Dev

    def fake(t):
        return t.as_subclass(Fake)

    good = dict(arena=fake(arena), job_stream=fake(i32), job_off=fake(i64), job_len=fake(i64))
    # write_jobs_device's tensor validation
    with pytest.raises(ValueError, match="job_stream must hold 4-byte integers"):
        s.write_jobs_routed_device(**{**good, "job_stream": fake(i64)})
    with pytest.raises(ValueError, match="job_stream must hold 4-byte integers"):
        s.write_jobs_routed_device(**{**good, "job_stream": fake(i32.float())})
    with pytest.raises(ValueError, match="job_off must hold 8-byte integers"):
        s.write_jobs_routed_device(**{**good, "job_off": fake(i32)})
    with pytest.raises(ValueError, match="job_len must hold 8-byte integers"):
        s.write_jobs_routed_device(**{**good, "job_len": fake(i64.double())})
    with pytest.raises(ValueError, match="arena must hold 1-byte integers"):
        s.write_jobs_routed_device(**{**good, "arena": fake(i64)})
    with pytest.raises(ValueError, match="job_off must be contiguous"):
        s.write_jobs_routed_device(**{**good, "job_off": fake(torch.zeros(6, dtype=torch.int64)[::2])})
    with pytest.raises(ValueError, match="job_stream has 3 entries, job_off 2, job_len 3"):
        s.write_jobs_routed_device(**{**good, "job_off": fake(i64[:2])})
    with pytest.raises(ValueError, match="job_stream has 3 entries, job_off 3, job_len 4"):
        s.write_jobs_routed_device(**{**good, "job_len": fake(torch.zeros(4, dtype=torch.int64))})
    with pytest.raises(ValueError, match="16-byte boundary"):
        s.write_jobs_routed_device(**{**good, "arena": fake(torch.zeros(256, dtype=torch.uint8)[1:])})
    # write_routed_device's opts validation
    for name, v in (("long_blocks", 1 << 32), ("long_blocks", -1), ("max_long", -1), ("max_long", 1 << 32),
                    ("long_bytes", 1 << 64), ("long_bytes", -1)):
        with pytest.raises(ValueError, match=name):
            s.write_jobs_routed_device(**good, **{name: v})
    # no jobs: nothing is called (the set has no library behind it), whatever valid opts say
    s.write_jobs_routed_device(fake(arena), fake(i32[:0]), fake(i64[:0]), fake(i64[:0]), long_blocks=3, max_long=1)
