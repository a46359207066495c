"""The C ABI and the Python surface of msha_absorb_chain_device and
msha_dstreams_write_routed_device, as far as they can be checked without a GPU: the
defines, exports and bindings, argument checks that come before any device work, the new
stats struct's layout against a compiled C program, the older structs' sizes, and
DeviceStreamSet's validation."""
import ctypes
import os
import subprocess

import pytest

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["msha_absorb_chain_device", "msha_dstreams_write_routed_device", "msha_dstreams_get_route_stats",
           "msha_dstreams_route_read"]
FIELDS = ["calls", "rows", "launches_route", "launches_copy", "launches_chain", "launches_tail", "launches_write",
          "last_routed", "last_routed_bytes", "last_kernel_ms"]


def test_symbols_declared_bound_and_exported():
    assert L.MSHA_HAS_ABSORB_CHAIN == 1 and L.MSHA_HAS_STREAMS_DEVICE_ROUTED == 1 and L.ABI_VERSION == 10
    header = open(L.HEADER_PATH).read()
    assert "#define MSHA_HAS_ABSORB_CHAIN 1" in header and "#define MSHA_HAS_STREAMS_DEVICE_ROUTED 1" in header
    assert "#define MSHA_ABI_VERSION 10u" in header and L.lib().msha_abi_version() == 10
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    declared = set(L.header_symbols())
    for s in SYMBOLS:
        assert s in declared and s in L.SIGNATURES and s in exported, s
        assert hasattr(L.lib(), s), s
    assert L.SIGNATURES["msha_absorb_chain_device"] == L.SIGNATURES["msha_absorb_device"]   # the same contract


def test_sources_are_in_both_build_lists():
    text = open(os.path.join(ROOT, "mirbft_amd", "csrc", "Makefile")).read()
    for f in ("stream_chain.hpp", "stream_chain.hip", "stream_write.hpp"):
        assert f in L._SRC_FILES and f in text.split("SRC_ID")[0]
    assert "stream_chain_kernels.o" in text.split("$(OUT):")[1]


def test_null_and_bad_arguments_rejected_without_a_gpu():
    lib = L.lib()
    bad = L.MSHA_ERR_INVALID_ARG
    assert lib.msha_absorb_chain_device(None, None, None, None, None, 1, None) == bad
    assert lib.msha_absorb_chain_device(None, None, None, None, None, 0, None) == bad
    assert lib.msha_dstreams_write_routed_device(None, None, None, None, None, None, 1, None, None) == bad
    assert lib.msha_dstreams_write_routed_device(None, None, None, None, None, None, 0, None, None) == bad
    st = L.MshaDstreamsRouteStats()
    assert lib.msha_dstreams_get_route_stats(None, ctypes.byref(st)) == bad
    assert lib.msha_dstreams_get_route_stats(None, None) == bad
    n = ctypes.c_uint64(7)
    assert lib.msha_dstreams_route_read(None, None, 0, ctypes.byref(n), ctypes.byref(n)) == bad
    assert n.value == 7


def test_null_pointers_on_a_context_without_a_gpu():
    """A context without a device cannot exist here, so the pointer checks are reached only
    where one can be created; where none can, the creation's own error is the result."""
    lib = L.lib()
    ctx = ctypes.c_void_p()
    if lib.msha_ctx_create(1, ctypes.byref(ctx)) != L.MSHA_OK:
        return
    try:
        assert lib.msha_absorb_chain_device(ctx, None, None, None, None, 3, None) == L.MSHA_ERR_INVALID_ARG
        assert b"null pointer" in lib.msha_last_error(ctx)
        assert lib.msha_absorb_chain_device(ctx, None, None, None, None, 0, None) == L.MSHA_OK
    finally:
        lib.msha_ctx_destroy(ctx)


def test_stats_struct_matches_the_header(tmp_path):
    assert [name for name, _ in L.MshaDstreamsRouteStats._fields_] == FIELDS
    olds = {"msha_dstreams_stats": L.MshaDstreamsStats, "msha_dstreams_jobs_stats": L.MshaDstreamsJobsStats,
            "msha_stats": L.MshaStats, "msha_parts_route_stats": L.MshaPartsRouteStats,
            "msha_route_opts": L.MshaRouteOpts, "msha_streams_stats": L.MshaStreamsStats}
    body = 'printf("size %zu\\n", sizeof(msha_dstreams_route_stats));\n'
    body += "".join('printf("old_%s %%zu\\n", sizeof(%s));\n' % (k, k) for k in olds)
    body += "".join('printf("%s %%zu\\n", offsetof(msha_dstreams_route_stats, %s));\n' % (f, f) for f in FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n%s return 0;\n}\n'
                   % body)
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines() if line)
    assert ctypes.sizeof(L.MshaDstreamsRouteStats) == int(got.pop("size")) == 80
    want_old = {"msha_dstreams_stats": 56, "msha_dstreams_jobs_stats": 72, "msha_stats": 192,
                "msha_parts_route_stats": 104, "msha_route_opts": 16, "msha_streams_stats": 88}
    for k, cls in olds.items():
        assert int(got.pop("old_" + k)) == ctypes.sizeof(cls) == want_old[k], k      # the older structs are as they were
    assert list(got) == FIELDS
    for f in FIELDS:
        assert getattr(L.MshaDstreamsRouteStats, f).offset == int(got[f]), f


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


def test_write_routed_device_validates_before_the_call():
    import torch
    from mirbft_amd.engine import Engine
    assert hasattr(Engine, "absorb_chain_device")
    s = _unopened_set()
    arena = torch.zeros(128, dtype=torch.uint8)
    i64 = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(ValueError, match="cuda:0"):
        s.write_routed_device(arena, i64, i64, i64)

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
        s.write_routed_device(**{**good, "part_off": fake(i64.int())})
    with pytest.raises(ValueError, match="row_part_begin has 3 entries, expected 2"):
        s.write_routed_device(**good, rows=fake(torch.zeros(1, dtype=torch.int32)))
    with pytest.raises(ValueError, match="part_len has 2 entries, part_off 3"):
        s.write_routed_device(**{**good, "part_len": fake(i64[:2])})
    with pytest.raises(ValueError, match="16-byte boundary"):
        s.write_routed_device(**{**good, "arena": fake(torch.zeros(256, dtype=torch.uint8)[1:])})
    for name, v in (("long_blocks", 1 << 32), ("max_long", -1), ("long_bytes", 1 << 64)):
        with pytest.raises(ValueError, match=name):
            s.write_routed_device(**good, **{name: v})
    # no rows: nothing is called (the set has no library behind it)
    s.write_routed_device(fake(arena), fake(i64[:0]), fake(i64[:0]), fake(i64[:1]),
                          rows=fake(torch.zeros(0, dtype=torch.int32)))
