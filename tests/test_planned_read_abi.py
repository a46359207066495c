"""msha_planned_read_plan in the C ABI (include/mirsha.h "The plan of the last
msha_digest_batch_device_planned call"): the symbol declared, exported and bound,
MSHA_HAS_PLANNED_READ, the ABI version unchanged, the msha_planned_plan mirror laid out
as the header's struct, a header-only C probe of the macro, bad arguments rejected without
a GPU. No compute calls here (CPU suite)."""
import ctypes
import os
import re
import subprocess

from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["n", "folded", "lanes", "head", "early", "late", "long_lanes", "long_listed", "gate", "long_cap",
          "head_cap", "head_per_wg", "gave_up"]


def test_symbol_declared_exported_and_bound():
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    s = "msha_planned_read_plan"
    assert s in L.header_symbols()
    assert s in exported
    assert s in L.SIGNATURES and hasattr(L.lib(), s)
    from mirbft_amd.engine import Engine
    assert callable(Engine.planned_read_plan)


def test_header_constant_and_abi_version():
    text = open(L.HEADER_PATH).read()
    assert re.search(r"^#define MSHA_HAS_PLANNED_READ 1\s*$", text, re.M) and L.MSHA_HAS_PLANNED_READ == 1
    assert re.search(r"^#define MSHA_ABI_VERSION 10u\s*$", text, re.M)
    assert L.lib().msha_abi_version() == L.ABI_VERSION == 10
    assert ctypes.sizeof(L.MshaStats) == 192          # msha_stats is as it was


def test_struct_mirror_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mirsha.h"\nint main(void) {\n'
                   'printf("%zu", sizeof(msha_planned_plan));\n' +
                   "".join('printf(" %%zu", offsetof(msha_planned_plan, %s));\n' % f for f in FIELDS) +
                   'printf(" %zu\\n", sizeof(msha_stats));\nreturn 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    nums = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert ctypes.sizeof(L.MshaPlannedPlan) == nums[0] == 64
    assert [f for f, _ in L.MshaPlannedPlan._fields_] == FIELDS
    assert [getattr(L.MshaPlannedPlan, f).offset for f in FIELDS] == nums[1:-1]
    assert nums[1:-1] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56]
    assert nums[-1] == 192


def test_header_only_probe_compiles(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include "mirsha.h"\n'
                   '#if !defined(MSHA_HAS_PLANNED_READ) || MSHA_HAS_PLANNED_READ != 1\n#error not defined\n#endif\n'
                   'int main(void) {\n  msha_planned_plan p = {0};\n'
                   '  int (*f)(msha_ctx*, msha_planned_plan*, uint32_t*, uint64_t, uint32_t*, uint64_t) = 0;\n'
                   '  (void)f;\n  return (int)p.n + (MSHA_HAS_PLANNED_READ == 1 ? 0 : 1);\n}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    str(src), "-o", str(tmp_path / "probe")], check=True)
    assert subprocess.run([str(tmp_path / "probe")]).returncode == 0


def test_bad_args_rejected_without_gpu():
    """No context can exist here; a null context or a null out is refused whatever else
    is passed."""
    f = L.lib().msha_planned_read_plan
    p = L.MshaPlannedPlan()
    p.n = 7
    assert f(None, ctypes.byref(p), None, 0, None, 0) == L.MSHA_ERR_INVALID_ARG
    assert f(None, None, None, 0, None, 0) == L.MSHA_ERR_INVALID_ARG
    assert p.n == 7
