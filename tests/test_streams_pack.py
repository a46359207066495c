"""The write planner of the stream sets (mirbft_amd/csrc/stream_pack.hpp: grouping by
stream, packing whole blocks into bounded staging pieces, new tails and lengths) under
AddressSanitizer + UBSan, as a stand-alone program with its own main
(tests/cpp/stream_pack_check.cpp). Host code only: nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_pack_under_asan_ubsan(tmp_path):
    exe = tmp_path / "stream_pack_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "stream_pack_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "stream_pack ok" in r.stdout
