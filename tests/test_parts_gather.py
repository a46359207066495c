"""The parts gather (mirbft_amd/csrc/parts_gather.hpp: walking an action's parts, which
aligned 16-byte granules are read, masking by the part's bounds, shifting into the
block) under AddressSanitizer + UBSan, as a stand-alone program with its own main
(tests/cpp/parts_gather_check.cpp), over the boundary matrix the GPU test launches
(tests/parts_matrix.py). Host code only: nothing is loaded into Python."""
import hashlib
import os
import subprocess

import parts_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_boundary_matrix_is_what_it_says():
    arena, off, ln, begin, want, seen = parts_matrix.boundary_matrix()
    n = begin.size - 1
    assert n == 201 + sum(L + 1 for L in parts_matrix.EXHAUSTIVE) and want.shape == (n, 32)
    assert seen == set(range(16))                       # every start residue mod 16
    assert (ln == 0).any() and int(begin[-1]) == off.size
    counts = set(np_diff(begin))
    assert counts >= {0, 1, 2, 3, 4, 5, 6}
    for i in (0, 57, 200, 201, n - 1):                  # the expected digests are hashlib's of the join
        parts = [arena[int(off[j]): int(off[j]) + int(ln[j])].tobytes() for j in range(int(begin[i]), int(begin[i + 1]))]
        assert hashlib.sha256(b"".join(parts)).digest() == want[i].tobytes()
    assert arena.size >= int((off + ln).max()) + 64      # the slack the device contract asks for


def np_diff(begin):
    return [int(b) - int(a) for a, b in zip(begin, begin[1:])]


def test_epoch_change_pool_in_parts_form_and_scattered():
    """workloads.epoch_change_parts_pool is epoch_change_pool cut into the parts
    epochChangeHashData yields; scatter_parts keeps every action's bytes and puts the
    8-byte fields and the rest in two regions."""
    from mirbft_amd.workloads import epoch_change_parts_pool, epoch_change_pool, scatter_parts
    parts = epoch_change_parts_pool(count=4, max_set=30)
    assert [b"".join(m) for m in parts] == epoch_change_pool(count=4, max_set=30)
    assert all({len(p) for p in m} <= {8, 32, 332} for m in parts)
    arena, off, ln, begin = scatter_parts(parts, slack=64)
    assert begin.size == 5 and int(begin[-1]) == off.size == sum(len(m) for m in parts)
    for i, m in enumerate(parts):
        got = [arena[int(off[j]): int(off[j]) + int(ln[j])].tobytes() for j in range(int(begin[i]), int(begin[i + 1]))]
        assert got == m
    fields = off[ln == 8]
    assert int(fields.max()) + 8 <= int(off[ln != 8].min())      # two regions
    assert arena.size == int((off + ln).max()) + 64


def test_parts_gather_under_asan_ubsan(tmp_path):
    arena, off, ln, begin, _, _ = parts_matrix.boundary_matrix()
    batch = tmp_path / "matrix.bin"
    parts_matrix.write_batch(batch, arena, off, ln, begin)
    exe = tmp_path / "parts_gather_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "parts_gather_check.cpp")], check=True)
    r = subprocess.run([str(exe), str(batch)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "matrix: %d actions" % (begin.size - 1) in r.stdout
    assert "parts_gather ok" in r.stdout
