"""The grouping of msha_dstreams_write_jobs_device (mirbft_amd/csrc/stream_jobs.hpp)
under AddressSanitizer + UBSan, as a stand-alone program with its own main
(tests/cpp/stream_jobs_check.cpp), over the job lists the GPU test launches
(tests/dstream_jobs_matrix.py); and the builders proven to cover what they claim. Host
code only: nothing is loaded into Python."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import dstream_jobs_matrix as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stream_jobs") / "stream_jobs_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "stream_jobs_check.cpp")], check=True)
    return str(exe)


@pytest.fixture(scope="module")
def tile(checker):
    return int(subprocess.run([checker, "--tile"], capture_output=True, text=True, check=True).stdout)


def _digits(ids):
    return {(p, int(d)) for p in range(4) for d in np.unique((ids.astype(np.uint64) >> np.uint64(8 * p)) & np.uint64(255))}


def _never_twice_in_a_row(ids):
    return not (ids[1:] == ids[:-1]).any()


def test_order_case_covers_what_it_claims(tile):
    c = J.order_case()
    assert (c.n, c.k) == (5, 40) and set(c.ids.tolist()) == {0, 1, 2, 3, 4}
    assert c.k < 64 <= tile                                                     # one round of one wave
    assert min(np.bincount(c.ids)) >= 3 and _never_twice_in_a_row(c.ids)        # repeats, interleaved
    assert int(c.len.min()) == 0 and int(c.len.max()) == 70
    assert [len(c.seeds[s]) % 64 for s in range(4)] == [0, 1, 55, 63] and 4 not in c.seeds
    assert J.start_residues(c) == set(range(16))
    perm, n_valid = J.order(c)
    assert n_valid == 40 and sorted(perm.tolist()) == list(range(40))
    assert (np.diff(c.ids[perm].astype(np.int64)) >= 0).all()
    for s in range(5):                                                          # stable: job order inside a stream
        assert perm[c.ids[perm] == s].tolist() == np.nonzero(c.ids == s)[0].tolist()


def test_pass_edge_cases_cover_what_they_claim(tile):
    assert [n for n, _ in J.PASS_EDGES] == [1, 255, 256, 65535, 65536, 1 << 24]
    for n, passes in J.PASS_EDGES:
        c = J.pass_edge_case(n)
        assert (n.bit_length() + 7) // 8 == passes
        ids = c.ids
        assert int(ids.max()) < n and {0, n - 1} <= set(ids.tolist())
        assert min(np.unique(ids, return_counts=True)[1]) >= 3                  # every id at least three times
        assert n == 1 or _never_twice_in_a_row(ids)
        assert 550 <= c.k <= 650 and 256 < c.k < tile                           # several waves of one tile
        have = set(ids.tolist())
        for bit in J.ONE_DIGIT:                                                 # pairs that differ in exactly one digit
            if bit < n:
                assert any((x ^ bit) in have for x in have), (n, hex(bit))
                assert {0, bit} <= have
        used = _digits(ids)
        # every pass has more than one digit to order, but the top pass of n = 256^p: only the key n has its digit
        for p in range(passes):
            top_of_power = p == passes - 1 and n in (256, 65536, 1 << 24)
            assert len({d for q, d in used if q == p}) >= 2 or n == 1 or top_of_power
        assert J.start_residues(c) == set(range(16))


def test_tile_and_stream_cases_cover_what_they_claim(tile):
    T = tile
    assert T >= 512 and T % 256 == 0
    assert J.tile_edge_ks(T) == (1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5)
    for c, k in zip(J.tile_edge_cases(T), J.tile_edge_ks(T)):
        assert (c.n, c.k) == (7, k) and int(c.ids.max()) < 7
    one = J.one_stream_case(T)
    assert (one.n, one.k) == (3, 4 * T + 3) and set(one.ids.tolist()) == {1}
    assert set(one.len.tolist()) == {0, 32} and (one.len == 0).sum() > 100
    a, b = J.distinct_cases()
    assert a.n == a.k == b.n == b.k == 3000
    assert sorted(a.ids.tolist()) == list(range(3000)) and b.ids.tolist() == list(range(2999, -1, -1))
    assert J.order(b)[0].tolist() == list(range(2999, -1, -1))


def test_skew_case_covers_what_it_claims(tile):
    c = J.skew_case()
    assert (c.n, c.k) == (1000, 20000) and c.k > 4 * tile and c.k % tile       # several tiles, the last one partial
    bad = c.ids >= 1000
    assert 0.04 < bad.mean() < 0.06 and set(c.ids[bad].tolist()) == {1000, 1001, (1 << 32) - 1}
    counts = np.bincount(c.ids[~bad], minlength=1000)
    assert counts.max() > 2000 and (counts == 0).sum() > 100 and (counts > 0).sum() > 200    # heavy, empty and many streams
    perm, n_valid = J.order(c)
    assert n_valid == int((~bad).sum())
    assert perm[n_valid:].tolist() == np.nonzero(bad)[0].tolist()               # the dropped jobs last, in job order
    rows, off, ln, begin = J.grouped(c)
    assert rows.tolist() == np.nonzero(counts)[0].tolist() and int(begin[-1]) == n_valid
    assert np.diff(begin.astype(np.int64)).tolist() == counts[counts > 0].tolist()


def test_expectations_are_hashlib_over_the_job_order(tile):
    c = J.one_stream_case(tile // 64)                                           # the builder the GPU test uses, cut short
    assert J.digests(c)[0].tolist() == [1] and len(c.seeds[1]) == 5
    c = J.order_case()
    rows, dig = J.digests(c)
    assert rows.tolist() == [0, 1, 2, 3, 4]
    for r, s in enumerate(rows):
        data = c.seeds.get(int(s), b"") + b"".join(c.chunk(j) for j in range(c.k) if c.ids[j] == s)
        assert dig[r].tobytes() == hashlib.sha256(data).digest()
    g_rows, off, ln, begin = J.grouped(c)                                       # the host CSR names the same bytes
    for r, s in enumerate(g_rows):
        data = b"".join(c.arena[int(off[j]): int(off[j] + ln[j])].tobytes() for j in range(int(begin[r]), int(begin[r + 1])))
        assert hashlib.sha256(c.seeds.get(int(s), b"") + data).digest() == dig[r].tobytes()
    assert len({c.chunk(j) for j in range(c.k) if c.len[j]}) == int((c.len > 0).sum())      # distinct chunks


def test_sort_path_under_asan_ubsan(tmp_path, checker, tile):
    cases = J.sort_cases(tile)
    path = str(tmp_path / "cases.bin")
    J.write_ids(path, cases)
    r = subprocess.run([checker, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    for i, c in enumerate(cases):
        want = "case cases.bin#%d: %d streams, %d jobs, %d passes, %d valid" % (
            i, c.n, c.k, (c.n.bit_length() + 7) // 8, J.order(c)[1])
        assert want in r.stdout, want
    assert "case wide: 4294967294 streams, 5000 jobs, 4 passes" in r.stdout
    assert "layout ok" in r.stdout and "stream_jobs ok" in r.stdout
