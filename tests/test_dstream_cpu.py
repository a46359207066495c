"""The data path of k_dstream_write (mirbft_amd/csrc/stream_device.hpp) under
AddressSanitizer + UBSan, as a stand-alone program with its own main
(tests/cpp/stream_device_check.cpp), over the batches the GPU test launches
(tests/dstream_matrix.py); the builders proven to cover what they claim; and the model
shown to follow the header. Host code only: nothing is loaded into Python."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import dstream_matrix as M
import parts_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tba():
    return M.tail_by_append()


def _row_bytes(batch, r):
    arena, off, ln, begin = batch
    return b"".join(arena[int(off[j]): int(off[j]) + int(ln[j])].tobytes() for j in range(int(begin[r]), int(begin[r + 1])))


def test_tail_by_append_covers_what_it_claims(tba):
    pre, app, pairs = tba
    assert len(pairs) == 8384 and set(pairs) == {(t, a) for t in range(64) for a in range(131)}
    assert pre[3].size == app[3].size == len(pairs) + 1
    for s in (0, 1, 130, 131, 5000, 8383):                                  # rows carry what pairs says
        t, a = pairs[s]
        assert len(_row_bytes(pre, s)) == t and len(_row_bytes(app, s)) == a
    assert np.diff(pre[3].astype(np.int64)).tolist() == [1 if t else 0 for t, _ in pairs]   # one part, or a zero-part row
    assert pre[2].tolist() == [t for t, _ in pairs if t]
    app_tot = np.cumsum(np.append(0, app[2]).astype(np.int64))[app[3].astype(np.int64)]
    assert np.diff(app_tot).tolist() == [a for _, a in pairs]
    assert M.start_residues(pre) == M.start_residues(app) == set(range(16))
    counts = np.diff(app[3].astype(np.int64))
    assert set(counts.tolist()) == {1, 2, 3}                                # 1..3 parts a row
    first = app[3][:-1].astype(np.int64)
    empties = sum(1 for s in range(len(pairs)) if pairs[s][1] and (app[2][first[s]: first[s] + counts[s]] == 0).any())
    assert empties > 100                                                    # empty parts among non-empty ones
    # both sides of the block edges, and the sum's padding edges before and after the write
    for t, a in [(0, 0), (10, 53), (10, 54), (10, 55), (1, 63), (63, 1), (63, 65), (63, 66), (0, 64), (0, 128), (0, 130)]:
        assert (t, a) in pairs
    for edge in (55, 56, 63, 0):
        assert any(t % 64 == edge for t, _ in pairs)
        assert any((t + a) % 64 == edge and a for t, a in pairs)
    assert {(t + a) // 64 for t, a in pairs} == {0, 1, 2, 3}                # 0..3 blocks compressed by a write
    for b in (pre, app):
        assert b[0].size >= int((b[1] + b[2]).max()) + M.SLACK


def test_three_rounds_is_the_boundary_matrix():
    batch, rounds = M.three_rounds()
    ref = parts_matrix.boundary_matrix()
    assert rounds == 3 and all(np.array_equal(x, y) for x, y in zip(batch, ref[:4]))
    n = batch[3].size - 1
    m = M.Model(n)
    m.write(batch)
    assert np.array_equal(m.sum(), ref[4])                                  # round one: the matrix's own digests
    tails = {int(x) % 64 for x in m.lengths()}
    assert {0, 1, 55, 56, 63} <= tails                                      # what round two starts from


def test_model_follows_the_header():
    rng = np.random.default_rng(5)
    ar = parts_matrix.Arena(rng)
    pieces = [rng.bytes(70), rng.bytes(3), b"", rng.bytes(60)]
    for i, p in enumerate(pieces):
        ar.put(p, (7 * i + 1) % 16)
    arena, off, ln = ar.arrays(M.SLACK)
    begin = np.array([0, 2, 2, 4], dtype=np.uint64)
    m = M.Model(3)
    m.write((arena, off, ln, begin))
    assert m.lengths().tolist() == [73, 0, 60]
    assert m.sum()[0].tobytes() == hashlib.sha256(pieces[0] + pieces[1]).digest()
    assert m.sum()[1].tobytes() == hashlib.sha256(b"").digest()
    assert m.buffers()[0, :9].tobytes() == (pieces[0] + pieces[1])[64:] and not m.buffers()[0, 9:].any()
    # rows: a permuted subset; an id >= n and a decreasing range change nothing; sum zeroes the bad row
    bad = np.array([0, 2, 1, 4], dtype=np.uint64)
    before = m.sum()
    m.write((arena, off, ln, bad), rows=np.array([2, 1, 7], dtype=np.uint32))
    assert m.sum()[2].tobytes() == hashlib.sha256(pieces[3] + pieces[0] + pieces[1]).digest()
    assert np.array_equal(m.sum()[:2], before[:2])
    got = m.sum(rows=np.array([1, 3], dtype=np.uint32))
    assert got[0].tobytes() == hashlib.sha256(b"").digest() and not got[1].any()
    # snap: the sum, then New() + Write(sum); reset: New()
    d = m.snap(rows=[0])[0].tobytes()
    assert d == before[0].tobytes() and m.lengths()[0] == 32 and m.buffers()[0, :32].tobytes() == d
    assert m.sum()[0].tobytes() == hashlib.sha256(d).digest()
    m.reset(rows=[0])
    assert m.sum()[0].tobytes() == hashlib.sha256(b"").digest() and m.lengths()[0] == 0


def test_write_path_under_asan_ubsan(tmp_path, tba):
    pre, app, pairs = tba
    n = len(pairs)
    files = [str(tmp_path / "tail_by_append.bin"), str(tmp_path / "three_rounds.bin"), str(tmp_path / "rows.bin")]
    M.write_rounds(files[0], n, M.model_rounds(n, [(pre, None), (app, None)]))
    batch, rounds = M.three_rounds()
    n3 = batch[3].size - 1
    M.write_rounds(files[1], n3, M.model_rounds(n3, [(batch, None)] * rounds))
    # rows: the boundary matrix's rows onto a permuted subset of twice as many streams, twice; an id out of
    # range and a decreasing range among them
    rng = np.random.default_rng(11)
    rows = rng.permutation(2 * n3)[:n3].astype(np.uint32)
    rows[5] = 2 * n3 + 9
    begin = batch[3].copy()
    begin[41] = begin[40] - np.uint64(1)                                    # row 40 decreases (row 41 grows by one part)
    sub = (batch[0], batch[1], batch[2], begin)
    M.write_rounds(files[2], 2 * n3, M.model_rounds(2 * n3, [(sub, rows), (sub, rows)]))
    exe = tmp_path / "stream_device_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "stream_device_check.cpp")], check=True)
    r = subprocess.run([str(exe)] + files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "rounds: %d streams, 2 rounds, %d rows" % (n, 2 * n) in r.stdout
    assert "rounds: %d streams, 3 rounds, %d rows" % (n3, 3 * n3) in r.stdout
    assert "rounds: %d streams, 2 rounds, %d rows" % (2 * n3, 2 * n3) in r.stdout
    assert "stream_device ok" in r.stdout
