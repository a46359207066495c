"""The cases of msha_dstreams_write_jobs_routed_device (tests/dstream_jobs_route_matrix.py)
without a GPU: jobs_of() shown to round-trip -- stable grouping of its jobs gives back the
route case's per-stream byte strings -- for all three interleavings, which are shown to
differ; each jobs-only builder proven, by set equality, to reach what it claims; every
case that is not a caps case shown to fit both caps under the model alone, so the GPU
tests may demand that routed equals long exactly; the dropped-jobs case shown to tell a
model that counts dropped lengths from the right one; and the workspace layout
(mirbft_amd/csrc/stream_jobs_route.hpp) under AddressSanitizer + UBSan as a stand-alone
program with its own main (tests/cpp/stream_jobs_route_check.cpp). Host code only:
nothing is loaded into Python."""
import os
import re
import subprocess

import numpy as np
import pytest

import dstream_jobs_matrix as J
import dstream_jobs_route_matrix as R
import dstream_matrix
import dstream_route_matrix as M
from mirbft_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")
TILE = 2048


def _const(header, name):
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1).split("//")[0])


def _fits(case, streams=None):
    """The model of `case` grouped; it must fit both caps with room the GPU cannot lack."""
    streams, rc = R.grouped(case, streams)
    r = M.model_of(rc)
    assert r.all_fit and r.count == len(r.long)
    assert len(r.long) <= case.max_long <= 16 * 8             # 16 x CUs of the smallest part one could meet
    assert sum(M.round16(r.total[x]) for x in r.long) + M.SLACK <= case.long_bytes
    assert r.invalid_stream == [] and r.invalid_range == []
    return streams, rc, r


def _pre_leaves_the_tails(case):
    if case.pre is None:
        assert not case.tails
        return
    m = dstream_matrix.Model(case.n)
    m.write(case.pre)
    assert m.length == [case.tails.get(s, 0) for s in range(case.n)] and all(t < 64 for t in m.length)


def test_constants_are_the_sources():
    assert R.SLACK == L.MSHA_DEVICE_ARENA_SLACK and R.STATE_BYTES == L.MSHA_STREAM_STATE_BYTES
    assert _const("stream_jobs.hpp", "kDigitBits") == 8 and TILE == 4 * 64 * 8      # kWaves x 64 x kRounds
    assert _const("parts_plan.hpp", "kWaveSumParts") == 32 and _const("parts_concat.hpp", "kLargePart") == 512
    assert L.MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT == 64 and L.MSHA_ROUTE_LONG_BYTES_DEFAULT == 32 << 20


@pytest.mark.parametrize("interleave", R.INTERLEAVES)
def test_jobs_of_round_trips(interleave):
    """Grouping the jobs stably by stream gives back every row's bytes, the route model of
    the grouped case is the route case's own, and the opts and the pre batch travel."""
    seen = 0
    for name, rc, caps in R.converted():
        case = R.jobs_of(rc, interleave)
        _pre_leaves_the_tails(case)
        want = {s: d for s, d in R.row_bytes(rc).items() if d}
        assert {s: d for s, d in R.stream_bytes(case).items() if d} == want, name
        assert case.k == rc.batch[1].size and case.valid().all()
        streams, g = R.grouped(case)
        assert g.n == rc.n and g.tails == list(rc.tails) and g.opts() == rc.opts()
        stream_of = (lambda r: r) if rc.rows is None else (lambda r: int(rc.rows[r]))
        a, b = M.model_of(rc), M.model_of(g)
        assert {stream_of(r) for r in a.long} == b.long, name
        assert {stream_of(r): t for r, t in a.total.items()} == b.total
        assert (a.all_fit, a.count) == (b.all_fit, b.count)
        assert {s: b.whole[s] for s in (stream_of(r) for r in a.whole)} == {stream_of(r): w for r, w in a.whole.items()}
        seen += 1
    assert seen == 3 + 1 + 1 + 10 + len(R.CAPS) + 2


def test_interleavings_differ_and_keep_each_rows_order():
    rc, _ = M.slots(9)
    cases = {i: R.jobs_of(rc, i) for i in R.INTERLEAVES}
    assert len({c.ids.tobytes() for c in cases.values()}) == 3
    begin = rc.batch[3]
    counts = [int(b) - int(a) for a, b in zip(begin, begin[1:])]
    rr, rev, sh = (cases[i].ids.tolist() for i in R.INTERLEAVES)
    live = [r for r, c in enumerate(counts) if c]
    assert rr[:len(live)] == live                                   # one job of every row that has one
    assert rev == [r for r in reversed(range(len(counts))) for _ in range(counts[r])]
    assert sh != sorted(sh) and sh != rev and sorted(sh) == sorted(rr)
    for c in cases.values():                                        # a row's offsets in the row's order
        for r in live:
            mine = c.off[c.ids == r]
            assert mine.tolist() == rc.batch[1][int(begin[r]): int(begin[r + 1])].tolist()
    # slots permuted: the jobs name the permuted streams
    rc, _ = M.slots(9, permute=True)
    c = R.jobs_of(rc, "round_robin")
    assert set(c.ids.tolist()) <= set(rc.rows.tolist()) and c.n == rc.n > rc.rows.size


def test_converted_non_caps_cases_fit_both_caps():
    for name, rc, caps in R.converted():
        for interleave in R.INTERLEAVES:
            case = R.jobs_of(rc, interleave)
            if not caps:
                _fits(case)
    for (max_long, long_bytes), want in zip(R.CAPS, R.CAPS_WANT):
        r = M.model_of(R.grouped(R.jobs_of(M.caps(max_long, long_bytes), "shuffle"))[1])
        assert r.count == want and r.long == {0, 2, 3, 5, 7}


def test_dropped_jobs_cover_what_they_claim():
    case, (below, at, short) = R.dropped_jobs()
    _pre_leaves_the_tails(case)
    streams, rc, r = _fits(case)
    n, lb = case.n, case.long_blocks
    dropped = [j for j in range(case.k) if int(case.ids[j]) >= n]
    assert {int(case.ids[j]) for j in dropped} == set(J.INVALID(n)) == {n, n + 1, 0xFFFFFFFF}
    assert dropped[-1] == case.k - 1                                # the call's last job is dropped
    assert all(int(case.len[j]) == R.DROP_LEN for j in dropped) and len(dropped) == 6
    assert r.long == {at} and r.whole[at] == lb and r.total[at] == 64 * lb
    assert case.tails[below] + int(case.len[case.ids == below].sum()) == 64 * lb - 1 and r.whole[below] == lb - 1
    assert short not in r.long and r.whole[short] == 0
    # dealt between the two streams' jobs: a dropped job before and after a job of each
    for s in (below, at):
        mine = np.nonzero(case.ids == s)[0]
        assert any(mine[0] < j < mine[-1] for j in dropped), s
    # the model that counts dropped lengths for the stream they are dealt to finds another long set
    naive = dict(r.whole)
    for j, s in case.note["adopt"].items():
        naive[s] = (case.tails.get(s, 0) + int(case.len[case.ids == s].sum()) + R.DROP_LEN) // 64
    assert sorted(case.note["adopt"]) == dropped
    assert {s for s, w in naive.items() if w >= lb} == {below, at} != r.long
    # and the order puts them last
    perm, n_valid = R.order(case)
    assert n_valid == case.k - len(dropped) and sorted(perm[n_valid:].tolist()) == dropped


def test_empty_chunks_cover_what_they_claim():
    case, nm = R.empty_chunks()
    _pre_leaves_the_tails(case)
    streams, rc, r = _fits(case)
    lens = {s: case.len[case.ids == s].tolist() for s in range(case.n)}
    assert r.long == {nm["inside"], nm["one_job"], nm["wave_below"], nm["wave_at"], nm["large"]}
    inside = lens[nm["inside"]]
    assert 0 in inside[1:-1] and inside[0] and inside[-1] and inside.count(0) == 4
    assert lens[nm["only_empty"]] == [0] * 5 and case.tails[nm["only_empty"]] == 7 and r.whole[nm["only_empty"]] == 0
    assert len(lens[nm["one_job"]]) == 1
    wave = _const("parts_plan.hpp", "kWaveSumParts")
    assert (len(lens[nm["wave_below"]]), len(lens[nm["wave_at"]])) == (wave - 1, wave)
    assert lens[nm["large"]] == [_const("parts_concat.hpp", "kLargePart")]
    assert all(case.tails.get(s, 0) for s in (nm["inside"], nm["one_job"], nm["wave_at"], nm["large"]))
    ids = case.ids.tolist()
    assert all(a != b for a, b in zip(ids[:6], ids[1:6]))            # interleaved, not stream by stream


@pytest.mark.parametrize("n,passes", J.PASS_EDGES)
def test_pass_edges_cover_what_they_claim(n, passes):
    case, long_ids = R.pass_edges(n)
    assert case.n == n and case.pre is None and (n.bit_length() + 7) // 8 == passes
    assert set(long_ids) == {s for s in (0, 255, 256, 65535) if s < n} | {n - 1}
    touched = case.touched()
    streams, rc, r = _fits(case, touched)
    assert {int(streams[x]) for x in r.long} == set(long_ids)
    short = [int(s) for s in touched if int(s) not in long_ids]
    assert all(int(case.len[case.ids == s].sum()) < 64 for s in short)
    assert len(short) >= 30 or n == 1                                # n == 1: the one stream is the long one
    # the long ids differ only in the top digit of some pass from an id that is there too
    if n > 65536:
        assert {0, 255, 256, 65535, n - 1} <= set(touched.tolist())
    # every long stream's jobs are spread through the call, short jobs between them
    for s in long_ids:
        mine = np.nonzero(case.ids == s)[0]
        assert mine.size >= 5 and (n == 1 or len(short) == 0 or mine[-1] - mine[0] > mine.size)
    assert case.k < 400


@pytest.mark.parametrize("k", [TILE - 1, TILE, TILE + 1])
def test_tile_edges_cover_what_they_claim(k):
    case, long_stream = R.tile_edges(TILE, k)
    assert case.k == k and case.n == 7 and case.long_blocks == L.MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT
    streams, rc, r = _fits(case)
    assert r.long == {long_stream}
    assert max(w for s, w in r.whole.items() if s != long_stream) < 16
    pos = set(np.nonzero(case.ids == long_stream)[0].tolist())
    assert pos == set(case.note["positions"]) and {0, k - 1} <= pos
    if k > TILE:
        assert {TILE - 1, TILE} <= pos                               # on both sides of the tile boundary
    else:
        assert k - 1 in pos and J.tile_edge_ks(TILE)[8:11] == (TILE - 1, TILE, TILE + 1)
    assert set(case.ids.tolist()) == set(range(7)) and 0 in case.len.tolist()


def test_reference_shape():
    case = R.reference_shape()
    assert case.opts() == {} and case.defaults and (case.n, case.k) == (4, 2048)
    assert case.ids[:9].tolist() == [0, 1, 2, 3, 0, 1, 2, 3, 0] and set(case.len.tolist()) == {32}
    streams, rc, r = _fits(case)
    assert r.long == {0, 1, 2, 3} and set(r.whole.values()) == {256}
    assert case.long_blocks == L.MSHA_DSTREAMS_ROUTE_LONG_BLOCKS_DEFAULT
    assert case.long_bytes <= L.MSHA_ROUTE_LONG_BYTES_DEFAULT       # the model's caps are within the defaults


def test_fed_restates_an_export():
    import hashlib
    case, _ = R.empty_chunks()
    fed = R.Fed(range(case.n))
    fed.write(case.pre)
    fed.write_jobs(case)
    ex = fed.export()
    m = dstream_matrix.Model(case.n)
    m.write(case.pre)
    m.write(R.grouped(case)[1].batch)
    assert np.array_equal(ex[:, 36:100], m.buffers())
    assert np.array_equal(ex[:, 100:108].copy().view(">u8").reshape(-1), m.lengths())
    assert [hashlib.sha256(fed.data[s]).digest() for s in range(case.n)] == [bytes(x) for x in m.sum()]


def test_layout_under_asan_ubsan(tmp_path):
    exe = tmp_path / "stream_jobs_route_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "stream_jobs_route_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"stream_jobs_route ok: (\d+) layouts, (\d+) refused", r.stdout)
    assert m and int(m.group(1)) == 6 * 6 * 3 * 4 and int(m.group(2)) == 10
