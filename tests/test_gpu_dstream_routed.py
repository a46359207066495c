"""msha_dstreams_write_routed_device on the GPU (mirbft_amd/csrc/stream_chain.hip and the
chain kernel k_absorb_chain8): Write with its long rows on the eight-lane chain. Every
case compares the whole 108-byte export of every stream with the model -- hashlib-fed
streams (tests/dstream_matrix.py Model) for buffer and length, FIPS 180-4 in Python
(tests/stream_matrix.py) for the chaining state -- and with a twin set fed by
write_device; the device status; the routed rows against the route model
(tests/dstream_route_matrix.py, whose cases tests/test_dstream_route_cpu.py proves); and
every launch counter. Thresholds are forced small through the opts."""
import hashlib
import struct

import numpy as np
import pytest

import dstream_matrix as D
import dstream_route_matrix as M
import stream_matrix as S
from mirbft_amd import DeviceStreamSet, MshaError
from mirbft_amd import _lib as L

pytestmark = pytest.mark.gpu

BEGIN_TEXT = ("msha_hash_actions_device: action_part_begin decreases (begin[i+1] < begin[i]); "
              "those digests are zero")
ROW_TEXT = "msha_dstreams_*: row out of range"
ROUTE_DELTA = {"calls": 1, "launches_route": 2, "launches_copy": 1, "launches_chain": 1, "launches_tail": 1,
               "launches_write": 1}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.size == 0:
        return torch.empty(0, dtype=torch.from_numpy(a).dtype, device="cuda:0")
    return torch.from_numpy(a).to("cuda:0")


def _sync():
    import torch
    torch.cuda.synchronize()


class Bytes:
    """What each stream was fed, to restate its chaining state in Python."""

    def __init__(self, n):
        self.n = n
        self.data = [b""] * n

    def write(self, batch, rows=None):
        arena, off, ln, begin = batch
        ids = range(self.n) if rows is None else [int(r) for r in rows]
        for r, s in enumerate(ids):
            j0, j1 = int(begin[r]), int(begin[r + 1])
            if s >= self.n or j1 < j0:
                continue
            self.data[s] += b"".join(arena[int(off[j]): int(off[j]) + int(ln[j])].tobytes() for j in range(j0, j1))

    def export(self):
        out = np.zeros((self.n, L.MSHA_STREAM_STATE_BYTES), dtype=np.uint8)
        for s, d in enumerate(self.data):
            keep = len(d) % 64
            row = (b"sha\x03" + struct.pack(">8I", *S.midstate(d)) + (d[len(d) - keep:] if keep else b"").ljust(64, b"\0")
                   + struct.pack(">Q", len(d)))
            out[s] = np.frombuffer(row, dtype=np.uint8)
        return out


def _status(engine):
    """'' when clean, else the error's text; a second look is always clean (reported once)."""
    try:
        engine.device_status()
    except MshaError as e:
        assert e.code == L.MSHA_ERR_INVALID_ARG
        engine.device_status()
        return str(e)
    return ""


def _delta(after, before):
    return {k: after[k] - before[k] for k in after if not k.startswith("last_") and after[k] != before[k]}


def _check_export(s, twin, model, fed, where):
    ex, ex2 = s.export_state(), twin.export_state()
    want = fed.export()
    bad = [int(i) for i in np.nonzero((ex != want).any(axis=1))[0]]
    assert bad == [], (where, bad[:8])
    assert np.array_equal(ex, ex2), where
    assert np.array_equal(ex[:, 36:100], model.buffers()), where            # zero past the buffered count
    assert np.array_equal(ex[:, 100:108].copy().view(">u8").reshape(-1), model.lengths()), where


def _run(engine, case, want_status=(), timing=False):
    """One routed call of `case` on a fresh set beside a twin fed by write_device.
    -> (routed rows, route model)."""
    with DeviceStreamSet(engine, case.n) as s, DeviceStreamSet(engine, case.n) as twin:
        model, fed = D.Model(case.n), Bytes(case.n)
        pre = [_dev(x) for x in case.pre]
        for x in (s, twin):
            x.write_device(*pre)
        model.write(case.pre)
        fed.write(case.pre)
        _sync()
        assert s.lengths().tolist() == list(case.tails)
        route = M.model_of(case, model.length)
        batch = [_dev(x) for x in case.batch]
        rows = None if case.rows is None else _dev(case.rows)
        b_stats, b_jobs, b_route, b_eng = s.stats(), s.jobs_stats(), s.route_stats(), engine.stats()
        s.write_routed_device(*batch, rows=rows, **case.opts())
        _sync()
        text = _status(engine)
        a_route = s.route_stats()
        assert s.stats() == b_stats and s.jobs_stats() == b_jobs             # neither counts a routed call
        assert _delta(a_route, b_route) == dict(ROUTE_DELTA, rows=case.batch[3].size - 1)
        eng = _delta(engine.stats(), b_eng)
        assert {k: v for k, v in eng.items() if k.startswith("launches_")} == {"launches_coop": 1, "launches_chain8": 1}
        twin.write_device(*batch, rows=rows)
        _sync()
        assert _status(engine) == text                                       # the same errors as write_device
        for t in want_status:
            assert t in text, (t, text)
        assert "concat" not in text and (bool(text) == bool(want_status))    # bit 16 is never raised
        model.write(case.batch, case.rows)
        fed.write(case.batch, case.rows)
        _check_export(s, twin, model, fed, "after the routed call")
        ids, nbytes = s.routed_rows()
        problems = M.check_route(ids.tolist(), nbytes, route)
        assert problems == [], problems
        if timing:
            assert a_route["last_routed"] == len(ids) and a_route["last_routed_bytes"] == nbytes
            assert a_route["last_kernel_ms"] > 0
        else:
            assert a_route["last_routed"] == a_route["last_routed_bytes"] == 0 and a_route["last_kernel_ms"] == 0
        return sorted(ids.tolist()), route


@pytest.mark.parametrize("long_blocks", [2, 3, 4])
def test_threshold_edge(engine, long_blocks, monkeypatch):
    """Prior tails 0, 1, 55, 56, 63 x totals 64 L - 1, 64 L, 64 L + 1 for L = long_blocks and
    L + 1: exactly the rows whose write compresses long_blocks blocks or more are routed."""
    if long_blocks == 3:
        monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    case, combos = M.threshold_edge(long_blocks)
    ids, route = _run(engine, case, timing=long_blocks == 3)
    assert ids == sorted(i for i, (_, lx, d) in enumerate(combos) if 64 * lx + d >= 64 * long_blocks)
    assert len(ids) == 25


def test_new_tail_edges(engine):
    case, combos = M.new_tail_edges()
    ids, route = _run(engine, case)
    assert ids == list(range(len(combos)))


@pytest.mark.parametrize("wave_sum", [None, "1"])
def test_gather_paths(engine, monkeypatch, wave_sum):
    """A part of 2,000 bytes at an odd offset (the whole workgroup copies it), 300 small
    parts with empty ones among them (two steps of the copy, the wave's sum), and the same
    with every row summed by its wave."""
    if wave_sum:
        monkeypatch.setenv("MSHA_PARTS_PLAN_WAVE_SUM", wave_sum)
    case, (three, many, short) = M.gather_paths()
    ids, route = _run(engine, case)
    assert ids == [three, many]


@pytest.mark.parametrize("k", [1, 8, 9, 16, 17])
@pytest.mark.parametrize("permute", [False, True])
def test_slots(engine, k, permute):
    case, routed = M.slots(k, permute=permute)
    ids, route = _run(engine, case)
    assert ids == routed


def test_slots_one_long_chain_beside_short_ones(engine):
    case, routed = M.slots(4, big=True)
    ids, route = _run(engine, case)
    assert ids == routed and route.whole[routed[0]] == 65


R16 = M.round16(M.CAP_TOTAL)


@pytest.mark.parametrize("max_long,long_bytes,want", [
    (1, M.LONG_BYTES, 1), (2, M.LONG_BYTES, 2), (5, M.LONG_BYTES, 5),
    (64, 5 * R16 + M.SLACK, 5), (64, 5 * R16 + M.SLACK - 1, 4),
    (64, 3 * R16 + M.SLACK, 3), (64, 3 * R16 + M.SLACK - 1, 2)])
def test_caps(engine, max_long, long_bytes, want):
    """Five long rows of one total: the header's count is routed, and every stream is
    exact whichever rows they are."""
    ids, route = _run(engine, M.caps(max_long, long_bytes))
    assert len(ids) == want == route.count and set(ids) <= route.long


def test_errors_beside_routed_rows(engine):
    case, (bad_stream, bad_range, _) = M.errors()
    ids, route = _run(engine, case, want_status=(ROW_TEXT, BEGIN_TEXT))
    assert bad_stream not in ids and bad_range not in ids and len(ids) >= 2


def test_no_long_row(engine):
    ids, route = _run(engine, M.no_long())
    assert ids == [] and route.long == set()


def test_rounds(engine):
    """Three routed writes to the same streams with write_device, snap_device and
    sum_device between them; the sums against hashlib."""
    import torch
    case = M.rounds_case()
    n = case.n
    other = M.no_long()
    small = tuple(x if i < 3 else x[:n + 1] for i, x in enumerate(other.batch))      # its first n rows
    with DeviceStreamSet(engine, n) as s, DeviceStreamSet(engine, n) as twin:
        model, fed = D.Model(n), Bytes(n)
        batch, sm = [_dev(x) for x in case.batch], [_dev(x) for x in small]
        out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
        _sync()
        for k in range(3):
            route = M.model_of(case, model.length)
            s.write_routed_device(*batch, **case.opts())
            twin.write_device(*batch)
            model.write(case.batch)
            fed.write(case.batch)
            _sync()
            ids, nbytes = s.routed_rows()
            assert M.check_route(ids.tolist(), nbytes, route) == [] and sorted(ids.tolist()) == [0, 1, 3, 5], k
            _check_export(s, twin, model, fed, k)
            s.sum_device(out)
            _sync()
            assert np.array_equal(out.cpu().numpy(), model.sum()), k
            want = [hashlib.sha256(d).digest() for d in fed.data]
            assert [bytes(r) for r in out.cpu().numpy()] == want, k
            if k == 0:
                for x in (s, twin):
                    x.write_device(*sm)
                model.write(small)
                fed.write(small)
            if k == 1:
                for x in (s, twin):
                    x.snap_device(out)
                _sync()
                model.snap()
                fed.data = [hashlib.sha256(d).digest() for d in fed.data]
                assert [bytes(r) for r in out.cpu().numpy()] == fed.data
        assert s.route_stats()["calls"] == 3 and _status(engine) == ""


def test_workspace_grows_between_calls_on_two_streams(engine):
    """A small routed write, one that must grow the set's workspace, the small one again,
    alternating between two caller streams with no host wait between them; the sums
    against hashlib. The set is fresh, so the first call allocates for 6 rows and a 4 KiB
    buffer (under 5 KB with its spare) and the second needs 300 rows and 64 KiB: the old
    buffer is freed under a call that may still be running."""
    import torch
    n = 300
    rng = np.random.default_rng(0x6A0)
    arena = rng.integers(0, 256, (1 << 16) + M.SLACK, dtype=np.uint8)

    def batch(k, least, span):
        """k rows of two parts, least .. least + span - 1 bytes a row: from 128 bytes a row is long at long_blocks 2."""
        total = np.array([least + (37 * r) % span for r in range(k)], dtype=np.uint64)
        first = total // 3
        ln = np.stack([first, total - first], axis=1).reshape(-1)
        off = rng.integers(0, (1 << 16) - 200, 2 * k).astype(np.uint64)
        return arena, off, ln, np.arange(0, 2 * k + 1, 2, dtype=np.uint64)

    few = np.array([7, 2, 299, 11, 5, 0], dtype=np.uint32)
    calls = [(batch(few.size, 130, 60), few, 4 << 10), (batch(n, 40, 150), None, 64 << 10),
             (batch(few.size, 130, 60), few, 4 << 10)]
    assert all(sum(1 for r in range(b[3].size - 1) if int(b[2][2 * r] + b[2][2 * r + 1]) >= 128) > 4 for b, _, _ in calls)
    dev = [([_dev(x) for x in b], None if rows is None else _dev(rows)) for b, rows, _ in calls]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    with DeviceStreamSet(engine, n) as s:
        fed = Bytes(n)
        _sync()
        for k, (b, rows, long_bytes) in enumerate(calls):
            s.write_routed_device(*dev[k][0], rows=dev[k][1], stream=streams[k % 2], long_blocks=2, max_long=4,
                                  long_bytes=long_bytes)
            fed.write(b, rows)
        _sync()
        assert _status(engine) == "" and s.route_stats()["calls"] == 3
        assert len(s.routed_rows()[0]) == 4                                  # the last call's: more long rows than slots
        s.sum_device(out)
        _sync()
        assert [bytes(r) for r in out.cpu().numpy()] == [hashlib.sha256(d).digest() for d in fed.data]


def test_capture(engine):
    """Refused with the jobs entry's text while the workspace is too small; after one call
    outside the capture, capture and two replays: the streams have appended three times."""
    import torch
    case, routed = M.slots(9)
    n = case.n
    batch = [_dev(x) for x in case.batch]
    with DeviceStreamSet(engine, n) as s, DeviceStreamSet(engine, n) as twin:
        model, fed = D.Model(n), Bytes(n)
        st = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        _sync()
        with torch.cuda.stream(st):
            g.capture_begin()
            try:
                with pytest.raises(MshaError, match="the workspace cannot grow while the stream is being captured: "
                                                    "make one call of this size outside the capture first"):
                    s.write_routed_device(*batch, stream=st, **case.opts())
                s.reset_device(stream=st)                                    # the refusal left the capture valid
            finally:
                g.capture_end()
        del g
        _sync()
        assert s.route_stats()["calls"] == 0 and not s.lengths().any()
        s.write_routed_device(*batch, **case.opts())
        _sync()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            g.capture_begin()
            try:
                s.write_routed_device(*batch, stream=st, **case.opts())
            finally:
                g.capture_end()                                              # raises if the capture was invalidated
        _sync()
        assert s.route_stats()["calls"] == 2
        g.replay()
        _sync()
        g.replay()
        _sync()
        for _ in range(3):
            twin.write_device(*batch)
            model.write(case.batch)
            fed.write(case.batch)
        _sync()
        _check_export(s, twin, model, fed, "after two replays")
        assert _status(engine) == ""
        del g
