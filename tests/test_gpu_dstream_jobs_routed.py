"""msha_dstreams_write_jobs_routed_device on the GPU: jobs in call order, grouped by stream
inside the call (mirbft_amd/csrc/stream_jobs.hip), the grouped streams written with the
long ones on the eight-lane chain (stream_chain.hip, k_absorb_chain8). Every case
(tests/dstream_jobs_route_matrix.py, whose cases tests/test_dstream_jobs_route_cpu.py
proves) runs on a fresh set beside a twin fed by write_jobs_device and compares the whole
108-byte export of every stream with the model -- hashlib-fed streams
(tests/dstream_matrix.py Model) for buffer and length, FIPS 180-4 in Python for the
chaining state -- and with the twin; the device status; the routed streams against the
route model of tests/dstream_route_matrix.py; the job order against numpy's stable
argsort; and every counter. Thresholds are forced small through the opts."""
import dataclasses
import hashlib

import numpy as np
import pytest

import dstream_jobs_matrix as J
import dstream_jobs_route_matrix as R
import dstream_matrix as D
import dstream_route_matrix as M
from mirbft_amd import DeviceStreamSet, MshaError
from mirbft_amd import _lib as L

pytestmark = pytest.mark.gpu

ROW_TEXT = "msha_dstreams_*: row out of range (a d_row entry >= n); no stream was touched and those digests are zero"
WS_TEXT = ("the workspace cannot grow while the stream is being captured: "
           "make one call of this size outside the capture first")
FULL_SET = 5000             # sets up to this many streams are modelled and compared whole
DELTA = {"calls": 1, "launches_rows": 2, "launches_route": 2, "launches_copy": 1, "launches_chain": 1,
         "launches_tail": 1, "launches_write": 1}


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


def _job_args(case):
    return [_dev(case.arena), _dev(case.ids), _dev(case.off), _dev(case.len)]


def _passes(n):
    return (n.bit_length() + 7) // 8


def _modelled(case):
    """The streams the models restate: all of a small set, the touched ones of a large one."""
    return np.arange(case.n, dtype=np.uint32) if case.n <= FULL_SET else case.touched()


def _watched(case, streams):
    """Streams compared with the twin and with what they held before: the modelled ones,
    and of a large set their neighbours and a spread of others."""
    if case.n <= FULL_SET:
        return streams.astype(np.uint64)
    t = streams.astype(np.int64)
    near = np.concatenate([t, t - 1, t + 1, np.linspace(0, case.n - 1, 300).astype(np.int64)])
    return np.unique(near[(near >= 0) & (near < case.n)]).astype(np.uint64)


def _check_export(s, twin, streams, watch, model, fed, where):
    ex = s.export_state(streams.astype(np.uint64))
    want = fed.export()
    bad = [int(streams[i]) for i in np.nonzero((ex != want).any(axis=1))[0]]
    assert bad == [], (where, bad[:8])
    assert np.array_equal(ex[:, 36:100], model.buffers()), where            # zero past the buffered count
    assert np.array_equal(ex[:, 100:108].copy().view(">u8").reshape(-1), model.lengths()), where
    assert np.array_equal(s.export_state(watch), twin.export_state(watch)), where


def _check_read(s, case, streams, route):
    """The read-back of the set's last call against numpy's argsort and the route model.
    -> the routed streams, sorted."""
    order, n_valid, routed, nbytes = s.jobs_route_read()
    perm, want_valid = R.order(case)
    assert n_valid == want_valid
    assert np.array_equal(order, perm), np.nonzero(order != perm)[0][:10]
    assert np.isin(routed, streams).all(), routed
    rows = np.searchsorted(streams, routed)                                  # the model's row of each routed stream
    problems = M.check_route(rows.tolist(), nbytes, route)
    assert problems == [], problems
    return sorted(int(x) for x in routed), nbytes


def _run(engine, case, dropped=False, timing=False):
    """One call of `case` on a fresh set beside a twin fed by write_jobs_device.
    -> (routed streams, route model, the model's streams)."""
    streams = _modelled(case)
    watch = _watched(case, streams)
    _, rc = R.grouped(case, streams)
    p = _passes(case.n)
    with DeviceStreamSet(engine, case.n) as s, DeviceStreamSet(engine, case.n) as twin:
        model, fed = D.Model(int(streams.size)), R.Fed(streams)
        if case.pre is not None:
            pre = [_dev(x) for x in case.pre]
            for x in (s, twin):
                x.write_device(*pre)
            model.write(case.pre)
            fed.write(case.pre)
            _sync()
            assert s.lengths().tolist() == [case.tails.get(i, 0) for i in range(case.n)]
        before = s.export_state(watch)
        route = M.model_of(rc, model.length)
        jargs = _job_args(case)
        b_stats, b_jobs, b_route, b_jr, b_eng = s.stats(), s.jobs_stats(), s.route_stats(), s.jobs_route_stats(), \
            engine.stats()
        assert b_jr["calls"] == 0
        s.write_jobs_routed_device(*jargs, **case.opts())
        _sync()
        text = _status(engine)
        a_jr = s.jobs_route_stats()
        # none of the three older structs counts the call
        assert s.stats() == b_stats and s.jobs_stats() == b_jobs and s.route_stats() == b_route
        assert _delta(a_jr, b_jr) == dict(DELTA, jobs=case.k, launches_sort=3 * p)
        assert (a_jr["last_passes"], a_jr["last_jobs"]) == (p, case.k)
        eng = _delta(engine.stats(), b_eng)
        assert {k: v for k, v in eng.items() if k.startswith("launches_")} == {"launches_coop": 1, "launches_chain8": 1}
        twin.write_jobs_device(*jargs)
        _sync()
        assert _status(engine) == text                                       # the same errors as write_jobs_device
        if dropped:
            assert text.endswith(ROW_TEXT) and "decreases" not in text and "concat" not in text, text  # bit 32 alone
        else:
            assert text == ""
        model.write(rc.batch)
        fed.write_jobs(case)
        _check_export(s, twin, streams, watch, model, fed, "after the call")
        after = s.export_state(watch)
        idle = ~np.isin(watch, case.touched().astype(np.uint64))
        assert np.array_equal(after[idle], before[idle])                     # no valid job names them: bit-identical
        routed, nbytes = _check_read(s, case, streams, route)
        # the two older read-backs keep meaning the last jobs call and the last routed call: there was none
        assert s.jobs_order()[0].size == 0 and s.routed_rows()[0].size == 0
        if timing:
            assert a_jr["last_routed"] == len(routed) and a_jr["last_routed_bytes"] == nbytes
            assert a_jr["last_kernel_ms"] > 0
        else:
            assert a_jr["last_routed"] == a_jr["last_routed_bytes"] == 0 and a_jr["last_kernel_ms"] == 0
        return routed, route, streams


def _long_streams(route, streams):
    return sorted(int(streams[r]) for r in route.long)


# ---- the converter over the route matrix --------------------------------------------
@pytest.mark.parametrize("interleave", R.INTERLEAVES)
@pytest.mark.parametrize("long_blocks", [2, 3, 4])
def test_threshold_edge(engine, long_blocks, interleave, monkeypatch):
    """MSHA_PARTS_TIMING=1 on one of the nine: last_routed, last_routed_bytes and
    last_kernel_ms are filled then and zero otherwise."""
    timing = long_blocks == 3 and interleave == "shuffle"
    if timing:
        monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    rc, combos = M.threshold_edge(long_blocks)
    routed, route, streams = _run(engine, R.jobs_of(rc, interleave), timing=timing)
    assert routed == sorted(i for i, (_, lx, d) in enumerate(combos) if 64 * lx + d >= 64 * long_blocks)
    assert len(routed) == 25


@pytest.mark.parametrize("interleave", R.INTERLEAVES)
def test_new_tail_edges(engine, interleave):
    rc, combos = M.new_tail_edges()
    routed, route, _ = _run(engine, R.jobs_of(rc, interleave))
    assert routed == list(range(len(combos)))


@pytest.mark.parametrize("interleave", R.INTERLEAVES)
@pytest.mark.parametrize("wave_sum", [None, "1"])
def test_gather_paths(engine, monkeypatch, wave_sum, interleave):
    if wave_sum:
        monkeypatch.setenv("MSHA_PARTS_PLAN_WAVE_SUM", wave_sum)
    rc, (three, many, short) = M.gather_paths()
    routed, route, _ = _run(engine, R.jobs_of(rc, interleave))
    assert routed == [three, many]


@pytest.mark.parametrize("interleave", R.INTERLEAVES)
@pytest.mark.parametrize("k", [1, 8, 9, 16, 17])
@pytest.mark.parametrize("permute", [False, True])
def test_slots(engine, k, permute, interleave):
    rc, rows = M.slots(k, permute=permute)
    routed, route, _ = _run(engine, R.jobs_of(rc, interleave))
    assert routed == sorted(r if rc.rows is None else int(rc.rows[r]) for r in rows)


@pytest.mark.parametrize("interleave", R.INTERLEAVES)
@pytest.mark.parametrize("caps,want", list(zip(R.CAPS, R.CAPS_WANT)))
def test_caps(engine, caps, want, interleave):
    """Five long streams of one total: the header's count is routed, and every stream is
    exact whichever they are."""
    routed, route, _ = _run(engine, R.jobs_of(M.caps(*caps), interleave))
    assert len(routed) == want == route.count and set(routed) <= route.long


@pytest.mark.parametrize("interleave", R.INTERLEAVES)
def test_no_long_stream(engine, interleave):
    routed, route, _ = _run(engine, R.jobs_of(M.no_long(), interleave))
    assert routed == [] and route.long == set()


@pytest.mark.parametrize("interleave", R.INTERLEAVES)
def test_rounds_case(engine, interleave):
    routed, route, _ = _run(engine, R.jobs_of(M.rounds_case(), interleave))
    assert routed == [0, 1, 3, 5]


# ---- what only jobs can say ----------------------------------------------------------
def test_dropped_jobs(engine):
    """Ids n, n + 1 and 0xFFFFFFFF between the jobs of a stream one byte under the threshold
    and of one at it: the first stays a lane, the second is routed, bit 32 is reported once."""
    case, (below, at, short) = R.dropped_jobs()
    routed, route, _ = _run(engine, case, dropped=True)
    assert routed == [at]


def test_empty_chunks(engine):
    case, nm = R.empty_chunks()
    routed, route, _ = _run(engine, case)
    assert routed == sorted(nm[k] for k in ("inside", "one_job", "wave_below", "wave_at", "large"))


@pytest.mark.parametrize("n,passes", J.PASS_EDGES)
def test_pass_edges(engine, n, passes):
    case, long_ids = R.pass_edges(n)
    assert _passes(n) == passes
    routed, route, streams = _run(engine, case)
    assert routed == long_ids == _long_streams(route, streams)


@pytest.fixture(scope="module")
def tile(engine):
    with DeviceStreamSet(engine, 1) as s:
        return int(s.jobs_stats()["tile_jobs"])


@pytest.mark.parametrize("dk", [-1, 0, 1])
def test_tile_edges(engine, tile, dk):
    case, long_stream = R.tile_edges(tile, tile + dk)
    routed, route, _ = _run(engine, case)
    assert routed == [long_stream]


def test_reference_shape_with_default_opts(engine):
    """4 streams x 512 digests of 32 bytes in commit-major order, no opts: 256 blocks a
    stream, all four routed; the sums against hashlib."""
    import torch
    case = R.reference_shape()
    routed, route, _ = _run(engine, case)
    assert routed == [0, 1, 2, 3]
    with DeviceStreamSet(engine, case.n) as s:
        out = torch.zeros((case.n, 32), dtype=torch.uint8, device="cuda:0")
        _sync()
        s.write_jobs_routed_device(*_job_args(case))
        s.sum_device(out)
        _sync()
        rows = case.arena[: 32 * case.k].reshape(-1, case.n, 32)
        assert [bytes(r) for r in out.cpu().numpy()] == [hashlib.sha256(rows[:, i].tobytes()).digest()
                                                         for i in range(case.n)]
        assert _status(engine) == ""


# ---- beyond the matrix ---------------------------------------------------------------
def test_calls_in_sequence(engine):
    """Three calls on one set -- stream 2 long in the first, short in the second, long again
    in the third -- with write_device, write_jobs_device, write_routed_device and
    snap_device between them; every export against the models and the twin, the sums
    against hashlib, and the older entries' read-backs left meaning their own last calls."""
    import torch
    n, lb = 5, 2
    opts = dict(long_blocks=lb, max_long=M.MAX_LONG, long_bytes=M.LONG_BYTES)
    streams = np.arange(n, dtype=np.uint32)

    def jobs(seed, lens_by_stream):
        b = R._Jobs(seed, n)
        b.deal([(s, list(lens)) for s, lens in lens_by_stream.items()])
        return b.case(lb)

    calls = [jobs(0x5E01, {0: [10, 20], 2: [100, 0, 90, 70], 4: [300]}),            # 2: 260 bytes, long
             jobs(0x5E02, {1: [64, 64, 1], 2: [5, 6], 3: [0]}),                     # 2: short
             jobs(0x5E03, {2: [33] * 9, 0: [7], n + 1: [50]})]                      # 2: long again, one job dropped
    other = jobs(0x5E04, {0: [40], 2: [9, 9], 3: [200]})                            # what the older entries are given
    with DeviceStreamSet(engine, n) as s, DeviceStreamSet(engine, n) as twin:
        model, fed = D.Model(n), R.Fed(streams)
        out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
        _sync()
        og = R.grouped(other)[1].batch
        d_og = [_dev(x) for x in og]

        def both(name, *a, **kw):
            for x in (s, twin):
                getattr(x, name)(*a, **kw)

        for k, case in enumerate(calls):
            _, rc = R.grouped(case)
            route = M.model_of(rc, model.length)
            jargs = _job_args(case)
            s.write_jobs_routed_device(*jargs, **opts)
            twin.write_jobs_device(*jargs)
            model.write(rc.batch)
            fed.write_jobs(case)
            _sync()
            assert (ROW_TEXT in _status(engine)) == (k == 2)
            routed, _ = _check_read(s, case, streams, route)
            assert (2 in routed) == (k != 1), (k, routed)
            _check_export(s, twin, streams, streams.astype(np.uint64), model, fed, k)
            s.sum_device(out)
            _sync()
            assert [bytes(r) for r in out.cpu().numpy()] == [hashlib.sha256(fed.data[i]).digest() for i in range(n)], k
            # between the calls: the other entries, on both sets
            if k == 0:
                both("write_device", *d_og)
                both("write_jobs_device", *_job_args(other))
                for _ in range(2):
                    model.write(og)
                    fed.write(og)
            if k == 1:
                both("write_routed_device", *d_og, **opts)
                model.write(og)
                fed.write(og)
                both("snap_device", out)
                _sync()
                model.snap()
                fed.data = {i: hashlib.sha256(d).digest() for i, d in fed.data.items()}
                assert [bytes(r) for r in out.cpu().numpy()] == [fed.data[i] for i in range(n)]
            _sync()
        assert s.jobs_route_stats()["calls"] == 3 and s.jobs_stats()["calls"] == 1 and s.route_stats()["calls"] == 1
        # the older read-backs are their own entries' last calls, not this entry's
        order, n_valid = s.jobs_order()
        assert np.array_equal(order, R.order(other)[0]) and n_valid == other.k
        assert s.routed_rows()[0].tolist() == [3]                            # `other`'s row of 200 bytes after a snap
        assert _status(engine) == ""


def test_workspace_grows_between_calls_on_two_streams(engine, tile):
    """A small call, one that must grow the set's workspace (jobs past a tile, a larger
    buffer), the small one again, alternating between two caller streams with no host wait
    between them; the sums against hashlib."""
    import torch
    n = 300
    rng = np.random.default_rng(0x6B0)
    hashes = [hashlib.sha256() for _ in range(n)]
    length = [0] * n
    cases = []
    for i, (k, long_bytes) in enumerate(((60, 4 << 10), (2 * tile + 17, 64 << 10), (9, 4 << 10))):
        ids = rng.integers(0, n, k)
        ids[: k // 2] = ids[0]                                               # one stream takes half the jobs: long
        rng.shuffle(ids)
        case = J.Case("growth_%d" % k, n, ids, rng.integers(20, 41, k), 0x6B1 + i)
        cases.append((case, long_bytes))
        tails = [x % 64 for x in length]                                     # before the call
        for j in range(k):
            hashes[int(ids[j])].update(case.chunk(j))
            length[int(ids[j])] += int(case.len[j])
    # the last call's long streams, by the header's rule: 9 jobs of at most 40 bytes, so at most the hot one
    total = np.bincount(case.ids.astype(np.int64), weights=case.len.astype(np.float64), minlength=n).astype(np.int64)
    want_routed = [i for i in range(n) if (tails[i] + int(total[i])) // 64 >= 2]
    assert len(want_routed) <= 1
    args = [_job_args(c) for c, _ in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    with DeviceStreamSet(engine, n) as s:
        _sync()
        for i, (case, long_bytes) in enumerate(cases):
            s.write_jobs_routed_device(*args[i], stream=streams[i % 2], long_blocks=2, max_long=4, long_bytes=long_bytes)
        _sync()
        st = s.jobs_route_stats()
        assert _status(engine) == "" and (st["calls"], st["last_jobs"], st["launches_write"]) == (3, 9, 3)
        order, n_valid, routed, nbytes = s.jobs_route_read()
        last = cases[-1][0]
        assert n_valid == 9 and np.array_equal(order, J.order(last)[0])
        assert routed.tolist() == want_routed
        s.sum_device(out)
        _sync()
        assert [bytes(r) for r in out.cpu().numpy()] == [h.digest() for h in hashes]
        # n_jobs == 0 launches nothing, with or without pointers
        assert engine._lib.msha_dstreams_write_jobs_routed_device(s._h, None, None, None, None, 0, None, None) == L.MSHA_OK
        assert s.jobs_route_stats() == st
        # refused on the host, no stream changed
        before = s.export_state()
        a = args[-1]
        f = engine._lib.msha_dstreams_write_jobs_routed_device
        p = [x.data_ptr() for x in a]
        assert f(s._h, p[0], None, p[2], p[3], 9, None, None) == L.MSHA_ERR_INVALID_ARG
        assert f(s._h, p[0] + 1, p[1], p[2], p[3], 9, None, None) == L.MSHA_ERR_INVALID_ARG
        rc = f(s._h, p[0], p[1], p[2], p[3], (1 << 32) - 1, None, None)
        assert rc == L.MSHA_ERR_INVALID_ARG
        with pytest.raises(MshaError, match="n_jobs must be below"):
            engine._check(rc)
        with pytest.raises(MshaError, match="long_bytes"):
            s.write_jobs_routed_device(*a, long_bytes=16)
        with pytest.raises(MshaError, match="max_long"):
            s.write_jobs_routed_device(*a, max_long=1 << 20)
        assert np.array_equal(s.export_state(), before) and s.jobs_route_stats() == st
        assert _status(engine) == ""


def test_capture(engine, monkeypatch):
    """One call of the size outside capture, then the call plus sum_device captured and
    replayed twice: three appends. A larger call on a capturing stream is refused with the
    workspace text and leaves the capture valid. MSHA_PARTS_TIMING=1 never times a
    captured call."""
    import torch
    rc, rows = M.slots(9)
    case = R.jobs_of(rc, "shuffle")
    larger = R.jobs_of(M.no_long(), "round_robin")
    assert larger.k > case.k and larger.n > case.n
    n = larger.n                                                             # one set takes both, from New()
    case = dataclasses.replace(case, n=n, pre=None, tails={})
    streams = np.arange(n, dtype=np.uint32)
    opts = case.opts()
    jargs, big = _job_args(case), _job_args(larger)
    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    with DeviceStreamSet(engine, n) as s, DeviceStreamSet(engine, n) as twin:
        model, fed = D.Model(n), R.Fed(streams)
        out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
        st = torch.cuda.Stream()
        _sync()
        s.write_jobs_routed_device(*jargs, **opts)                           # the call of that size, timed
        assert s.jobs_route_stats()["last_kernel_ms"] > 0
        _sync()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(st):
            g.capture_begin()
            try:
                with pytest.raises(MshaError, match=WS_TEXT):
                    s.write_jobs_routed_device(*big, stream=st, long_blocks=2, max_long=M.MAX_LONG,
                                               long_bytes=2 * M.LONG_BYTES)
                assert s.jobs_route_stats()["calls"] == 1
                s.write_jobs_routed_device(*jargs, stream=st, **opts)        # the refusal left the capture valid
                ms = s.jobs_route_stats()["last_kernel_ms"]
                s.sum_device(out, stream=st)
            finally:
                g.capture_end()                                              # raises if the capture was invalidated
        _sync()
        assert ms == 0.0 and s.jobs_route_stats()["calls"] == 2
        _, grouped = R.grouped(case, streams)

        def want():
            return [hashlib.sha256(fed.data[i]).digest() for i in range(n)]

        twin.write_jobs_device(*jargs)
        model.write(grouped.batch)
        fed.write_jobs(case)
        _sync()
        _check_export(s, twin, streams, streams.astype(np.uint64), model, fed, "the capture itself ran nothing")
        for times in (2, 3):
            out.zero_()
            _sync()
            g.replay()
            _sync()
            twin.write_jobs_device(*jargs)
            model.write(grouped.batch)
            fed.write_jobs(case)
            _sync()
            assert [bytes(r) for r in out.cpu().numpy()] == want(), times
            _check_export(s, twin, streams, streams.astype(np.uint64), model, fed, times)
        assert _status(engine) == ""
        del g
