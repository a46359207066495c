"""msha_dstreams_write_jobs_device on the GPU (mirbft_amd/csrc/stream_jobs.hip): jobs in
call order, grouped by stream inside the call. Every case (tests/dstream_jobs_matrix.py)
is held against three things that do not come from the code under test: the job order
against numpy's stable argsort, the touched streams' digests against hashlib, and the
whole exported state (108 bytes a stream) against a second set fed by the existing
write_device with the host's CSR. Streams no job names must export what they did before."""
import hashlib

import numpy as np
import pytest

import dstream_jobs_matrix as J
from mirbft_amd import DeviceStreamSet, MshaError
from mirbft_amd import _lib as L

pytestmark = pytest.mark.gpu

ROW_TEXT = "msha_dstreams_*: row out of range (a d_row entry >= n); no stream was touched and those digests are zero"


def _dev(a: np.ndarray):
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
    """The set's calls run on the context's stream, not torch's."""
    import torch
    torch.cuda.synchronize()


def _sum(s, rows):
    import torch
    out = torch.full((len(rows), 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_rows = _dev(np.asarray(rows, dtype=np.uint32))
    _sync()
    s.sum_device(out, rows=d_rows)
    _sync()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def tile(engine):
    with DeviceStreamSet(engine, 1) as s:
        st = s.jobs_stats()
    assert st["tile_jobs"] >= 512 and st["calls"] == 0                  # valid from create
    return int(st["tile_jobs"])


def _job_args(case):
    return [_dev(case.arena), _dev(case.ids), _dev(case.off), _dev(case.len)]


def _watched(case, touched):
    """Streams whose state is compared before and after: all of a small set; of a large
    one the touched streams, their neighbours and a spread of others."""
    if case.n <= 70000:
        return np.arange(case.n, dtype=np.uint64)
    t = touched.astype(np.int64)
    near = np.concatenate([t, t - 1, t + 1, np.linspace(0, case.n - 1, 500).astype(np.int64)])
    return np.unique(near[(near >= 0) & (near < case.n)]).astype(np.uint64)


def _run_case(engine, case, passes=None, invalid=False):
    perm, n_valid = J.order(case)
    rows, g_off, g_len, g_begin = J.grouped(case)
    want_rows, want = J.digests(case)
    assert np.array_equal(rows, want_rows)
    watch = _watched(case, rows)
    touched = np.isin(watch, rows.astype(np.uint64))
    with DeviceStreamSet(engine, case.n) as s, DeviceStreamSet(engine, case.n) as ref:
        seed = J.seed_batch(case)
        if seed is not None:
            args = [_dev(x) for x in seed]
            s.write_device(*args)
            ref.write_device(*args)
            _sync()
        before = s.export_state(watch)
        old = s.stats()
        jargs = _job_args(case)
        s.write_jobs_device(*jargs)
        _sync()
        order, got_valid = s.jobs_order()
        assert got_valid == n_valid
        assert np.array_equal(order, perm), np.nonzero(order != perm)[0][:10]
        st = s.jobs_stats()
        p = (case.n.bit_length() + 7) // 8
        assert passes is None or p == passes
        assert (st["calls"], st["jobs"], st["last_jobs"], st["last_passes"]) == (1, case.k, case.k, p)
        assert (st["launches_sort"], st["launches_rows"], st["launches_write"]) == (3 * p, 2, 1)
        assert s.stats() == old                                         # the set's other counters count none of it
        if invalid:
            with pytest.raises(MshaError) as ei:
                engine.device_status()
            assert ei.value.code == L.MSHA_ERR_INVALID_ARG and str(ei.value).endswith(ROW_TEXT), str(ei.value)
        engine.device_status()                                          # clean, or reported once
        if rows.size:
            ref.write_device(_dev(case.arena), _dev(g_off), _dev(g_len), _dev(g_begin), rows=_dev(rows))
            _sync()
        after = s.export_state(watch)
        assert np.array_equal(after, ref.export_state(watch))           # all 108 bytes, against write_device
        assert np.array_equal(after[~touched], before[~touched])        # no job names them: bit-identical
        if rows.size:
            got = _sum(s, rows)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert bad.size == 0, (case.name, len(bad), rows[bad][:10])
        engine.device_status()


def test_order(engine):
    _run_case(engine, J.order_case(), passes=1)


@pytest.mark.parametrize("n,passes", J.PASS_EDGES)
def test_pass_edges(engine, n, passes):
    _run_case(engine, J.pass_edge_case(n), passes=passes)


def test_tile_edges(engine, tile):
    for case in J.tile_edge_cases(tile):
        _run_case(engine, case, passes=1)


def test_one_stream(engine, tile):
    _run_case(engine, J.one_stream_case(tile), passes=1)


def test_all_distinct(engine):
    for case in J.distinct_cases():
        _run_case(engine, case, passes=2)


def test_skew_with_invalid_ids(engine):
    _run_case(engine, J.skew_case(), passes=2, invalid=True)


def test_recorder_shape(engine):
    """NodeState.Apply's order (recorder.go:333-359): 20 digests, each written by all 512
    nodes before the next (job d n + s), in two calls, then snap_device. The chain is
    hashlib's."""
    import torch
    n, digs = 512, 20
    rng = np.random.default_rng(801)
    table = rng.integers(0, 256, n * digs * 32 + J.SLACK, dtype=np.uint8)
    ids = np.tile(np.arange(n, dtype=np.uint32), digs)
    off = 32 * np.arange(n * digs, dtype=np.uint64)
    ln = np.full(n * digs, 32, dtype=np.uint64)
    half = n * (digs // 2)
    d_table = _dev(table)
    with DeviceStreamSet(engine, n) as s:
        for lo, hi in ((0, half), (half, n * digs)):
            s.write_jobs_device(d_table, _dev(ids[lo:hi]), _dev(off[lo:hi]), _dev(ln[lo:hi]))
            _sync()
        out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
        _sync()
        s.snap_device(out)
        _sync()
        engine.device_status()
        got = out.cpu().numpy()
        rows = table[: n * digs * 32].reshape(digs, n, 32)
        for node in range(n):
            want = hashlib.sha256(rows[:, node].tobytes()).digest()
            assert got[node].tobytes() == want, node
        assert set(s.lengths().tolist()) == {32}
        again = _sum(s, np.arange(n))
        assert again[7].tobytes() == hashlib.sha256(got[7].tobytes()).digest()
        st = s.jobs_stats()
        assert (st["calls"], st["jobs"], st["last_passes"]) == (2, n * digs, 2)


def test_workspace_growth(engine, tile):
    """Small, large, small again on one set; k = 0 launches nothing."""
    rng = np.random.default_rng(901)
    n = 300
    hashes = [hashlib.sha256() for _ in range(n)]
    with DeviceStreamSet(engine, n) as s:
        for k in (50, 5 * tile + 17, 9):
            ids = rng.integers(0, n, k)
            case = J.Case("growth_%d" % k, n, ids, rng.integers(0, 41, k), 902 + k)
            s.write_jobs_device(*_job_args(case))
            _sync()
            order, n_valid = s.jobs_order()
            assert n_valid == k and np.array_equal(order, J.order(case)[0])
            for j in range(k):
                hashes[int(ids[j])].update(case.chunk(j))
        st = s.jobs_stats()
        assert (st["calls"], st["last_jobs"], st["launches_write"]) == (3, 9, 3)
        empty = J.Case("none", n, [], [], 903)
        s.write_jobs_device(*_job_args(empty))
        i32 = _dev(np.zeros(0, dtype=np.uint32))
        assert engine._lib.msha_dstreams_write_jobs_device(s._h, None, None, None, None, 0, None) == L.MSHA_OK
        assert s.jobs_stats() == st and i32.numel() == 0
        got = _sum(s, np.arange(n))
        want = np.frombuffer(b"".join(h.digest() for h in hashes), np.uint8).reshape(n, 32)
        assert np.array_equal(got, want)
        # refused on the host, no stream changed: a null pointer, an arena off its alignment, too many jobs
        before = s.export_state()
        a = _job_args(case)
        f = engine._lib.msha_dstreams_write_jobs_device
        assert f(s._h, a[0].data_ptr(), None, a[2].data_ptr(), a[3].data_ptr(), 9, None) == L.MSHA_ERR_INVALID_ARG
        assert f(s._h, a[0].data_ptr() + 1, a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), 9,
                 None) == L.MSHA_ERR_INVALID_ARG
        rc = f(s._h, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), (1 << 32) - 1, None)
        assert rc == L.MSHA_ERR_INVALID_ARG
        with pytest.raises(MshaError, match="n_jobs must be below"):
            engine._check(rc)
        assert np.array_equal(s.export_state(), before) and s.jobs_stats() == st
        engine.device_status()


def test_capture(engine, monkeypatch):
    """A captured call on a fresh set is refused (its workspace cannot grow there); after
    one call of that size outside the capture, jobs + sum capture as a chain of kernel
    nodes and every replay appends again. MSHA_PARTS_TIMING=1 times the call outside
    capture and never inside."""
    import torch
    rng = np.random.default_rng(951)
    n, k = 200, 3000
    ids = rng.integers(0, n, k)
    case = J.Case("capture", n, ids, rng.integers(0, 41, k), 952)
    once = [b"".join(case.chunk(j) for j in np.nonzero(ids == s_)[0]) for s_ in range(n)]
    a = _job_args(case)
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    _sync()

    def want(times):
        return np.frombuffer(b"".join(hashlib.sha256(x * times).digest() for x in once), np.uint8).reshape(n, 32)

    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    with DeviceStreamSet(engine, n) as s:
        st = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            g.capture_begin()
            try:
                with pytest.raises(MshaError, match="outside the capture first"):
                    s.write_jobs_device(*a, stream=st)
                s.sum_device(out, stream=st)                            # the refusal left the capture valid
            finally:
                g.capture_end()
        del g
        torch.cuda.synchronize()
        assert s.jobs_stats()["calls"] == 0 and not s.lengths().any()
        s.write_jobs_device(*a)                                         # the call of that size, timed
        assert s.jobs_stats()["last_kernel_ms"] > 0
        s.sum_device(out)
        engine.device_status()
        assert np.array_equal(out.cpu().numpy(), want(1))
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            g.capture_begin()
            try:
                s.write_jobs_device(*a, stream=st)
                ms = s.jobs_stats()["last_kernel_ms"]
                s.sum_device(out, stream=st)
            finally:
                g.capture_end()                                         # raises if the capture was invalidated
        torch.cuda.synchronize()
        assert ms == 0.0 and s.jobs_stats()["calls"] == 2
        assert s.lengths().tolist() == [len(x) for x in once]           # the capture itself ran nothing
        for times in (2, 3):
            out.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy(), want(times)), times
        assert s.lengths().tolist() == [3 * len(x) for x in once]
        monkeypatch.delenv("MSHA_PARTS_TIMING")
        s.write_jobs_device(*a)
        assert s.jobs_stats()["last_kernel_ms"] == 0.0
        engine.device_status()
        del g
