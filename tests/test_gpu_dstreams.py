"""Device stream sets on the GPU (msha_dstreams_*, mirbft_amd/csrc/stream_device.hip):
streams whose state, buffer and length live in HBM, written from parts at any byte
offset and summed there. Every expected digest is hashlib's, fed incrementally
(tests/dstream_matrix.py's model), never another path of the engine -- except where a
test is about agreeing with the host StreamSet (interop, long streams), existing and
separately tested code. The batches are the ones the sanitized host program runs
(tests/test_dstream_cpu.py)."""
import hashlib
import random

import numpy as np
import pytest

import dstream_matrix as M
import parts_matrix
from mirbft_amd import DeviceStreamSet, GPUHasher, MshaError, StreamSet
from mirbft_amd import _lib as L

pytestmark = pytest.mark.gpu

BEGIN_TEXT = ("msha_hash_actions_device: action_part_begin decreases (begin[i+1] < begin[i]); "
              "those digests are zero")
ROW_TEXT = "msha_dstreams_*: row out of range"


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


def _out(n):
    import torch
    out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()            # filled (on torch's stream) before a call writes it (on the context's)
    return out


def _sync():
    """The set's calls run on the context's stream, not torch's: wait for the device before
    reading a result through torch or letting an uploaded argument go."""
    import torch
    torch.cuda.synchronize()


def _write(s, batch, rows=None):
    args = [_dev(x) for x in batch] + [None if rows is None else _dev(rows)]
    s.write_device(*args)
    _sync()


def _sum(s, rows=None):
    out = _out(s.n if rows is None else len(rows))
    d_rows = None if rows is None else _dev(np.asarray(rows, dtype=np.uint32))
    s.sum_device(out, rows=d_rows)
    _sync()
    return out.cpu().numpy()


def _bad_rows(got, want):
    return [int(i) for i in np.nonzero((got != want).any(axis=1))[0]]


def _packed(chunks_per_row, rng=None, seed=1):
    """Rows of byte chunks -> a batch on parts_matrix.Arena (every part at its own residue)."""
    ar = parts_matrix.Arena(rng or np.random.default_rng(seed))
    begin, k = [0], 0
    for chunks in chunks_per_row:
        for c in chunks:
            k += 1
            ar.put(c, (5 * k) % 16)
        begin.append(len(ar.off))
    arena, off, ln = ar.arrays(M.SLACK)
    return arena, off, ln, np.array(begin, dtype=np.uint64)


def test_tail_by_append_one_launch(engine):
    """Every buffered tail 0..63 x every appended total 0..130: the tails pre-loaded by one
    write, the appends in one launch of 8,384 lanes; sums, lengths and exported buffers."""
    pre, app, pairs = M.tail_by_append()
    n = len(pairs)
    m = M.Model(n)
    with DeviceStreamSet(engine, n) as s:
        _write(s, pre)
        m.write(pre)
        assert s.lengths().tolist() == [t for t, _ in pairs]
        before = s.stats()
        _write(s, app)
        m.write(app)
        got = _sum(s)
        engine.device_status()
        after = s.stats()
        assert after["launches"] - before["launches"] == 2 and after["writes"] - before["writes"] == 1
        bad = _bad_rows(got, m.sum())
        assert bad == [], (len(bad), [pairs[i] for i in bad[:10]])
        assert s.lengths().tolist() == [t + a for t, a in pairs]
        ex = s.export_state()
        assert ex.shape == (n, L.MSHA_STREAM_STATE_BYTES) and (ex[:, :4] == np.frombuffer(b"sha\x03", np.uint8)).all()
        assert np.array_equal(ex[:, 36:100], m.buffers())               # the buffered bytes, zero past length % 64
        assert np.array_equal(ex[:, 100:108].copy().view(">u8").reshape(-1), m.lengths())


def test_three_rounds(engine):
    """The gather's boundary matrix written three times to the same streams: each round
    starts from the tails the one before left; a sum after each."""
    batch, rounds = M.three_rounds()
    n = batch[3].size - 1
    m = M.Model(n)
    d = [_dev(x) for x in batch]
    with DeviceStreamSet(engine, n) as s:
        for k in range(rounds):
            s.write_device(*d)
            m.write(batch)
            got = _sum(s)
            bad = _bad_rows(got, m.sum())
            assert bad == [], (k, len(bad), bad[:10])
        engine.device_status()
        assert np.array_equal(s.lengths(), m.lengths())


def test_rows_permuted_subset(engine):
    batch, _ = M.three_rounds()
    k = batch[3].size - 1
    n = 2 * k + 3
    rng = np.random.default_rng(21)
    rows = rng.permutation(n)[:k].astype(np.uint32)
    m = M.Model(n)
    with DeviceStreamSet(engine, n) as s:
        seedb = _packed([[rng.bytes(int(rng.integers(0, 100)))] for _ in range(n)], rng)
        _write(s, seedb)                                                # every stream holds something first
        m.write(seedb)
        before = s.export_state()
        _write(s, batch, rows=rows)
        m.write(batch, rows=rows)
        after = s.export_state()
        engine.device_status()
        named = np.zeros(n, dtype=bool)
        named[rows] = True
        assert np.array_equal(after[~named], before[~named])            # byte-identical where not named
        assert _bad_rows(_sum(s), m.sum()) == []
        sub = rng.permutation(n)[:50].astype(np.uint32)                 # sum through rows too
        assert np.array_equal(_sum(s, rows=sub), m.sum(rows=sub))
        assert np.array_equal(s.lengths(sub), m.lengths()[sub])
        # d_row NULL names every stream: n_rows != n is refused on the host
        d = [_dev(x) for x in batch]
        rc = engine._lib.msha_dstreams_write_device(s._h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                                    d[3].data_ptr(), None, k, None)
        assert rc == L.MSHA_ERR_INVALID_ARG
        with pytest.raises(MshaError, match="n_rows must equal n"):
            engine._check(rc)
        out = _out(k)
        assert engine._lib.msha_dstreams_sum_device(s._h, None, k, out.data_ptr(), None) == L.MSHA_ERR_INVALID_ARG
        assert engine._lib.msha_dstreams_write_device(s._h, d[0].data_ptr() + 1, d[1].data_ptr(), d[2].data_ptr(),
                                                      d[3].data_ptr(), _dev(rows).data_ptr(), k,
                                                      None) == L.MSHA_ERR_INVALID_ARG
        assert np.array_equal(s.export_state(), after)                  # the refused calls changed nothing
        engine.device_status()


def test_snap_and_reset(engine):
    rng = np.random.default_rng(31)
    n = 300
    lens = [int(x) for x in rng.integers(0, 200, n)]
    for i, t in enumerate((0, 23, 24, 31, 32, 55, 56, 63, 64, 119, 120)):      # the sum's edges, and 32 more after a snap
        lens[i] = t
    first = _packed([[rng.bytes(x)] for x in lens], rng)
    more = _packed([[rng.bytes(int(x)), rng.bytes(5)] for x in rng.integers(0, 100, n)], rng)
    m = M.Model(n)
    with GPUHasher(engine).new_device_streams(n) as s:
        assert isinstance(s, DeviceStreamSet)
        _write(s, first)
        m.write(first)
        out = _out(n)
        s.snap_device(out)
        _sync()
        want = m.snap()
        assert _bad_rows(out.cpu().numpy(), want) == []
        assert set(s.lengths().tolist()) == {32}
        ex = s.export_state()
        assert np.array_equal(ex[:, 36:68], want) and not ex[:, 68:100].any()
        assert _bad_rows(_sum(s), m.sum()) == []                        # sha256(digest)
        _write(s, more)
        m.write(more)
        assert _bad_rows(_sum(s), m.sum()) == []                        # ... continued
        some = np.arange(0, n, 3, dtype=np.uint32)
        d_some = _dev(some)
        s.reset_device(rows=d_some)
        _sync()
        m.reset(rows=some)
        got = _sum(s)
        assert _bad_rows(got, m.sum()) == [] and got[0].tobytes() == hashlib.sha256(b"").digest()
        assert np.array_equal(s.lengths(), m.lengths())
        s.reset_device()
        assert not s.lengths().any() and (s.export_state()[:, 36:] == 0).all()
        st = s.stats()
        assert (st["writes"], st["sums"], st["snaps"], st["resets"]) == (2, 3, 1, 2) and st["launches"] == 8
        engine.device_status()


def test_checkpoint_chain_in_hbm(engine):
    """NodeState.Apply / Snap (recorder.go:288-359) for 4 nodes x 20 intervals with the
    request digests produced in HBM: digest_batch_device fills a device table, each
    interval's part lists name its 32-byte rows, write_device then snap_device; no digest
    visits the host between the calls."""
    import torch
    rnd = random.Random(11)
    nodes, intervals = 4, 20
    counts = [[rnd.randrange(0, 41) for _ in range(nodes)] for _ in range(intervals)]
    reqs = [b"%d-%d-%d" % (n, i, j) for i in range(intervals) for n in range(nodes) for j in range(counts[i][n])]
    lens = np.array([len(r) for r in reqs], dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)[:-1]]).astype(np.uint64)
    arena = np.zeros(int(offs[-1] + lens[-1]) + M.SLACK, dtype=np.uint8)
    for o, r in zip(offs, reqs):
        arena[int(o): int(o) + len(r)] = np.frombuffer(r, dtype=np.uint8)
    table = torch.zeros(32 * len(reqs) + M.SLACK, dtype=torch.uint8, device="cuda:0")
    _sync()
    engine.digest_batch_device(_dev(arena), _dev(offs), _dev(lens), table)
    part_off = _dev(32 * np.arange(len(reqs), dtype=np.uint64))
    part_len = _dev(np.full(len(reqs), 32, dtype=np.uint64))
    begins = np.concatenate([[0], np.cumsum([c for row in counts for c in row])]).astype(np.uint64)
    outs = _out(nodes * intervals).view(intervals, nodes, 32)
    d_begins = [_dev(begins[nodes * i: nodes * i + nodes + 1]) for i in range(intervals)]
    engine.device_status()                                              # the table is complete (the context's stream)
    with DeviceStreamSet(engine, nodes) as s:
        for i in range(intervals):
            s.write_device(table, part_off, part_len, d_begins[i])
            s.snap_device(outs[i])
        engine.device_status()
        got = outs.cpu().numpy()
        assert s.lengths().tolist() == [32] * nodes
    streams = [hashlib.sha256() for _ in range(nodes)]                  # Hasher.New() (recorder.go:420)
    it = iter(reqs)
    for i in range(intervals):
        for n in range(nodes):
            for _ in range(counts[i][n]):
                streams[n].update(hashlib.sha256(next(it)).digest())    # Apply (:348)
            exp = streams[n].digest()                                   # Snap: Sum(nil) (:298)
            assert got[i, n].tobytes() == exp, (n, i)
            streams[n] = hashlib.sha256(exp)                            # New + Write(CheckpointHash) (:299-300)


def test_interop_with_the_host_set(engine):
    rng = np.random.default_rng(41)
    n = 200
    a = [rng.bytes(int(x)) for x in rng.integers(0, 300, n)]
    b = [rng.bytes(int(x)) for x in rng.integers(0, 300, n)]
    ids = np.arange(n, dtype=np.uint64)
    want = np.frombuffer(b"".join(hashlib.sha256(x + y).digest() for x, y in zip(a, b)), np.uint8).reshape(n, 32)
    ba, bb = _packed([[x] for x in a], rng), _packed([[y] for y in b], rng)
    with StreamSet(engine, n) as host, DeviceStreamSet(engine, n) as dev:
        host.write(ids, a)                                              # host -> device
        dev.import_state(None, host.export_state())
        _write(dev, bb)
        assert _bad_rows(_sum(dev), want) == []
        host.write(ids, b)
        assert np.array_equal(host.export_state(), dev.export_state())  # the same writes: the same bytes
        dev.reset_device()                                              # device -> host
        host.reset()
        _write(dev, ba)
        half = dev.export_state()
        host.import_state(None, half)
        host.write(ids, b)
        assert _bad_rows(host.sum(), want) == []
        # an import through ids: the last entry wins; a wrong magic changes nothing
        dev.import_state([3, 5, 3], np.stack([half[10], half[11], half[12]]))
        assert np.array_equal(dev.export_state([3, 5]), half[[12, 11]])
        wrong = half[:2].copy()
        wrong[1, 0] ^= 1
        with pytest.raises(MshaError, match="magic"):
            dev.import_state([0, 1], wrong)
        with pytest.raises(MshaError, match="out of range"):
            dev.export_state([n])
        assert np.array_equal(dev.export_state([0, 1]), half[:2])
        junk = half[20].copy()
        junk[36 + int(dev.lengths([20])[0]) % 64: 100] = 0xEE           # bytes past length % 64 are ignored
        dev.import_state([20], junk[None])
        assert np.array_equal(dev.export_state([20])[0], half[20])
        engine.device_status()


def test_long_streams(engine):
    """A stream 2^35 + 40 bytes in: the length is 64-bit in the row and in the padding."""
    rng = np.random.default_rng(51)
    state = np.zeros((2, L.MSHA_STREAM_STATE_BYTES), dtype=np.uint8)
    for r, length in enumerate(((1 << 35) + 40, (1 << 32) - 1)):
        state[r, :4] = np.frombuffer(b"sha\x03", np.uint8)
        state[r, 4:36] = np.frombuffer(rng.bytes(32), np.uint8)
        state[r, 36:36 + length % 64] = np.frombuffer(rng.bytes(length % 64), np.uint8)
        state[r, 100:108] = np.frombuffer(int(length).to_bytes(8, "big"), np.uint8)
    chunks = [rng.bytes(100), rng.bytes(100)]
    with StreamSet(engine, 2) as host, DeviceStreamSet(engine, 2) as dev:
        host.import_state(None, state)
        dev.import_state(None, state)
        assert np.array_equal(dev.export_state(), state)
        assert dev.lengths().tolist() == [(1 << 35) + 40, (1 << 32) - 1]
        host.write([0, 1], chunks)
        _write(dev, _packed([[c[:33], c[33:]] for c in chunks], rng))
        assert np.array_equal(_sum(dev), host.sum())
        assert np.array_equal(dev.export_state(), host.export_state())
        assert dev.lengths().tolist() == [(1 << 35) + 140, (1 << 32) + 99]
        engine.device_status()


def test_errors_reported_by_device_status(engine):
    rng = np.random.default_rng(61)
    n = 70
    batch = _packed([[rng.bytes(int(x))] * 2 for x in rng.integers(1, 90, n)], rng)
    rows = rng.permutation(n).astype(np.uint32)
    m = M.Model(n)
    with DeviceStreamSet(engine, n) as s:
        _write(s, batch)
        m.write(batch)
        engine.device_status()
        before = s.export_state()
        bad_begin = batch[3].copy()
        bad_begin[31] = bad_begin[30] - np.uint64(1)                    # row 30 decreases
        bad_rows = rows.copy()
        bad_rows[7] = n                                                 # row 7 names a stream that is not there
        lost = int(rows[7])
        bad = (batch[0], batch[1], batch[2], bad_begin)
        _write(s, bad, rows=bad_rows)
        m.write(bad, rows=bad_rows)
        after = s.export_state()
        for flagged in (lost, int(rows[30])):
            assert np.array_equal(after[flagged], before[flagged])      # unchanged
        assert _bad_rows(_sum(s), m.sum()) == []                        # the valid rows were applied
        with pytest.raises(MshaError) as ei:
            engine.device_status()
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG
        assert str(ei.value).endswith(BEGIN_TEXT + "; and " + ROW_TEXT + " (a d_row entry >= n); no stream was touched "
                                      "and those digests are zero"), str(ei.value)
        engine.device_status()                                          # reported once
        # bit 32 alone: its own text; sum and snap zero the row, reset touches nothing
        got = _sum(s, rows=bad_rows)
        want = m.sum(rows=bad_rows)
        assert not got[7].any() and _bad_rows(got, want) == []
        with pytest.raises(MshaError) as ei:
            engine.device_status()
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG and (": " + ROW_TEXT) in str(ei.value)
        assert "action_part_begin" not in str(ei.value)
        engine.device_status()
        out = _out(n)
        d_bad = _dev(bad_rows)
        s.snap_device(out, rows=d_bad)
        _sync()
        want = m.snap(rows=bad_rows)
        assert not out.cpu().numpy()[7].any() and _bad_rows(out.cpu().numpy(), want) == []
        assert np.array_equal(s.export_state([lost])[0], after[lost])   # the stream the bad row replaced: not snapped
        d_reset = _dev(np.array([n + 5, 0], dtype=np.uint32))
        s.reset_device(rows=d_reset)
        m.reset(rows=[0])
        with pytest.raises(MshaError, match="row out of range"):
            engine.device_status()
        assert _bad_rows(_sum(s), m.sum()) == []
        engine.device_status()


def test_graph_capture_replays_append(engine):
    """write_device + sum_device captured as a linear chain of two kernel nodes: nothing
    runs during the capture, and every replay appends the bytes again."""
    import torch
    rng = np.random.default_rng(71)
    n = 300
    rows_bytes = [[rng.bytes(int(x)) for x in rng.integers(0, 70, int(rng.integers(0, 4)))] for _ in range(n)]
    batch = _packed(rows_bytes, rng)
    d = [_dev(x) for x in batch]
    out = _out(n)
    once = [b"".join(r) for r in rows_bytes]

    def want(times):
        return np.frombuffer(b"".join(hashlib.sha256(x * times).digest() for x in once), np.uint8).reshape(n, 32)

    with DeviceStreamSet(engine, n) as s:
        s.write_device(*d)                                              # the warm call
        s.sum_device(out)
        engine.device_status()
        assert _bad_rows(out.cpu().numpy(), want(1)) == []
        st = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            g.capture_begin()
            try:
                s.write_device(*d, stream=st)
                s.sum_device(out, stream=st)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert s.stats()["launches"] == 4 and s.stats()["last_kernel_ms"] == 0.0
        assert s.lengths().tolist() == [len(x) for x in once]           # the capture itself ran nothing
        for times in (2, 3):
            out.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert _bad_rows(out.cpu().numpy(), want(times)) == [], times
        assert s.lengths().tolist() == [3 * len(x) for x in once]
        engine.device_status()
        del g


def test_timing_is_read_at_each_call(engine, monkeypatch):
    """MSHA_PARTS_TIMING is read by every write and sum, not once in the process: off, on
    and off again inside one process, the digests and the other counters the same each time."""
    rng = np.random.default_rng(72)
    n = 70
    rows_bytes = [[rng.bytes(40)] for _ in range(n)]
    batch = _packed(rows_bytes, rng)
    d = [_dev(x) for x in batch]

    def round_(s, times):
        """One write and one sum, digests and counters checked; the two calls' last_kernel_ms."""
        before = s.stats()
        s.write_device(*d)
        mid = s.stats()
        got = _sum(s)
        after = s.stats()
        engine.device_status()
        want = np.frombuffer(b"".join(hashlib.sha256(r[0] * times).digest() for r in rows_bytes), np.uint8)
        assert _bad_rows(got, want.reshape(n, 32)) == [], times
        assert [after[k] - before[k] for k in ("writes", "sums", "snaps", "resets", "launches")] == [1, 1, 0, 0, 2]
        assert mid["launches"] - before["launches"] == 1 and mid["last_rows"] == after["last_rows"] == n
        return mid["last_kernel_ms"], after["last_kernel_ms"]

    with DeviceStreamSet(engine, n) as s:
        monkeypatch.delenv("MSHA_PARTS_TIMING", raising=False)
        assert round_(s, 1) == (0.0, 0.0)
        monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
        w_ms, s_ms = round_(s, 2)
        assert w_ms > 0 and s_ms > 0
        monkeypatch.delenv("MSHA_PARTS_TIMING")
        assert round_(s, 3) == (0.0, 0.0)
        assert s.lengths().tolist() == [120] * n


def test_timing_never_enters_a_capture(engine, monkeypatch):
    """With MSHA_PARTS_TIMING=1 a write and a sum on a capturing stream are not timed: no
    event is recorded or waited for inside the capture (that would invalidate it), the
    captured calls report 0 ms, and each replay appends what the arena holds by then."""
    import torch
    rng = np.random.default_rng(73)
    n = 300
    rows_bytes = [[rng.bytes(int(x)) for x in rng.integers(0, 70, int(rng.integers(0, 4)))] for _ in range(n)]
    arena, off, ln, begin = _packed(rows_bytes, rng)
    d = [_dev(x) for x in (arena, off, ln, begin)]
    out = _out(n)
    hashes = [hashlib.sha256(b"".join(r)) for r in rows_bytes]

    def want():
        return np.frombuffer(b"".join(h.digest() for h in hashes), np.uint8).reshape(n, 32)

    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    with DeviceStreamSet(engine, n) as s:
        s.write_device(*d)                                              # the warm calls, timed
        assert s.stats()["last_kernel_ms"] > 0
        s.sum_device(out)
        assert s.stats()["last_kernel_ms"] > 0
        engine.device_status()
        assert _bad_rows(out.cpu().numpy(), want()) == []
        st = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            g.capture_begin()
            try:
                s.write_device(*d, stream=st)
                w_ms = s.stats()["last_kernel_ms"]
                s.sum_device(out, stream=st)
            finally:
                g.capture_end()                                         # raises if the capture was invalidated
        torch.cuda.synchronize()
        assert s.stats()["launches"] == 4 and (w_ms, s.stats()["last_kernel_ms"]) == (0.0, 0.0)
        assert s.lengths().tolist() == [len(b"".join(r)) for r in rows_bytes]   # the capture itself ran nothing
        for _ in range(2):
            fresh = rng.integers(0, 256, arena.size, dtype=np.uint8)
            d[0].copy_(_dev(fresh))
            out.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            host = fresh.tobytes()
            for i in range(n):
                for j in range(int(begin[i]), int(begin[i + 1])):
                    hashes[i].update(host[int(off[j]):int(off[j] + ln[j])])
            assert _bad_rows(out.cpu().numpy(), want()) == []
        engine.device_status()
        del g
