"""msha_hash_actions_device on the GPU (k_digest_parts, mirbft_amd/csrc/parts_kernels.hip):
multi-part actions hashed from HBM, parts at any byte offset. Every expected digest is
hashlib's of the joined parts or a committed fixture (tests/golden/actions.json), never
another path of the engine. The shapes are the smallest at which the gather can go
wrong; the boundary matrix is the one the sanitized host program runs
(tests/parts_matrix.py, tests/test_parts_gather.py)."""
import hashlib

import numpy as np
import pytest

import parts_matrix
from mirbft_amd import MshaError, pack_parts
from mirbft_amd import _lib as L

gpu = pytest.mark.gpu

SLACK = L.MSHA_DEVICE_ARENA_SLACK
CAPTURE_MESSAGE = "make one call of this size outside the capture first"


def _sha(parts) -> bytes:
    return hashlib.sha256(b"".join(parts)).digest()


def _want(actions) -> np.ndarray:
    return np.frombuffer(b"".join(_sha(a) for a in actions), dtype=np.uint8).reshape(-1, 32)


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


def _run(engine, arena, off, ln, begin, order=None) -> np.ndarray:
    """One hash_actions_device call on uploaded copies; the digests, after a clean device_status()."""
    import torch
    n = begin.size - 1
    out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    engine.hash_actions_device(_dev(arena), _dev(off), _dev(ln), _dev(begin), out,
                               order=None if order is None else _dev(order))
    engine.device_status()
    return out.cpu().numpy()


def _packed(actions):
    """pack_parts(): parts back to back, hence unaligned; the device contract's slack appended."""
    arena, off, ln, begin = pack_parts(actions)
    return np.concatenate([arena, np.full(SLACK, 0xEE, dtype=np.uint8)]), off, ln, begin


def _bad_rows(got, want):
    return [int(i) for i in np.nonzero((got != want).any(axis=1))[0]]


@gpu
def test_golden_actions_alone_and_together(engine, actions_golden):
    actions = [parts for _, _, parts, _ in actions_golden]
    want = np.frombuffer(b"".join(d for _, _, _, d in actions_golden), dtype=np.uint8).reshape(-1, 32)
    for i, (name, _, parts, digest) in enumerate(actions_golden):       # each alone: n = 1
        got = _run(engine, *_packed([parts]))
        assert got.tobytes() == digest, name
    got = _run(engine, *_packed(actions))
    assert _bad_rows(got, want) == [], [actions_golden[i][0] for i in _bad_rows(got, want)]


@pytest.fixture(scope="module")
def matrix():
    return parts_matrix.boundary_matrix()


@gpu
@pytest.mark.parametrize("reverse", [False, True], ids=["in_order", "order_reversed"])
def test_boundary_matrix_one_launch(engine, matrix, reverse):
    """L = 0..200 cut into 0..6 parts, and both sides of every padding and block edge cut
    in two at every position, all start residues mod 16: one launch (four workgroups);
    again with `order` reversed (lane i hashes action n-1-i, the digest still lands in
    its action's slot)."""
    arena, off, ln, begin, want, seen = matrix
    assert seen == set(range(16))
    n = begin.size - 1
    order = np.arange(n, dtype=np.uint32)[::-1] if reverse else None
    got = _run(engine, arena, off, ln, begin, order=order)
    bad = _bad_rows(got, want)
    assert bad == [], (len(bad), [(i, [int(x) for x in ln[int(begin[i]):int(begin[i + 1])]],
                                   [int(x) % 16 for x in off[int(begin[i]):int(begin[i + 1])]]) for i in bad[:8]])


def _epoch_change_parts(rng, n_p, n_q, new_epoch=7):
    from mirbft_amd.encoding import Checkpoint, EpochChange, SetEntry, epoch_change_hash_data
    cps = [Checkpoint(seq_no=500 * (j + 1), value=rng.bytes(332)) for j in range(2)]
    p = [SetEntry(epoch=int(rng.integers(0, 8)), seq_no=s, digest=rng.bytes(32)) for s in range(n_p)]
    q = [SetEntry(epoch=int(rng.integers(0, 8)), seq_no=s, digest=rng.bytes(32)) for s in range(n_q)]
    return epoch_change_hash_data(EpochChange(new_epoch=new_epoch, checkpoints=cps, p_set=p, q_set=q))


@gpu
def test_divergent_wave(engine):
    """One 64-lane wave whose lanes run very different gathers and block counts: a
    zero-part action, one 5,000-byte part, 300 one-byte parts, parts of 1, 2 and 3 bytes
    at residues 13, 14 and 15 (each straddles a dword, the last a granule), and an
    EpochChange-shaped action. The compression is shared by the lanes that still have
    a block; the others wait."""
    rng = np.random.default_rng(0xD1)
    ar = parts_matrix.Arena(rng)
    begin, actions = [0], []

    def action(pieces, residues):
        for p, r in zip(pieces, residues):
            ar.put(p, r)
        begin.append(len(ar.off))
        actions.append(list(pieces))

    ec = _epoch_change_parts(rng, 9, 5)
    for lane in range(64):
        kind = lane % 5
        if kind == 0:
            action([], [])
        elif kind == 1:
            action([rng.bytes(5000)], [(lane * 3) % 16])
        elif kind == 2:
            action([rng.bytes(1) for _ in range(300)], [(lane + 7 * k) % 16 for k in range(300)])
        elif kind == 3:
            action([rng.bytes(1), rng.bytes(2), rng.bytes(3), rng.bytes(3), rng.bytes(2)], [13, 14, 15, 14, 15])
        else:
            action(ec, [(0 if len(p) == 32 else 8 * (k % 2) if len(p) == 8 else 4) for k, p in enumerate(ec)])
    arena, off, ln = ar.arrays(SLACK)
    got = _run(engine, arena, off, ln, np.array(begin, dtype=np.uint64))
    assert _bad_rows(got, _want(actions)) == []


@gpu
def test_epoch_change_as_the_reference_shapes_it(engine):
    """Eight EpochChange messages from encoding.epoch_change_hash_data (P and Q sets up
    to 40 entries): the big-endian fields live in one region, the digests and checkpoint
    values in another, and two actions share one message's parts."""
    from mirbft_amd.workloads import scatter_parts
    rng = np.random.default_rng(0xEC)
    sizes = [(0, 0), (1, 0), (0, 1), (40, 40), (17, 3), (2, 33), (40, 0), (25, 25)]
    msgs = [_epoch_change_parts(rng, p, q, new_epoch=i + 1) for i, (p, q) in enumerate(sizes)]
    arena, off, ln, begin = scatter_parts(msgs, slack=SLACK)
    # a ninth action over message 3's parts again (the same arena bytes, listed once more)
    lo, hi = int(begin[3]), int(begin[4])
    off = np.concatenate([off, off[lo:hi]])
    ln = np.concatenate([ln, ln[lo:hi]])
    begin = np.concatenate([begin, [begin[-1] + np.uint64(hi - lo)]]).astype(np.uint64)
    want = _want(msgs + [msgs[3]])
    assert {int(x) for x in ln} == {8, 32, 332} and (off[ln == 8] % 16 == 8).any()
    got = _run(engine, arena, off, ln, begin)
    assert _bad_rows(got, want) == []
    assert got[8].tobytes() == got[3].tobytes()


@gpu
def test_overlapping_and_repeated_parts(engine):
    rng = np.random.default_rng(0x0E)
    base = rng.bytes(400)
    arena = np.frombuffer(base + bytes(SLACK), dtype=np.uint8)
    spans = [
        [(0, 100), (50, 100), (99, 3)],                 # overlapping
        [(7, 61), (7, 61), (7, 61)],                    # one part three times
        [(3, 397), (0, 400), (399, 1), (0, 0), (200, 64)],
        [(130, 1)] * 70,                                # one byte, seventy times
    ]
    off = np.array([o for a in spans for o, _ in a], dtype=np.uint64)
    ln = np.array([l for a in spans for _, l in a], dtype=np.uint64)
    begin = np.cumsum([0] + [len(a) for a in spans]).astype(np.uint64)
    want = _want([[base[o:o + l] for o, l in a] for a in spans])
    assert _bad_rows(_run(engine, arena, off, ln, begin), want) == []


@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_grid_edges(engine, n):
    """Workgroups of 256 lanes: one lane, one short of a workgroup, exactly one, one
    over, and four plus one; mixed small lengths, parts packed back to back."""
    rng = np.random.default_rng(n)
    actions = []
    for i in range(n):
        k = int(rng.integers(0, 5))
        actions.append([rng.bytes(int(rng.integers(0, 90))) for _ in range(k)])
    got = _run(engine, *_packed(actions))
    assert _bad_rows(got, _want(actions)) == []


@gpu
def test_parts_past_4gib(engine):
    """Offsets are 64-bit: one action whose parts lie before, across and after the 4 GiB
    line of a 4 GiB + 64 KiB arena. Only the touched bytes are initialised."""
    import torch
    line = 1 << 32
    try:
        arena = torch.empty(line + (64 << 10), dtype=torch.uint8, device="cuda:0")
    except (RuntimeError, MemoryError) as ex:      # torch.cuda.OutOfMemoryError is a RuntimeError
        pytest.skip("no room for a 4 GiB + 64 KiB device arena: %s" % str(ex).splitlines()[0])
    rng = np.random.default_rng(0x46)
    spans = [(line - 1000, 333), (line - 37, 150), (line + 4099, 1), (line - 1, 2), (line + 60000, 5000),
             (line - 64, 64)]
    parts = []
    for o, l in spans:
        b = rng.bytes(l)
        parts.append(b)
        arena[o:o + l] = torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to("cuda:0")
    # later spans overwrite earlier ones where they overlap: read the bytes back
    lo = line - 1024
    window = arena[lo:].cpu().numpy()
    parts = [window[o - lo:o - lo + l].tobytes() for o, l in spans]
    off = np.array([o for o, _ in spans], dtype=np.uint64)
    ln = np.array([l for _, l in spans], dtype=np.uint64)
    begin = np.array([0, len(spans), len(spans) + 0], dtype=np.uint64)       # and a zero-part action after it
    out = torch.full((2, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    engine.hash_actions_device(arena, _dev(off), _dev(ln), _dev(begin), out)
    engine.device_status()
    got = out.cpu().numpy()
    del arena
    torch.cuda.empty_cache()
    assert got[0].tobytes() == _sha(parts)
    assert got[1].tobytes() == _sha([])


@gpu
def test_decreasing_begin_is_flagged_and_zeroed(engine):
    """The host cannot see begin[]: a decreasing pair zeroes that action's digest (never
    a wrong one), every other digest is right, device_status() raises
    MSHA_ERR_INVALID_ARG once, and the next good call is exact."""
    import torch
    rng = np.random.default_rng(0xBE)
    actions = [[rng.bytes(int(rng.integers(1, 80))) for _ in range(3)] for _ in range(300)]
    arena, off, ln, begin = _packed(actions)
    bad = begin.copy()
    bad[131] = begin[130] - np.uint64(2)        # action 130: begin[131] < begin[130]; action 131 gains parts
    acts_bad = list(actions)
    acts_bad[131] = actions[129][1:] + actions[130] + actions[131]      # parts 388..395 (three an action)
    out = torch.full((300, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    engine.hash_actions_device(_dev(arena), _dev(off), _dev(ln), _dev(bad), out)
    with pytest.raises(MshaError) as ei:
        engine.device_status()
    assert ei.value.code == L.MSHA_ERR_INVALID_ARG and "action_part_begin" in str(ei.value)
    engine.device_status()                      # reported once, then clean
    got = out.cpu().numpy()
    assert not got[130].any()
    want = _want(acts_bad)
    assert _bad_rows(got, want) == [130]
    assert _bad_rows(_run(engine, arena, off, ln, begin), _want(actions)) == []


@gpu
def test_capturable_into_a_graph(engine):
    """One launch on the caller's stream, no library stream, no host wait: the call
    captures into a HIP graph (nothing runs during the capture) and the replay hashes
    what the arena holds by then."""
    import torch
    rng = np.random.default_rng(0x6A)
    actions = [[rng.bytes(int(rng.integers(0, 90))) for _ in range(int(rng.integers(0, 5)))] for _ in range(300)]
    arena, off, ln, begin = _packed(actions)
    d_arena, d_off, d_ln, d_begin = _dev(arena), _dev(off), _dev(ln), _dev(begin)
    out = torch.zeros((300, 32), dtype=torch.uint8, device="cuda:0")
    engine.hash_actions_device(d_arena, d_off, d_ln, d_begin, out)
    engine.device_status()
    out.zero_()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            engine.hash_actions_device(d_arena, d_off, d_ln, d_begin, out, stream=s)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert not out.any()
    fresh = rng.integers(0, 256, arena.size, dtype=np.uint8)
    d_arena.copy_(_dev(fresh))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    engine.device_status()
    host = fresh.tobytes()
    want = _want([[host[int(off[j]):int(off[j] + ln[j])] for j in range(int(begin[i]), int(begin[i + 1]))]
                  for i in range(300)])
    assert _bad_rows(out.cpu().numpy(), want) == []


@gpu
def test_parts_stats_count_calls_actions_and_launches(engine):
    before = engine.parts_stats()
    rng = np.random.default_rng(5)
    for n in (3, 70):
        actions = [[rng.bytes(10), rng.bytes(9)] for _ in range(n)]
        assert _bad_rows(_run(engine, *_packed(actions)), _want(actions)) == []
    after = engine.parts_stats()
    assert after["calls"] - before["calls"] == 2
    assert after["actions"] - before["actions"] == 73
    assert after["launches"] - before["launches"] == 2
    assert after["last_lanes"] == 70
    assert after["last_kernel_ms"] == 0.0       # measured only under MSHA_PARTS_TIMING=1


def _timed_call(engine, actions):
    """One call over `actions`, its digests checked; the counters it moved and its last_kernel_ms."""
    before = engine.parts_stats()
    assert _bad_rows(_run(engine, *_packed(actions)), _want(actions)) == []
    after = engine.parts_stats()
    assert [after[k] - before[k] for k in ("calls", "actions", "launches")] == [1, len(actions), 1]
    assert after["last_lanes"] == len(actions)
    return after["last_kernel_ms"]


@gpu
def test_timing_is_read_at_each_call(engine, monkeypatch):
    """MSHA_PARTS_TIMING is read by every call, not once in the process: off, on and off
    again inside one process, the digests and the other counters the same each time."""
    rng = np.random.default_rng(0x71)
    actions = [[rng.bytes(40), rng.bytes(41)] for _ in range(70)]
    monkeypatch.delenv("MSHA_PARTS_TIMING", raising=False)
    assert _timed_call(engine, actions) == 0.0
    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    assert _timed_call(engine, actions) > 0
    monkeypatch.delenv("MSHA_PARTS_TIMING")
    assert _timed_call(engine, actions) == 0.0


@gpu
def test_timing_never_enters_a_capture(engine, monkeypatch):
    """With MSHA_PARTS_TIMING=1 a call on a capturing stream is not timed: no event is
    recorded or waited for inside the capture (that would invalidate it), the captured
    call reports 0 ms, and the graph replays as without the variable."""
    import torch
    rng = np.random.default_rng(0x72)
    actions = [[rng.bytes(int(rng.integers(0, 90))) for _ in range(int(rng.integers(0, 5)))] for _ in range(300)]
    arena, off, ln, begin = _packed(actions)
    d_arena, d_off, d_ln, d_begin = _dev(arena), _dev(off), _dev(ln), _dev(begin)
    out = torch.zeros((300, 32), dtype=torch.uint8, device="cuda:0")
    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    engine.hash_actions_device(d_arena, d_off, d_ln, d_begin, out)       # the warm call, timed
    engine.device_status()
    assert engine.parts_stats()["last_kernel_ms"] > 0
    assert _bad_rows(out.cpu().numpy(), _want(actions)) == []
    out.zero_()
    before = engine.parts_stats()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            engine.hash_actions_device(d_arena, d_off, d_ln, d_begin, out, stream=s)
        finally:
            g.capture_end()                                              # raises if the capture was invalidated
    torch.cuda.synchronize()
    after = engine.parts_stats()
    assert after["calls"] - before["calls"] == 1 and after["launches"] - before["launches"] == 1
    assert after["last_lanes"] == 300 and after["last_kernel_ms"] == 0.0
    assert not out.any()
    for _ in range(2):
        fresh = rng.integers(0, 256, arena.size, dtype=np.uint8)
        d_arena.copy_(_dev(fresh))
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        engine.device_status()
        host = fresh.tobytes()
        want = _want([[host[int(off[j]):int(off[j] + ln[j])] for j in range(int(begin[i]), int(begin[i + 1]))]
                      for i in range(300)])
        assert _bad_rows(out.cpu().numpy(), want) == []
    del g


@gpu
def test_capture_without_a_warm_call_fails_cleanly():
    """A fresh context has no error word and may not allocate one while the stream is
    being captured: MSHA_ERR_INVALID_ARG and the documented message, the capture ends
    empty, and the same call outside capture then works."""
    import torch
    from mirbft_amd import Engine
    rng = np.random.default_rng(0x6C)
    actions = [[rng.bytes(40), rng.bytes(41)] for _ in range(70)]
    arena, off, ln, begin = _packed(actions)
    d = [_dev(x) for x in (arena, off, ln, begin)]
    out = torch.zeros((70, 32), dtype=torch.uint8, device="cuda:0")
    with Engine(1) as eng:
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(MshaError) as ei:
                    eng.hash_actions_device(*d, out, stream=s)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG and CAPTURE_MESSAGE in str(ei.value)
        assert "msha_hash_actions_device" in str(ei.value)
        assert not out.any() and eng.parts_stats()["calls"] == 0
        eng.hash_actions_device(*d, out)
        eng.device_status()
        assert _bad_rows(out.cpu().numpy(), _want(actions)) == []
