"""msha_group_digests_device on the GPU (mirbft_amd/csrc/group.hip): digests grouped by
value, the groups numbered in order of first occurrence, everything left in device memory.
Every case compares first, group, members, the two group arrays (all sentinel-filled
before the call, so an entry that is not written, or one written past `listed`, shows),
the five result words and a guard word on each side of every array with
tests/group_matrix.py's numpy oracle, written from the header. Shapes are the smallest at
which each piece can go wrong: the wave (64), tile and scan-chunk edges, and a forced home
position for the probe chain and its wrap-around."""
import hashlib

import numpy as np
import pytest

import group_matrix as M
from mirbft_amd import _lib as L

gpu = pytest.mark.gpu

GUARD32 = 0x5A5A5A5A
CAPTURE_MESSAGE = "make one call of this size outside the capture first"
LAUNCHES = 6                    # init, insert, resolve, scan, rank, fill (include/mirsha.h)


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


_SIDE = []


def _side():
    """One side stream of torch's for the whole module."""
    import torch
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[0]


def _guarded(count):
    """count sentinel entries with a guard word on each side."""
    import torch
    t = torch.from_numpy(np.full(count + 2, M.SENTINEL, np.uint32).view(np.int32)).to("cuda:0")
    t[0] = t[-1] = GUARD32
    return t


class Call:
    """One group_digests_device call on uploaded copies of a case's arrays. Every output
    is the inside of a buffer with a guard word on each side."""

    def __init__(self, engine, case, run=True, members=True):
        import torch
        self.engine, self.case = engine, case
        self.host = case.digests()
        self.digests = _dev(self.host)
        self.scope = None if case.scope is None else _dev(case.scope)
        n, cap = case.n, case.group_cap
        self.full = [_guarded(n), _guarded(n), _guarded(n) if members else None, _guarded(cap), _guarded(cap)]
        self.result = torch.full((5,), -1, dtype=torch.int64, device="cuda:0")
        if run:
            self.run()

    def prefill(self):
        for t in self.full:
            if t is not None:
                t[1:-1] = int(np.uint32(M.SENTINEL).view(np.int32))
        self.result.fill_(-1)

    def run(self, stream=None):
        """On `stream`, or (None) on a side stream of torch's that is waited for, with
        everything torch did before waited for first."""
        import torch
        st = _side() if stream is None else stream
        if stream is None:
            torch.cuda.synchronize()
        n, cap = self.case.n, self.case.group_cap
        first, group, members, gf, gc = self.full
        self.engine.group_digests_device(
            self.digests, first[1:1 + n], group[1:1 + n], self.result, scope=self.scope,
            members=None if members is None else members[1:1 + n],
            group_first=gf[1:1 + cap] if cap else None, group_count=gc[1:1 + cap] if cap else None, stream=st)
        if stream is None:
            st.synchronize()

    def read(self):
        out = []
        for name, t in zip(("first", "group", "members", "group_first", "group_count"), self.full):
            if t is None:
                out.append(None)
                continue
            a = t.cpu().numpy().view(np.uint32)
            assert a[0] == GUARD32 == a[-1], "an entry beside %s was written" % name
            out.append(a[1:-1].copy())
        return tuple(out) + (tuple(int(x) for x in self.result.cpu().tolist()),)

    def want(self):
        return M.oracle(self.host, self.case.scope, self.case.group_cap)

    def check(self, want=None):
        want = self.want() if want is None else want
        got = self.read()
        print("%s: result %s, expected %s" % (self.case.name, got[5], want[5]))
        assert M.problems(want, got) == [], self.case.name
        return got


def _forced(monkeypatch, case):
    home = case.force_home()
    if home is None:
        monkeypatch.delenv("MSHA_GROUP_FORCE_HOME", raising=False)
    else:
        monkeypatch.setenv("MSHA_GROUP_FORCE_HOME", str(home))


@gpu
def test_stats_of_a_fresh_context():
    from mirbft_amd import Engine
    with Engine(1) as fresh:
        s = fresh.group_stats()
        assert s == {"calls": 0, "digests": 0, "launches": 0, "table_slots": 0, "last_kernel_ms": 0.0}


@gpu
@pytest.mark.parametrize("k", range(len(M.sizes())))
def test_sizes_and_patterns(engine, k):
    """Every size with every pattern: all distinct, one group, two groups alternating,
    mirrored pairs, a leader that is the last slot, random draws from n / 10 rows."""
    n = M.sizes()[k]
    cases = M.size_cases(n)
    assert {c.name.split("_", 1)[1] for c in cases} == {"distinct", "one", "two", "mirrored", "last_leader", "random"}
    for c in cases:
        got = Call(engine, c).check()
        assert engine.group_stats()["table_slots"] == M.capacity(n)
        if c.name.endswith("_one"):
            assert got[5] == (n, 1, 1, n, 0)
        if c.name.endswith("_distinct"):
            assert got[5] == (n, n, min(n, c.group_cap), 1, 0)
    engine.device_status()


@gpu
@pytest.mark.parametrize("b", range(32))
def test_whole_digest_is_compared(engine, b):
    """n = 65, slot 40 holds slot 3's row except for byte b: two groups, where a compare
    that left byte b out would see one."""
    c = M.byte_cases()[b]
    assert c.flips == [(40, b)]
    first, group, members, _, _, res = Call(engine, c).check()
    assert res == (65, 65, 16, 1, 0) and first[40] == 40 and group[40] == 40 and members[3] == members[40] == 1


@gpu
def test_scopes(engine):
    """One digest under three scopes gives three groups; scopes that differ in bit 31
    alone differ; d_scope NULL answers as all-zero scopes do."""
    three, bit31, zero, null = M.scope_cases()
    assert Call(engine, three).check()[5] == (96, 3, 3, 32, 0)
    assert Call(engine, bit31).check()[5] == (96, 2, 2, 48, 0)
    a, b = Call(engine, zero).check(), Call(engine, null).check()
    assert M.problems(a, b) == []


@gpu
@pytest.mark.parametrize("k", range(5))
def test_group_caps(engine, k):
    """group_cap 0 (both arrays NULL), 1, groups - 1, groups, groups + 1. Entries at and
    past listed keep the sentinel."""
    c = M.cap_cases()[k]
    _, _, _, gf, gc, res = Call(engine, c).check()
    assert res[1] == M.CAP_GROUPS and res[2] == min(res[1], c.group_cap)
    assert (gf[res[2]:] == M.SENTINEL).all() and (gc[res[2]:] == M.SENTINEL).all()
    assert np.all(np.diff(gf[:res[2]].astype(np.int64)) > 0)            # leaders ascend: first occurrence order


@gpu
def test_without_members(engine):
    """d_members NULL: everything else as with it."""
    c = M.cap_cases()[3]
    got = Call(engine, c, members=False).check()
    assert got[2] is None and got[5][1] == M.CAP_GROUPS


@gpu
@pytest.mark.parametrize("k", range(4))
def test_probe_chain_and_wrap_around(engine, monkeypatch, k):
    """n = 300 with every key's home forced to 0, and to capacity - 2 so that the chain
    runs over the table's end: 300 distinct keys, and 40 rows with duplicates."""
    c = M.probe_cases()[k]
    assert c.force_home() in (0, M.capacity(300) - 2)
    _forced(monkeypatch, c)
    Call(engine, c).check()
    monkeypatch.delenv("MSHA_GROUP_FORCE_HOME")
    Call(engine, c).check()                                                # and as the hash places them
    engine.device_status()


@gpu
def test_seed_changes_no_byte(engine, monkeypatch):
    """One random case under two values of MSHA_GROUP_SEED and under the context's own."""
    c = M.seed_case()
    want = M.case_oracle(c)
    outs = []
    for seed in ("1", "0xFEDCBA9876543210", None):
        if seed is None:
            monkeypatch.delenv("MSHA_GROUP_SEED")
        else:
            monkeypatch.setenv("MSHA_GROUP_SEED", seed)
        outs.append(Call(engine, c).check(want))
    assert M.problems(outs[0], outs[1]) == [] and M.problems(outs[0], outs[2]) == []


@gpu
def test_context_stream(engine):
    """stream NULL: the context's own stream."""
    import torch
    c = Call(engine, M.seed_case(), run=False)
    n, cap = c.case.n, c.case.group_cap
    torch.cuda.synchronize()
    engine.group_digests_device(c.digests, c.full[0][1:1 + n], c.full[1][1:1 + n], c.result, scope=c.scope,
                                members=c.full[2][1:1 + n], group_first=c.full[3][1:1 + cap],
                                group_count=c.full[4][1:1 + cap])
    engine.device_status()
    torch.cuda.synchronize()
    c.check()


@gpu
def test_host_refusals(engine):
    """Each refusal is MSHA_ERR_INVALID_ARG with its text and launches nothing. n == 0 is
    OK, launches nothing and leaves d_result as it was."""
    import torch
    c = Call(engine, M.Case("refusals", (np.arange(70) % 7).astype(np.uint32)), run=False)
    lib, ctx = engine._lib, engine._ctx
    dig, res = c.digests.data_ptr(), c.result.data_ptr()
    first, group, members, gf, gc = (t.data_ptr() + 4 for t in c.full)
    bad = L.MSHA_ERR_INVALID_ARG
    before = engine.group_stats()
    f = lib.msha_group_digests_device
    torch.cuda.synchronize()
    for args in ((None, 70, None, first, group, members, gf, gc, 16, res),
                 (dig, 70, None, None, group, members, gf, gc, 16, res),
                 (dig, 70, None, first, None, members, gf, gc, 16, res),
                 (dig, 70, None, first, group, members, gf, gc, 16, None)):
        assert f(ctx, *args, None) == bad
        assert b"msha_group_digests_device: null pointer" in lib.msha_last_error(ctx)
    assert f(ctx, dig + 8, 69, None, first, group, members, gf, gc, 16, res, None) == bad
    assert b"msha_group_digests_device: d_digests must be 16-byte aligned" in lib.msha_last_error(ctx)
    assert f(ctx, dig, (1 << 30) + 1, None, first, group, members, gf, gc, 16, res, None) == bad
    assert b"n must be at most 2^30" in lib.msha_last_error(ctx)
    for a, b in ((None, gc), (gf, None)):
        assert f(ctx, dig, 70, None, first, group, members, a, b, 16, res, None) == bad
        assert b"d_group_first or d_group_count is null with group_cap > 0" in lib.msha_last_error(ctx)
    assert f(ctx, dig, 0, None, first, group, members, gf, gc, 16, res, None) == L.MSHA_OK
    assert f(ctx, None, 0, None, None, None, None, None, None, 0, None, None) == L.MSHA_OK
    assert engine.group_stats() == before           # nothing was launched or counted
    engine.device_status()
    torch.cuda.synchronize()
    got = c.read()
    assert got[5] == (-1,) * 5 and all((a == M.SENTINEL).all() for a in got[:5])
    # group_cap 0 with NULL arrays and without d_members is a good call
    assert f(ctx, dig, 70, None, first, group, None, None, None, 0, res, None) == L.MSHA_OK
    torch.cuda.synchronize()
    assert tuple(c.result.cpu().tolist()) == (70, 7, 0, 10, 0)


@gpu
def test_capturable_into_a_graph(engine):
    """After a warm call the call captures into a HIP graph on a side stream (six launches
    counted for the capture; nothing runs during it), and each replay groups what the
    arrays hold by then."""
    import torch
    S = M.scan_slots()
    n = S + 1
    rng = np.random.default_rng(0x62A9)
    c = Call(engine, M.Case("graph", rng.integers(0, 1000, n).astype(np.uint32)))    # the warm call
    c.check()
    torch.cuda.synchronize()
    c.prefill()
    before = engine.group_stats()["launches"]
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            c.run(stream=s)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert engine.group_stats()["launches"] == before + LAUNCHES
    assert (c.result == -1).all() and (c.full[0][1:-1] == int(np.uint32(M.SENTINEL).view(np.int32))).all()
    groups = []
    for rows in (5, 70000):
        fresh = M.base_rows(rng.integers(0, rows, n)).reshape(-1)          # the inputs are rewritten
        c.host = fresh
        c.digests.copy_(_dev(fresh))
        c.prefill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        groups.append(c.check()[5][1])
    assert groups[0] == 5 and groups[1] > 30000
    engine.device_status()


@gpu
def test_capture_on_a_fresh_context_fails_cleanly():
    """A fresh context has neither its error word nor a workspace, and may allocate
    neither while the stream is being captured: MSHA_ERR_INVALID_ARG and the documented
    message; the same call outside the capture then works, and a larger one is refused
    in a capture again (the workspace would have to grow)."""
    import torch
    from mirbft_amd import Engine, MshaError
    with Engine(1) as eng:
        c = Call(eng, M.Case("fresh", (np.arange(300) % 11).astype(np.uint32)), run=False)
        big = Call(eng, M.Case("fresh_big", (np.arange(5000) % 13).astype(np.uint32)), run=False)
        for call, calls_before in ((c, 0), (big, 1)):
            s = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.capture_begin()
                try:
                    with pytest.raises(MshaError) as ei:
                        call.run(stream=s)
                finally:
                    g.capture_end()
            torch.cuda.synchronize()
            assert ei.value.code == L.MSHA_ERR_INVALID_ARG and CAPTURE_MESSAGE in str(ei.value)
            assert eng.group_stats()["calls"] == calls_before and (call.result == -1).all()
            call.run()
            call.check()


@gpu
def test_dedupe_then_digest_of_digests(engine):
    """50 batches of 20 digests drawn from 100 distinct ones: dedupe_digests_device's
    table and idx go to digest_of_digests_device as they are, and every batch's digest is
    hashlib's over the batch's raw concatenation."""
    import torch
    from mirbft_amd import GPUHasher, dedupe_digests_device
    rng = np.random.default_rng(0xDED0)
    pool = rng.integers(0, 256, (100, 32), dtype=np.uint8)
    pick = rng.integers(0, 100, 1000)
    raw = pool[pick]                                                       # [1000, 32]: 50 batches of 20
    hasher = GPUHasher(engine=engine)
    table, idx = dedupe_digests_device(hasher, _dev(raw.reshape(-1)))
    distinct = len(set(pick.tolist()))
    assert tuple(table.shape) == (distinct, 32) and idx.dtype == torch.int32 and idx.numel() == 1000
    assert np.array_equal(table.cpu().numpy()[idx.cpu().numpy()], raw)
    order = list(dict.fromkeys(pick.tolist()))                             # first occurrence order
    assert np.array_equal(table.cpu().numpy(), pool[order])
    begin = _dev(np.arange(0, 1001, 20, dtype=np.uint64))
    out = torch.empty(32 * 50, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    engine.digest_of_digests_device(table.reshape(-1), idx, begin, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(50, 32)
    for b in range(50):
        assert bytes(got[b]) == hashlib.sha256(raw[20 * b:20 * b + 20].tobytes()).digest(), b
    # on a stream of the caller's as well
    table2, idx2 = dedupe_digests_device(hasher, _dev(raw.reshape(-1)), stream=_side())
    assert torch.equal(table2, table) and torch.equal(idx2, idx)
    engine.device_status()


@gpu
def test_tally_per_sequence(engine):
    """8 sequences x 16 senders, the sequence index as the scope, two senders dissenting:
    the tally equals a Python dict per sequence, i.e. agreements :=
    s.prepares[string(s.digest)] (sequence.go:271-277) restated."""
    from mirbft_amd import GPUHasher, tally_digests_device
    rng = np.random.default_rng(0x7A11)
    honest = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    rows = np.repeat(honest, 16, axis=0)                                   # slot 16 s + sender
    rows[16 * 2 + 5] = rng.integers(0, 256, 32, dtype=np.uint8)            # sender 5 dissents in sequence 2
    rows[16 * 6 + 0] = honest[1]                                           # sender 0 sends another sequence's digest in 6
    scope = np.repeat(np.arange(8, dtype=np.uint32), 16)
    prepares = [dict() for _ in range(8)]
    for i in range(128):
        key = bytes(rows[i])
        prepares[int(scope[i])][key] = prepares[int(scope[i])].get(key, 0) + 1
    hasher = GPUHasher(engine=engine)
    groups, max_count, max_group, first, group, members, gf, gc = tally_digests_device(
        hasher, _dev(rows.reshape(-1)), scope=_dev(scope))
    assert groups == sum(len(p) for p in prepares) == 10 and max_count == 16 and max_group == 0
    members, first, group = (t.cpu().numpy().view(np.uint32) for t in (members, first, group))
    for i in range(128):
        assert members[i] == prepares[int(scope[i])][bytes(rows[i])], i
    assert gf.numel() == gc.numel() == 10
    for leader, count in zip(gf.cpu().tolist(), gc.cpu().tolist()):
        assert prepares[int(scope[leader])][bytes(rows[leader])] == count
    want = M.oracle(rows.reshape(-1), scope, 64)
    assert np.array_equal(first, want[0]) and np.array_equal(group, want[1])
    # without the scope the two sequences that hold honest[1] fall into one group
    assert tally_digests_device(hasher, _dev(rows.reshape(-1)))[0] == 9
    assert tally_digests_device(hasher, _dev(rows.reshape(-1)), scope=_dev(scope), group_cap=0)[6].numel() == 0
    engine.device_status()


@gpu
def test_stats_and_other_counters(engine, monkeypatch):
    """calls, digests and launches (six a call) advance; last_kernel_ms is set only under
    MSHA_PARTS_TIMING=1; the other entries' counters do not move."""
    c = M.Case("stats", (np.arange(1000) % 33).astype(np.uint32))
    others = (engine.stats(), engine.parts_stats(), engine.concat_stats(), engine.verify_stats())
    q0 = engine.group_stats()
    Call(engine, c).check()
    q1 = engine.group_stats()
    assert (q1["calls"] - q0["calls"], q1["digests"] - q0["digests"], q1["launches"] - q0["launches"]) == (1, 1000, LAUNCHES)
    assert q1["last_kernel_ms"] == 0.0 and q1["table_slots"] == 2048
    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    Call(engine, c).check()
    monkeypatch.delenv("MSHA_PARTS_TIMING")
    q2 = engine.group_stats()
    assert q2["last_kernel_ms"] > 0 and q2["launches"] - q0["launches"] == 2 * LAUNCHES
    Call(engine, c).check()
    assert engine.group_stats()["last_kernel_ms"] == 0.0
    assert (engine.stats(), engine.parts_stats(), engine.concat_stats(), engine.verify_stats()) == others
    engine.device_status()
