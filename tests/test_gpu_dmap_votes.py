"""The vote maps on the GPU (mirbft_amd/csrc/dmap_vote.hip): device digest maps that count
each voter once a key. Every sequence of tests/dmap_vote_matrix.py runs step by step on a
vote map: each output (sentinel-filled before the call, a guard word on each side of every
array) and the eleven result words are compared with the dict-of-sets oracle, written from
the header; and after every step so is the map itself, through read, read_voters, size and
a find_votes of every (key, voter) seen so far. The helpers are those of
tests/test_gpu_dmap.py."""
import hashlib

import numpy as np
import pytest

import dmap_matrix as M
import dmap_vote_matrix as V
import test_gpu_dmap as G
from mirbft_amd import _lib as L

gpu = pytest.mark.gpu

LAUNCHES = 10                   # group's init, insert, resolve; find, pair, count, totals, scan, commit, fill (include/mirsha.h)
SENT32 = G.SENT32
SEQ = {s.name: s for s in V.all_sequences()}
_dev, _guarded, _inside, _side = G._dev, G._guarded, G._inside, G._side


class Vote:
    """One vote_device call on uploaded copies of a step's arrays. Every output is the
    inside of a buffer with a guard word on each side."""

    def __init__(self, dmap, step):
        import torch
        self.dmap, self.step = dmap, step
        self.digests = _dev(step.digests())
        self.scope = None if step.scope is None else _dev(step.scope)
        self.voter = _dev(step.voter)
        n, cap = step.n, step.crossed_cap
        self.ids = _guarded(n)
        self.counted, self.before, self.after = ((_guarded(n) if step.counts else None) for _ in range(3))
        self.crossed = _guarded(cap)
        self.result = torch.full((11,), -1, dtype=torch.int64, device="cuda:0")

    def prefill(self):
        for t in (self.ids, self.counted, self.before, self.after, self.crossed):
            if t is not None:
                t[1:-1] = SENT32
        self.result.fill_(-1)

    def run(self, stream=None):
        import torch
        st = _side() if stream is None else stream
        if stream is None:
            torch.cuda.synchronize()
        n, cap = self.step.n, self.step.crossed_cap
        inner = lambda t: None if t is None else t[1:1 + n]                # noqa: E731
        self.dmap.vote_device(self.digests, self.voter, self.ids[1:1 + n], self.result, scope=self.scope,
                              threshold=self.step.threshold, counted=inner(self.counted), before=inner(self.before),
                              after=inner(self.after), crossed_slots=self.crossed[1:1 + cap] if cap else None, stream=st)
        if stream is None:
            st.synchronize()
        return self

    def read(self):
        opt = lambda name, t: None if t is None else _inside(name, t)      # noqa: E731
        return {"kind": V.VOTE, "ids": _inside("ids", self.ids), "counted": opt("counted", self.counted),
                "before": opt("before", self.before), "after": opt("after", self.after),
                "crossed": _inside("crossed_slot", self.crossed),
                "result": tuple(int(x) for x in self.result.cpu().tolist())}


def _find_votes(dmap, digests, scope, voter, counts=True, stream=None):
    """One find_votes_device call -> a step result without the state."""
    import torch
    n = digests.size // 32
    ids, voted, count = _guarded(n), _guarded(n), _guarded(n) if counts else None
    st = _side() if stream is None else stream
    torch.cuda.synchronize()
    dmap.find_votes_device(_dev(digests), _dev(voter), ids[1:1 + n], voted[1:1 + n],
                           scope=None if scope is None else _dev(scope),
                           count=None if count is None else count[1:1 + n], stream=st)
    st.synchronize()
    return {"kind": V.FIND_VOTES, "ids": _inside("ids", ids), "voted": _inside("voted", voted),
            "count": None if count is None else _inside("count", count)}


def _state(dmap):
    """What the map holds, through size, read and read_voters -- the whole range, and the
    masks in two pieces."""
    entries = dmap.size()
    scope, digests, count = dmap.read(0, entries)
    masks = dmap.read_voters(0, entries)
    assert masks.shape == (entries, V.words(dmap.max_voters))
    if entries > 1:
        k = entries // 2
        assert np.array_equal(np.concatenate([dmap.read_voters(0, k), dmap.read_voters(k)]), masks)
    return scope, digests, count, masks


class Runner:
    """A sequence step by step on a vote map of the engine's, beside the dict-of-sets oracle."""

    def __init__(self, engine, seq):
        from mirbft_amd import GPUHasher
        self.seq = seq
        self.dmap = GPUHasher(engine=engine).new_device_vote_map(seq.max_keys, seq.max_voters)
        self.oracle = V.VoteMap(seq.max_keys, seq.max_voters)
        self.seen_digests, self.seen_scope, self.seen_voter = [], [], []
        self.got = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.dmap.close()

    def _check_map(self, want_state, where):
        """read, read_voters and size against the oracle, the top word's unused bits, and a
        find_votes of every (key, voter) seen so far."""
        got = _state(self.dmap)
        for name, w, g in zip(("scope", "digests", "count", "masks"), want_state, got):
            assert w.shape == g.shape and np.array_equal(w, g), "%s: the map's %s differs" % (where, name)
        assert np.array_equal(V.popcount(got[3]), got[2]), "%s: count is not popcount(mask)" % where
        spare = 32 * V.words(self.seq.max_voters) - self.seq.max_voters
        if spare and got[3].size:
            assert not (got[3][:, -1] >> np.uint32(32 - spare)).any(), "%s: a bit past max_voters is set" % where
        if self.seen_digests:
            digests, scope, voter = (np.concatenate(x) for x in (self.seen_digests, self.seen_scope, self.seen_voter))
            want = self.oracle.find_votes(digests, scope, voter)
            have = _find_votes(self.dmap, digests, scope, voter)
            assert all(np.array_equal(want[k], have[k]) for k in ("ids", "count", "voted")), \
                "%s: a find_votes of every (key, voter) seen so far differs" % where
            again = _state(self.dmap)
            assert all(np.array_equal(x, y) for x, y in zip(got, again)), "%s: the find_votes changed the map" % where

    def step(self, st, k=0):
        where = "%s step %d" % (self.seq.name, k)
        if st.kind == V.VOTE:
            got = Vote(self.dmap, st).run().read()
        elif st.kind == V.FIND_VOTES:
            got = _find_votes(self.dmap, st.digests(), st.scope, st.voter, counts=st.counts)
        else:
            import torch
            torch.cuda.synchronize()
            self.dmap.clear_device(stream=_side())
            _side().synchronize()
            got = {"kind": V.CLEAR}
        want = V.apply(self.oracle, st)
        if st.kind != V.CLEAR:
            self.seen_digests.append(st.digests())
            self.seen_scope.append(np.zeros(st.n, np.uint32) if st.scope is None else np.asarray(st.scope, np.uint32))
            self.seen_voter.append(np.asarray(st.voter, np.uint32))
        got["state"] = _state(self.dmap)
        if "result" in want:
            print("%s: result %s, expected %s" % (where, got["result"], want["result"]))
        assert V.problems(want, got) == [], where
        self._check_map(want["state"], where)
        self.got.append(got)
        return got

    def run(self):
        for k, st in enumerate(self.seq.steps):
            self.step(st, k)
        return self.got


def _run(engine, name):
    with Runner(engine, SEQ[name]) as r:
        return r.run()


@gpu
@pytest.mark.parametrize("n", V.sizes())
def test_one_call_on_an_empty_map(engine, n):
    """Every size with every pattern: all (key, voter) pairs distinct, one key and one
    voter (counted at slot 0 only), random draws from n / 4 keys x 4 voters."""
    for pattern in ("distinct", "equal", "random"):
        got = _run(engine, "one_%d_%s" % (n, pattern))
        if pattern == "equal":
            assert got[0]["result"] == (n, 1, 1, 0, 0, 0, 1, 0, 1, n - 1, 0)
            assert got[0]["counted"].tolist() == [1] + [0] * (n - 1)
        if pattern == "distinct":
            assert got[0]["result"][8:] == (n, 0, 0) and (got[0]["counted"] == 1).all()
    engine.device_status()


@gpu
def test_second_scan_chunk_and_exact_fit(engine):
    """n = max_keys = 65,537 distinct keys with one voter: 257 tiles, so the scan takes a
    second chunk, and the call fits exactly."""
    got = _run(engine, "big_exact_fit")
    assert got[0]["result"] == (V.BIG, V.BIG, V.BIG, 0, V.BIG, 4, 1, 0, V.BIG, 0, 0)
    assert got[0]["crossed"].tolist() == [0, 1, 2, 3]


@gpu
@pytest.mark.parametrize("max_voters", V.MASK_EDGES)
def test_mask_word_edges(engine, max_voters):
    """Voters 0, 31, 32, 63, 64 and max_voters - 1 on one key and on several, then all of them
    again: two voters of a key in one word and in different words, and no bit at or past
    max_voters."""
    got = _run(engine, "mask_edges_%d" % max_voters)
    assert got[0]["state"][3].shape == (1, V.words(max_voters))


@gpu
@pytest.mark.parametrize("name", [s.name for s in V.duplicate_sequences()])
def test_the_smallest_slot_of_equal_votes_is_counted(engine, name):
    got = _run(engine, name)
    a, b = V.DUPLICATES[name[4:].replace("_reversed", "")]
    lo, hi = (599 - b, 599 - a) if name.endswith("_reversed") else (a, b)
    assert got[0]["counted"][lo] == 1 and got[0]["counted"][hi] == 0 and got[0]["result"][8:] == (599, 1, 0)


@gpu
@pytest.mark.parametrize("name", [s.name for s in V.across_sequences()])
def test_across_calls(engine, name):
    got = _run(engine, name)
    if name == "third_voter":
        assert [g["result"][4] for g in got] == [0, 0, 1] and got[2]["crossed"][0] == 0


@gpu
def test_a_plain_map_crosses_one_call_earlier(engine):
    """The slots of "third_voter" on a plain map with add_device: key A has three slots after
    the second call and crosses there; on the vote map it has two voters, and crosses with
    its third in the third call."""
    seq = V.third_voter_plain()
    with G.Runner(engine, seq) as r:
        plain = r.run()
    votes = _run(engine, "third_voter")
    assert [g["result"][4] for g in plain] == [0, 1, 0] and plain[1]["crossed"][0] == 0 and plain[1]["after"][0] == 4
    assert [g["result"][4] for g in votes] == [0, 0, 1] and votes[1]["after"][0] == 2 and votes[2]["after"][0] == 3


@gpu
@pytest.mark.parametrize("name", [s.name for s in V.bad_voter_sequences()])
def test_voters_out_of_range(engine, name):
    got = _run(engine, name)
    assert got[0]["result"] == (2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 2) and not got[0]["state"][3].any()
    assert got[1]["result"][8:] == (2, 0, 3)
    engine.device_status()                                                 # a caller's error, not the device's


@gpu
def test_full_is_all_or_nothing(engine):
    got = _run(engine, "full")
    assert got[1]["result"] == (5, 3, 2, 1, 0, 0, 0, 0, 3, 2, 0) and (got[1]["ids"] == V.NO_ID).all()
    assert got[1]["counted"].tolist() == [1, 1, 1, 0, 0]
    assert all(np.array_equal(a, b) for a, b in zip(got[0]["state"], got[1]["state"]))      # byte-identical
    assert got[3]["ids"].tolist() == [3, 1] and got[4]["result"][3] == 1 and got[5]["result"][3] == 0


@gpu
@pytest.mark.parametrize("name", [s.name for s in V.probe_sequences()])
def test_probe_chains_and_wrap_around(engine, monkeypatch, name):
    """Every pair's home in the call's pair table forced to 0 and to capacity - 1, every
    key's home in the map's table to 0 and to 63; again under another seed, and as the hash
    places them: byte for byte the same."""
    seq = SEQ[name]
    var, home = ("MSHA_DMAP_PAIR_FORCE_HOME", seq.pair_home) if seq.pair_home is not None else ("MSHA_DMAP_FORCE_HOME", seq.home)
    monkeypatch.setenv(var, str(home))
    first = _run(engine, name)
    monkeypatch.setenv("MSHA_DMAP_SEED", "0xFEDCBA9876543210")
    monkeypatch.setenv("MSHA_GROUP_SEED", "0x0123456789ABCDEF")
    second = _run(engine, name)
    monkeypatch.delenv(var)
    monkeypatch.setenv("MSHA_DMAP_SEED", "1")
    third = _run(engine, name)
    for other in (second, third):
        for a, b in zip(first, other):
            assert V.problems(a, b) == []
    engine.device_status()


@gpu
@pytest.mark.parametrize("name", [s.name for s in V.other_sequences()])
def test_optional_arrays_clear_and_find_votes(engine, name):
    _run(engine, name)
    engine.device_status()


@gpu
def test_the_two_kinds_refuse_each_other(engine):
    """msha_dmap_add_device on a vote map and the vote entries on a plain map:
    MSHA_ERR_INVALID_ARG with their texts, nothing launched; find, size, read and clear work
    on both."""
    import ctypes
    import torch
    from mirbft_amd import GPUHasher
    lib, ctx = engine._lib, engine._ctx
    bad = L.MSHA_ERR_INVALID_ARG
    st = V.vote(np.arange(70) % 7, np.arange(70) % 3, threshold=2)
    hasher = GPUHasher(engine=engine)
    with Runner(engine, V.VSequence("kinds", 16, [st])) as r, hasher.new_device_digest_map(16) as plain:
        v = Vote(r.dmap, st)
        dig, voter, res = v.digests.data_ptr(), v.voter.data_ptr(), v.result.data_ptr()
        ids, counted, before, after, crossed = (t.data_ptr() + 4 for t in (v.ids, v.counted, v.before, v.after, v.crossed))
        torch.cuda.synchronize()
        s0, p0 = (r.dmap.stats(), r.dmap.vote_stats()), (plain.stats(), plain.vote_stats())
        assert lib.msha_dmap_add_device(r.dmap._h, dig, 70, None, 2, ids, before, after, crossed, 8, res, None) == bad
        assert b"msha_dmap_add_device: this is a vote map (msha_dmap_create_voters)" in lib.msha_last_error(ctx)
        assert lib.msha_dmap_vote_device(plain._h, dig, 70, None, voter, 2, ids, counted, before, after, crossed, 8, res,
                                         None) == bad
        assert b"msha_dmap_vote_device: this map keeps no voters: create it with msha_dmap_create_voters" in lib.msha_last_error(ctx)
        assert lib.msha_dmap_find_votes_device(plain._h, dig, 70, None, voter, ids, before, counted, None) == bad
        assert b"msha_dmap_find_votes_device: this map keeps no voters" in lib.msha_last_error(ctx)
        out = (ctypes.c_uint32 * 4)()
        assert lib.msha_dmap_read_voters(plain._h, 0, 0, out) == bad
        assert b"msha_dmap_read_voters: this map keeps no voters" in lib.msha_last_error(ctx)
        assert (r.dmap.stats(), r.dmap.vote_stats()) == s0 and (plain.stats(), plain.vote_stats()) == p0
        assert plain.vote_stats()["max_voters"] == 0 and r.dmap.vote_stats()["max_voters"] == 4
        torch.cuda.synchronize()
        assert v.read()["result"] == (-1,) * 11 and r.dmap.size() == 0 and plain.size() == 0
        # the entries both kinds share
        r.step(st)
        got = G._find(r.dmap, st.digests(), None)
        assert np.array_equal(got["ids"], np.arange(70) % 7) and (got["count"] == 3).all()
        assert r.dmap.read()[2].tolist() == [3] * 7 and r.dmap.stats()["finds"] == 1
    engine.device_status()


@gpu
def test_host_refusals(engine):
    """Each refusal is MSHA_ERR_INVALID_ARG with its text and launches nothing. n == 0 is OK
    before any other check, launches nothing and leaves d_result as it was."""
    import ctypes
    import torch
    from mirbft_amd import MshaError
    lib, ctx = engine._lib, engine._ctx
    bad = L.MSHA_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for keys, voters, text in ((0, 4, b"a device digest map holds 1 .. 2^30 keys"), ((1 << 30) + 1, 4, b"1 .. 2^30 keys"),
                               (16, 0, b"a vote map takes 1 .. 1024 voters"), (16, 1025, b"1 .. 1024 voters")):
        assert lib.msha_dmap_create_voters(ctx, keys, voters, ctypes.byref(h)) == bad and not h.value
        assert b"msha_dmap_create_voters: " in lib.msha_last_error(ctx) and text in lib.msha_last_error(ctx)
    st = V.vote(np.arange(70) % 7, np.arange(70) % 5, threshold=2)
    with Runner(engine, V.VSequence("refusals", 16, [st], max_voters=5)) as r:
        a = Vote(r.dmap, st)
        m = r.dmap._h
        dig, voter, res = a.digests.data_ptr(), a.voter.data_ptr(), a.result.data_ptr()
        ids, counted, before, after, crossed = (t.data_ptr() + 4 for t in (a.ids, a.counted, a.before, a.after, a.crossed))
        s0 = (r.dmap.stats(), r.dmap.vote_stats())
        vote, find = lib.msha_dmap_vote_device, lib.msha_dmap_find_votes_device
        torch.cuda.synchronize()
        for args in ((None, 70, None, voter, 2, ids, counted, before, after, crossed, 8, res),
                     (dig, 70, None, None, 2, ids, counted, before, after, crossed, 8, res),
                     (dig, 70, None, voter, 2, None, counted, before, after, crossed, 8, res),
                     (dig, 70, None, voter, 2, ids, counted, before, after, crossed, 8, None)):
            assert vote(m, *args, None) == bad
            assert b"msha_dmap_vote_device: null pointer" in lib.msha_last_error(ctx)
        assert vote(m, dig + 8, 69, None, voter, 2, ids, counted, before, after, crossed, 8, res, None) == bad
        assert b"msha_dmap_vote_device: d_digests must be 16-byte aligned" in lib.msha_last_error(ctx)
        assert vote(m, dig, (1 << 30) + 1, None, voter, 2, ids, counted, before, after, crossed, 8, res, None) == bad
        assert b"msha_dmap_vote_device: n must be at most 2^30" in lib.msha_last_error(ctx)
        assert vote(m, dig, 70, None, voter, 2, ids, counted, before, after, None, 8, res, None) == bad
        assert b"d_crossed_slot is null with crossed_cap > 0" in lib.msha_last_error(ctx)
        for args in ((None, 70, None, voter, ids, before, counted), (dig, 70, None, None, ids, before, counted),
                     (dig, 70, None, voter, None, before, counted), (dig, 70, None, voter, ids, before, None)):
            assert find(m, *args, None) == bad
            assert b"msha_dmap_find_votes_device: null pointer" in lib.msha_last_error(ctx)
        assert find(m, dig + 8, 69, None, voter, ids, before, counted, None) == bad
        assert b"msha_dmap_find_votes_device: d_digests must be 16-byte aligned" in lib.msha_last_error(ctx)
        # n == 0 comes first
        assert vote(m, None, 0, None, None, 0, None, None, None, None, None, 0, None, None) == L.MSHA_OK
        assert vote(m, dig + 8, 0, None, voter, 2, ids, counted, before, after, None, 8, res, None) == L.MSHA_OK
        assert find(m, None, 0, None, None, None, None, None, None) == L.MSHA_OK
        assert (r.dmap.stats(), r.dmap.vote_stats()) == s0                 # nothing was launched or counted
        torch.cuda.synchronize()
        got = a.read()
        assert got["result"] == (-1,) * 11 and r.dmap.size() == 0
        assert all((got[k] == M.SENTINEL).all() for k in ("ids", "counted", "before", "after", "crossed"))
        # a range past entries
        a.run()
        assert r.dmap.size() == 7 and r.dmap.read_voters(7, 0).shape == (0, 1) and r.dmap.read_voters(3).shape == (4, 1)
        for first, k in ((0, 8), (7, 1), (8, 0)):
            with pytest.raises(MshaError, match="msha_dmap_read_voters: ids .* reach past the map's 7 entries") as ei:
                r.dmap.read_voters(first, k)
            assert ei.value.code == bad
    engine.device_status()


@gpu
def test_context_stream(engine):
    """stream NULL: the context's own stream."""
    import torch
    seq = SEQ["crossing"]
    with Runner(engine, seq) as r:
        a = Vote(r.dmap, seq.steps[0])
        n, cap = a.step.n, a.step.crossed_cap
        torch.cuda.synchronize()
        r.dmap.vote_device(a.digests, a.voter, a.ids[1:1 + n], a.result, threshold=a.step.threshold,
                           counted=a.counted[1:1 + n], before=a.before[1:1 + n], after=a.after[1:1 + n],
                           crossed_slots=a.crossed[1:1 + cap])
        ids, voted = _guarded(n), _guarded(n)
        r.dmap.find_votes_device(a.digests, a.voter, ids[1:1 + n], voted[1:1 + n])
        torch.cuda.synchronize()
        got = a.read()
        got["state"] = _state(r.dmap)
        assert V.problems(V.apply(r.oracle, seq.steps[0]), got) == []
        assert np.array_equal(_inside("ids", ids), got["ids"]) and (_inside("voted", voted) == 1).all()
        r.dmap.clear_device()
        assert r.dmap.size() == 0


@gpu
def test_capturable_into_a_graph(engine):
    """After a warm call of the same size a vote captures on a side stream (ten launches
    counted for the capture; nothing runs during it). The warm call counted every voter, so
    each replay counts nothing new: repeats == n - bad_voters, and the map stays as it
    was. A find_votes captures as one launch."""
    import torch
    rng = np.random.default_rng(0xD3A7)
    n = 1500
    val = rng.integers(0, 400, n).astype(np.uint32)
    voter = rng.integers(0, 9, n).astype(np.uint32)                        # voter 8 is out of range
    st = V.vote(val, voter, threshold=3, crossed_cap=16)
    with Runner(engine, V.VSequence("graph", 512, [st], max_voters=8)) as r:
        warm = r.step(st)
        bad = int((voter >= 8).sum())
        assert warm["result"][10] == bad > 0 and warm["result"][8] > 0
        a = Vote(r.dmap, st)
        s = torch.cuda.Stream()
        before = (r.dmap.vote_stats(), r.dmap.stats())
        g = G._capture(s, lambda: a.run(stream=s))
        after = (r.dmap.vote_stats(), r.dmap.stats())
        assert after[0]["launches"] == before[0]["launches"] + LAUNCHES and after[0]["votes"] == before[0]["votes"] + 1
        assert after[1] == before[1]
        assert (a.result == -1).all() and (a.ids[1:-1] == SENT32).all()    # nothing ran
        r._check_map(r.oracle.state(), "after the capture")
        for k in range(2):
            a.prefill()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = a.read()
            want = V.apply(r.oracle, st)
            got["state"] = _state(r.dmap)
            print("replay %d: result %s, expected %s" % (k, got["result"], want["result"]))
            assert V.problems(want, got) == []
            assert got["result"][8:] == (0, n - bad, bad) and not got["counted"].any()
        r._check_map(r.oracle.state(), "after two replays")
        # a find_votes: one launch, one kernel node
        ids, voted = _guarded(n), _guarded(n)
        f0 = r.dmap.vote_stats()
        gf = G._capture(s, lambda: r.dmap.find_votes_device(a.digests, a.voter, ids[1:1 + n], voted[1:1 + n], stream=s))
        f1 = r.dmap.vote_stats()
        assert (f1["launches"] - f0["launches"], f1["vote_finds"] - f0["vote_finds"]) == (1, 1)
        assert (_inside("ids", ids) == M.SENTINEL).all()
        gf.replay()
        torch.cuda.synchronize()
        want = r.oracle.find_votes(st.digests(), None, voter)
        assert np.array_equal(_inside("ids", ids), want["ids"]) and np.array_equal(_inside("voted", voted), want["voted"])
        assert np.array_equal(want["voted"], (voter < 8).astype(np.uint32))
    engine.device_status()


@gpu
def test_captured_vote_is_a_linear_chain_of_kernel_nodes(engine):
    """The graph the runtime captures from a vote: kLaunches nodes, all kernels, one edge
    fewer, and the edges make one path through all of them. A find_votes: one kernel node."""
    import torch
    KERNEL = 0                                                             # hipGraphNodeTypeKernel
    assert V.launches() == LAUNCHES
    st = V.vote(np.arange(600) % 50, np.arange(600) % 7, threshold=3)
    with Runner(engine, V.VSequence("chain", 64, [st], max_voters=7)) as r:
        r.step(st)                                                         # the warm call
        a = Vote(r.dmap, st)
        s = torch.cuda.Stream()
        types, edges = G._captured_graph(s, lambda: a.run(stream=s))
        print("vote: node types %s, edges %s" % (types, edges))
        assert types == [KERNEL] * LAUNCHES and len(edges) == LAUNCHES - 1
        nxt = dict(edges)
        assert len(nxt) == LAUNCHES - 1 and len(set(nxt.values())) == LAUNCHES - 1     # one in, one out
        (at,) = set(range(LAUNCHES)) - set(nxt.values())                              # the one root
        walk = [at]
        while walk[-1] in nxt:
            walk.append(nxt[walk[-1]])
        assert sorted(walk) == list(range(LAUNCHES))
        n = st.n
        ids, voted = _guarded(n), _guarded(n)
        types, edges = G._captured_graph(
            s, lambda: r.dmap.find_votes_device(a.digests, a.voter, ids[1:1 + n], voted[1:1 + n], stream=s))
        assert types == [KERNEL] and edges == []
        assert (a.result == -1).all() and (_inside("voted", voted) == M.SENTINEL).all()      # nothing ran
        r._check_map(r.oracle.state(), "after the captures")


@gpu
def test_capture_without_a_workspace_fails_cleanly():
    """A vote map on a fresh context has no workspace, and may allocate none while the stream
    is being captured: MSHA_ERR_INVALID_ARG and the documented message, the map unchanged;
    the same call outside the capture then works, and a larger one is refused in a capture
    again."""
    import torch
    from mirbft_amd import Engine, MshaError
    with Engine(1) as eng:
        small = V.vote(np.arange(300) % 11, np.arange(300) % 3, threshold=2)
        big = V.vote(np.arange(5000) % 13 + 100, np.arange(5000) % 4, threshold=2)
        with Runner(eng, V.VSequence("fresh", 64, [small, big])) as r:
            for k, st in enumerate((small, big)):
                a = Vote(r.dmap, st)
                s = torch.cuda.Stream()
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.stream(s):
                    g.capture_begin()
                    try:
                        with pytest.raises(MshaError) as ei:
                            a.run(stream=s)
                    finally:
                        g.capture_end()
                torch.cuda.synchronize()
                assert ei.value.code == L.MSHA_ERR_INVALID_ARG and G.CAPTURE_MESSAGE in str(ei.value)
                assert "msha_dmap_vote_device" in str(ei.value)
                assert r.dmap.vote_stats()["votes"] == k and (a.result == -1).all()
                r._check_map(r.oracle.state(), "after the refused capture")
                r.step(st, k)
        eng.device_status()


@gpu
def test_stats_and_isolation(engine, monkeypatch):
    """Vote calls move only the vote stats: ten launches a vote, one a find_votes;
    last_kernel_ms only under MSHA_PARTS_TIMING=1. A clear counts in msha_dmap_stats, as on
    a plain map. Every other entry's counters and the device error word are untouched."""
    import torch
    others = (engine.stats(), engine.parts_stats(), engine.concat_stats(), engine.verify_stats(), engine.group_stats())
    st = V.vote(np.arange(1000) % 33, np.arange(1000) % 40, threshold=2)
    with Runner(engine, V.VSequence("stats", 40, [st], max_voters=40)) as r:
        plain0 = {"adds": 0, "finds": 0, "clears": 0, "digests": 0, "launches": 0, "capacity": 128, "last_kernel_ms": 0.0}
        assert r.dmap.stats() == plain0
        assert r.dmap.vote_stats() == {"votes": 0, "vote_finds": 0, "slots": 0, "launches": 0, "max_voters": 40,
                                       "mask_words": 2, "last_kernel_ms": 0.0}
        Vote(r.dmap, st).run()
        s1 = r.dmap.vote_stats()
        assert (s1["votes"], s1["slots"], s1["launches"], s1["last_kernel_ms"]) == (1, 1000, LAUNCHES, 0.0)
        _find_votes(r.dmap, st.digests(), None, st.voter)
        s2 = r.dmap.vote_stats()
        assert (s2["vote_finds"], s2["slots"], s2["launches"]) == (1, 2000, LAUNCHES + 1)
        assert r.dmap.stats() == plain0
        r.dmap.clear_device(stream=_side())
        assert r.dmap.stats() == dict(plain0, clears=1, launches=1) and r.dmap.vote_stats() == s2
        monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
        Vote(r.dmap, st).run()
        monkeypatch.delenv("MSHA_PARTS_TIMING")
        s4 = r.dmap.vote_stats()
        assert s4["last_kernel_ms"] > 0 and s4["launches"] == 2 * LAUNCHES + 1
        Vote(r.dmap, st).run()
        assert r.dmap.vote_stats()["last_kernel_ms"] == 0.0 and r.dmap.size() == 33
        torch.cuda.synchronize()
    assert (engine.stats(), engine.parts_stats(), engine.concat_stats(), engine.verify_stats(),
            engine.group_stats()) == others
    engine.device_status()


@gpu
def test_acks_from_four_nodes_end_to_end(engine):
    """The four-node ack scenario of tests/test_gpu_dmap.py, 80 requests, with what the plain
    map cannot take: every fifth ack is sent twice, and one node sends all its acks again in
    the last call. Hashed on the GPU in 3 calls of digest_batch_device and tallied with
    tally_votes_into_map_device(quorum=3): ids, counted, before, after, the crossing slots of
    each call and the final voter sets are hashlib's over a dict of sets."""
    import torch
    from mirbft_amd import GPUHasher, tally_votes_into_map_device
    rng = np.random.default_rng(0xACC5)
    reqs = [b"request %d from client %d" % (r, r % 5) + bytes(rng.integers(0, 256, r % 7, dtype=np.uint8)) for r in range(80)]
    votes = [(r, node) for r in range(80) for node in range(4) if (r + node) % 4 != 3 or r % 3 == 0]
    votes = [votes[i] for i in rng.permutation(len(votes))][:240]
    calls = [votes[80 * c:80 * c + 80] for c in range(3)]
    calls = [part + part[::5] for part in calls]                           # every fifth ack twice
    calls[2] = calls[2] + [v for v in votes if v[1] == 2]                  # node 2 sends everything again
    hasher = GPUHasher(engine=engine)
    dmap = hasher.new_device_vote_map(128, 4)
    tally, ident = {}, {}
    total_repeats = 0
    for call, part in enumerate(calls):
        msgs = [reqs[r] for r, _ in part]
        scope = np.array([r % 5 for r, _ in part], dtype=np.uint32)       # the client
        voter = np.array([node for _, node in part], dtype=np.uint32)
        lens = np.array([len(m) for m in msgs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)[:-1]]).astype(np.int64)  # starts 16-byte aligned
        arena = np.frombuffer(b"".join(m + b"\0" * (-len(m) % 16) for m in msgs) + b"\0" * 64, dtype=np.uint8)
        out = torch.zeros(32 * len(part), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        engine.digest_batch_device(_dev(arena), _dev(offs), _dev(lens), out)
        engine.device_status()
        entries, added, full, crossed, ids, counted, before, after, repeats, bad = tally_votes_into_map_device(
            dmap, out, _dev(voter), scope=_dev(scope), quorum=3, stream=_side() if call == 1 else None)
        was = {k: set(v) for k, v in tally.items()}
        keys = [(int(scope[i]), hashlib.sha256(reqs[r]).digest()) for i, (r, _) in enumerate(part)]
        want_counted = []
        for i, key in enumerate(keys):
            ident.setdefault(key, len(ident))
            fresh = int(voter[i]) not in tally.setdefault(key, set())
            want_counted.append(int(fresh))
            tally[key].add(int(voter[i]))
        want_cross, seen = [], set()
        for i, key in enumerate(keys):
            b4 = len(was.get(key, ()))
            assert (int(ids[i]), int(counted[i]), int(before[i]), int(after[i])) == \
                (ident[key], want_counted[i], b4, len(tally[key])), (call, i)
            if key not in seen and b4 < 3 <= len(tally[key]):
                want_cross.append(i)
            seen.add(key)
        assert not full and bad == 0 and entries == len(tally) and added == len(tally) - len(was)
        assert repeats == len(part) - sum(want_counted) > 0
        assert crossed.cpu().tolist() == want_cross[:64] and len(want_cross) <= 64, call
        total_repeats += repeats
    assert any(len(v) >= 3 for v in tally.values()) and dmap.size() == len(tally) and total_repeats >= 48
    scope, digests, count = dmap.read()
    masks = dmap.read_voters()
    have = {(int(s), bytes(d)): {v for v in range(4) if int(m[0]) >> v & 1} for s, d, m in zip(scope, digests, masks)}
    assert have == tally and count.tolist() == [len(have[(int(s), bytes(d))]) for s, d in zip(scope, digests)]
    assert dmap.stats()["adds"] == 0 and dmap.vote_stats()["votes"] == 3
    dmap.close()
    engine.device_status()
