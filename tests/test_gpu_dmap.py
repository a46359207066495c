"""The device digest maps on the GPU (mirbft_amd/csrc/dmap.hip): tallies that persist
across calls in HBM. Every sequence of tests/dmap_matrix.py runs step by step on a map:
each output (sentinel-filled before the call, so an entry that is not written, or one
written past `listed`, shows), the eight result words and a guard word on each side of
every array are compared with the dict oracle, written from the header; and after every
step so is the map itself, through read, size and a find of all keys seen so far. Shapes
are the smallest at which each piece can go wrong: the wave (64) and tile (256) edges, a
second chunk of the scan, and a forced home position for the probe chain and its
wrap-around."""
import hashlib

import numpy as np
import pytest

import dmap_matrix as M
from mirbft_amd import _lib as L

gpu = pytest.mark.gpu

GUARD32 = 0x5A5A5A5A
CAPTURE_MESSAGE = "make one call of this size outside the capture first"
LAUNCHES = 7                    # group's init, insert, resolve; find, scan, commit, fill (include/mirsha.h)
SENT32 = int(np.uint32(M.SENTINEL).view(np.int32))
SEQ = {s.name: s for s in M.all_sequences()}


def _dev(a: np.ndarray):
    import torch
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
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


def _inside(name, t):
    a = t.cpu().numpy().view(np.uint32)
    assert a[0] == GUARD32 == a[-1], "an entry beside %s was written" % name
    return a[1:-1].copy()


class Add:
    """One add_device call on uploaded copies of a step's arrays. Every output is the
    inside of a buffer with a guard word on each side."""

    def __init__(self, dmap, step):
        import torch
        self.dmap, self.step = dmap, step
        self.digests = _dev(step.digests())
        self.scope = None if step.scope is None else _dev(step.scope)
        n, cap = step.n, step.crossed_cap
        self.ids = _guarded(n)
        self.before = _guarded(n) if step.counts else None
        self.after = _guarded(n) if step.counts else None
        self.crossed = _guarded(cap)
        self.result = torch.full((8,), -1, dtype=torch.int64, device="cuda:0")

    def prefill(self):
        for t in (self.ids, self.before, self.after, self.crossed):
            if t is not None:
                t[1:-1] = SENT32
        self.result.fill_(-1)

    def run(self, stream=None):
        """On `stream`, or (None) on a side stream of torch's that is waited for, with
        everything torch did before waited for first."""
        import torch
        st = _side() if stream is None else stream
        if stream is None:
            torch.cuda.synchronize()
        n, cap = self.step.n, self.step.crossed_cap
        self.dmap.add_device(self.digests, self.ids[1:1 + n], self.result, scope=self.scope,
                             threshold=self.step.threshold,
                             before=None if self.before is None else self.before[1:1 + n],
                             after=None if self.after is None else self.after[1:1 + n],
                             crossed_slots=self.crossed[1:1 + cap] if cap else None, stream=st)
        if stream is None:
            st.synchronize()
        return self

    def read(self):
        return {"kind": M.ADD, "ids": _inside("ids", self.ids),
                "before": None if self.before is None else _inside("before", self.before),
                "after": None if self.after is None else _inside("after", self.after),
                "crossed": _inside("crossed_slot", self.crossed),
                "result": tuple(int(x) for x in self.result.cpu().tolist())}


def _find(dmap, digests, scope, counts=True, stream=None):
    """One find_device call -> a step result without the state."""
    import torch
    n = digests.size // 32
    ids, count = _guarded(n), _guarded(n) if counts else None
    st = _side() if stream is None else stream
    torch.cuda.synchronize()
    dmap.find_device(_dev(digests), ids[1:1 + n], scope=None if scope is None else _dev(scope),
                     count=None if count is None else count[1:1 + n], stream=st)
    st.synchronize()
    return {"kind": M.FIND, "ids": _inside("ids", ids), "count": None if count is None else _inside("count", count)}


def _state(dmap):
    """What the map holds, through size and read -- the whole range, and in two pieces."""
    entries = dmap.size()
    scope, digests, count = dmap.read(0, entries)
    if entries > 1:
        k = entries // 2
        a, b = dmap.read(0, k), dmap.read(k, entries - k)
        assert all(np.array_equal(np.concatenate([x, y]), z) for x, y, z in zip(a, b, (scope, digests, count)))
    return scope, digests, count


class Runner:
    """A sequence step by step on a map of the engine's, beside the dict oracle."""

    def __init__(self, engine, seq):
        from mirbft_amd import GPUHasher
        self.seq = seq
        self.dmap = GPUHasher(engine=engine).new_device_digest_map(seq.max_keys)
        self.oracle = M.DictMap(seq.max_keys)
        self.seen_digests, self.seen_scope = [], []
        self.got = []

    def close(self):
        self.dmap.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check_map(self, want_state, where):
        """read and size against the oracle, and a find of every key seen so far."""
        got = _state(self.dmap)
        for name, w, g in zip(("scope", "digests", "count"), want_state, got):
            assert w.shape == g.shape and np.array_equal(w, g), "%s: read's %s differs" % (where, name)
        if self.seen_digests:
            digests = np.concatenate(self.seen_digests)
            scope = np.concatenate(self.seen_scope)
            want = self.oracle.find(digests, scope)
            have = _find(self.dmap, digests, scope)
            assert np.array_equal(want["ids"], have["ids"]) and np.array_equal(want["count"], have["count"]), \
                "%s: a find of all keys seen so far differs" % where
            again = _state(self.dmap)
            assert all(np.array_equal(x, y) for x, y in zip(got, again)), "%s: the find changed the map" % where

    def step(self, st, k=0):
        where = "%s step %d" % (self.seq.name, k)
        if st.kind == M.ADD:
            got = Add(self.dmap, st).run().read()
        elif st.kind == M.FIND:
            got = _find(self.dmap, st.digests(), st.scope, counts=st.counts)
        else:
            import torch
            torch.cuda.synchronize()
            self.dmap.clear_device(stream=_side())
            _side().synchronize()
            got = {"kind": M.CLEAR}
        want = M.apply(self.oracle, st)
        if st.kind != M.CLEAR:
            self.seen_digests.append(st.digests())
            self.seen_scope.append(np.zeros(st.n, np.uint32) if st.scope is None else np.asarray(st.scope, np.uint32))
        got["state"] = _state(self.dmap)
        if "result" in want:
            print("%s: result %s, expected %s" % (where, got["result"], want["result"]))
        assert M.problems(want, got) == [], where
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
@pytest.mark.parametrize("n", M.sizes())
def test_one_call_on_an_empty_map(engine, n):
    """Every size with every pattern: all distinct (an exact fit), all equal, random draws
    from n / 4 keys."""
    for pattern in ("distinct", "equal", "random"):
        got = _run(engine, "one_%d_%s" % (n, pattern))
        if pattern == "equal":
            assert got[0]["result"] == (n, 1, 1, 0, int(n >= 2), int(n >= 2), n, 0)
        if pattern == "distinct":
            assert got[0]["result"] == (n, n, n, 0, 0, 0, 1, 0) and got[0]["ids"].tolist() == list(range(n))
    engine.device_status()


@gpu
def test_second_scan_chunk_and_exact_fit(engine):
    """n = max_keys = 65,537 distinct keys: 257 tiles, so the scan takes a second chunk,
    and the call fits exactly."""
    got = _run(engine, "big_exact_fit")
    assert got[0]["result"] == (M.BIG, M.BIG, M.BIG, 0, M.BIG, 4, 1, 0) and got[0]["crossed"].tolist() == [0, 1, 2, 3]


@gpu
@pytest.mark.parametrize("name", [s.name for s in M.across_sequences()])
def test_across_calls(engine, name):
    """The same keys twice, disjoint keys, new and held keys interleaved inside a tile and
    across tile edges, a leader whose other members lie in another tile, and scopes."""
    _run(engine, name)


@gpu
@pytest.mark.parametrize("name", [s.name for s in M.stored_compare_sequences()])
def test_whole_stored_key_is_compared(engine, name):
    """A second call's key differs from stored key 3 in one byte, or in the scope, only: a
    compare with the stored keys that left it out would hand out id 3."""
    got = _run(engine, name)
    assert got[1]["ids"].tolist() == [65, 3, 10] and got[1]["result"][:3] == (3, 66, 1)


@gpu
@pytest.mark.parametrize("home", (0, 63))
def test_probe_chain_and_wrap_around(engine, monkeypatch, home):
    """max_keys 8, capacity 64, every key's home forced to 0 and to 63 (the chain wraps
    around): three adds, a find after each; and again under another seed, byte for byte."""
    seq = SEQ["chain_home_%d" % home]
    assert seq.home == home and engine is not None
    monkeypatch.setenv("MSHA_DMAP_FORCE_HOME", str(home))
    first = _run(engine, seq.name)
    monkeypatch.setenv("MSHA_DMAP_SEED", "0xFEDCBA9876543210")
    second = _run(engine, seq.name)
    monkeypatch.delenv("MSHA_DMAP_FORCE_HOME")
    monkeypatch.setenv("MSHA_DMAP_SEED", "1")
    third = _run(engine, seq.name)                                        # and as the hash places them
    for other in (second, third):
        for a, b in zip(first, other):
            assert M.problems(a, b) == []
    engine.device_status()


@gpu
def test_full_is_all_or_nothing(engine):
    got = _run(engine, "full")
    assert got[1]["result"] == (4, 3, 2, 1, 0, 0, 0, 0) and (got[1]["ids"] == M.NO_ID).all()
    assert all(np.array_equal(a, b) for a, b in zip(got[0]["state"], got[1]["state"]))      # byte-identical
    assert got[3]["ids"].tolist() == [3, 1] and got[4]["result"][3] == 1 and got[5]["result"][3] == 0


@gpu
@pytest.mark.parametrize("name", [s.name for s in M.crossing_sequences()])
def test_crossing(engine, name):
    got = _run(engine, name)
    if name == "crossing_two_tiles":
        assert got[0]["crossed"].tolist() == [10, 300, M.SENTINEL, M.SENTINEL]
    if name == "crossing_cap":
        assert got[0]["result"][4:6] == (5, 2) and got[0]["crossed"].tolist() == [0, 3]


@gpu
@pytest.mark.parametrize("name", [s.name for s in M.other_sequences()])
def test_optional_arrays_clear_and_find(engine, name):
    """d_before, d_after and d_count NULL; clear, then reuse (ids start at 0 again, old
    keys are absent); present and absent keys found."""
    _run(engine, name)
    engine.device_status()


@gpu
def test_context_stream(engine):
    """stream NULL: the context's own stream."""
    import torch
    seq = SEQ["crossing"]
    with Runner(engine, seq) as r:
        a = Add(r.dmap, seq.steps[0])
        n, cap = a.step.n, a.step.crossed_cap
        torch.cuda.synchronize()
        r.dmap.add_device(a.digests, a.ids[1:1 + n], a.result, threshold=a.step.threshold, before=a.before[1:1 + n],
                          after=a.after[1:1 + n], crossed_slots=a.crossed[1:1 + cap])
        ids = _guarded(n)
        r.dmap.find_device(a.digests, ids[1:1 + n])
        torch.cuda.synchronize()
        got = a.read()
        got["state"] = _state(r.dmap)
        assert M.problems(M.apply(r.oracle, seq.steps[0]), got) == []
        assert np.array_equal(_inside("ids", ids), got["ids"])
        r.dmap.clear_device()
        assert r.dmap.size() == 0


@gpu
def test_host_refusals(engine):
    """Each refusal is MSHA_ERR_INVALID_ARG with its text and launches nothing. n == 0 is
    OK, launches nothing and leaves d_result as it was."""
    import ctypes
    import torch
    from mirbft_amd import MshaError
    lib, ctx = engine._lib, engine._ctx
    bad = L.MSHA_ERR_INVALID_ARG
    h = ctypes.c_void_p()
    for keys in (0, (1 << 30) + 1):
        assert lib.msha_dmap_create(ctx, keys, ctypes.byref(h)) == bad and not h.value
        assert b"msha_dmap_create: a device digest map holds 1 .. 2^30 keys" in lib.msha_last_error(ctx)
    with Runner(engine, SEQ["find"]) as r:
        a = Add(r.dmap, M.add(np.arange(70) % 7, threshold=2))
        m = r.dmap._h
        dig, res = a.digests.data_ptr(), a.result.data_ptr()
        ids, before, after, crossed = (t.data_ptr() + 4 for t in (a.ids, a.before, a.after, a.crossed))
        s0 = r.dmap.stats()
        add, find = lib.msha_dmap_add_device, lib.msha_dmap_find_device
        torch.cuda.synchronize()
        for args in ((None, 70, None, 2, ids, before, after, crossed, 8, res),
                     (dig, 70, None, 2, None, before, after, crossed, 8, res),
                     (dig, 70, None, 2, ids, before, after, crossed, 8, None)):
            assert add(m, *args, None) == bad
            assert b"msha_dmap_add_device: null pointer" in lib.msha_last_error(ctx)
        assert add(m, dig + 8, 69, None, 2, ids, before, after, crossed, 8, res, None) == bad
        assert b"msha_dmap_add_device: d_digests must be 16-byte aligned" in lib.msha_last_error(ctx)
        assert add(m, dig, (1 << 30) + 1, None, 2, ids, before, after, crossed, 8, res, None) == bad
        assert b"msha_dmap_add_device: n must be at most 2^30" in lib.msha_last_error(ctx)
        assert add(m, dig, 70, None, 2, ids, before, after, None, 8, res, None) == bad
        assert b"d_crossed_slot is null with crossed_cap > 0" in lib.msha_last_error(ctx)
        for args in ((None, 70, None, ids, before), (dig, 70, None, None, before)):
            assert find(m, *args, None) == bad
            assert b"msha_dmap_find_device: null pointer" in lib.msha_last_error(ctx)
        assert find(m, dig + 8, 69, None, ids, before, None) == bad
        assert b"msha_dmap_find_device: d_digests must be 16-byte aligned" in lib.msha_last_error(ctx)
        assert find(m, dig, (1 << 30) + 1, None, ids, before, None) == bad
        assert b"msha_dmap_find_device: n must be at most 2^30" in lib.msha_last_error(ctx)
        assert add(m, dig, 0, None, 2, ids, before, after, crossed, 8, res, None) == L.MSHA_OK
        assert add(m, None, 0, None, 0, None, None, None, None, 0, None, None) == L.MSHA_OK
        assert find(m, None, 0, None, None, None, None) == L.MSHA_OK
        assert add(m, dig + 8, 0, None, 2, ids, before, after, crossed, 8, res, None) == L.MSHA_OK   # n == 0 comes first
        assert find(m, dig + 8, 0, None, ids, before, None) == L.MSHA_OK
        assert r.dmap.stats() == s0                     # nothing was launched or counted
        torch.cuda.synchronize()
        got = a.read()
        assert got["result"] == (-1,) * 8 and r.dmap.size() == 0
        assert all((got[k] == M.SENTINEL).all() for k in ("ids", "before", "after", "crossed"))
        # a range past entries
        a.run()
        assert r.dmap.size() == 7 and r.dmap.read(7, 0)[0].size == 0 and r.dmap.read(3)[2].tolist() == [10] * 4
        for first, k in ((0, 8), (7, 1), (8, 0)):
            with pytest.raises(MshaError, match="reach past the map's 7 entries") as ei:
                r.dmap.read(first, k)
            assert ei.value.code == bad
    engine.device_status()


def _capture(stream, fn):
    import torch
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g.capture_begin()
        try:
            fn()
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    return g


def _hip():
    """The HIP runtime this process already runs on (torch's), by the path it was loaded
    from. torch.cuda.CUDAGraph holds its graph privately and reports neither node types nor
    edges, so the chain test captures through the runtime's own calls; and it must be the
    runtime torch and libmirsha.so already share (mirbft_amd/_lib.py: one HIP runtime a
    process), which ctypes finds for certain only by the path of the loaded file."""
    import ctypes
    import torch  # noqa: F401
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime is loaded")


def _captured_graph(stream, fn):
    """fn()'s launches on `stream` captured by the runtime itself -> (the type of each
    node, the edges as pairs of node indices). Nothing runs."""
    import ctypes
    import torch
    hip = _hip()
    st = ctypes.c_void_p(stream.cuda_stream)
    graph = ctypes.c_void_p()
    torch.cuda.synchronize()
    assert hip.hipStreamBeginCapture(st, 2) == 0                          # hipStreamCaptureModeRelaxed
    try:
        fn()
    finally:
        assert hip.hipStreamEndCapture(st, ctypes.byref(graph)) == 0
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * max(n.value, 1))()
    assert hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
    types = []
    for k in range(n.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nodes[k]), ctypes.byref(t)) == 0
        types.append(t.value)
    e = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(e)) == 0
    src, dst = (ctypes.c_void_p * max(e.value, 1))(), (ctypes.c_void_p * max(e.value, 1))()
    if e.value:
        assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(e)) == 0
    index = {nodes[k]: k for k in range(n.value)}
    edges = [(index[src[k]], index[dst[k]]) for k in range(e.value)]
    assert hip.hipGraphDestroy(graph) == 0
    torch.cuda.synchronize()
    return types, edges


@gpu
def test_capturable_into_a_graph(engine):
    """After a warm call of the same size an add captures on a side stream (seven launches
    counted for the capture; nothing runs during it), and each replay adds again: counts
    against the oracle. A find captures as one launch."""
    import torch
    rng = np.random.default_rng(0xD3A7)
    val = rng.integers(0, 400, 1500).astype(np.uint32)
    st = M.add(val, threshold=8, crossed_cap=16)
    with Runner(engine, M.Sequence("graph", 512, [st])) as r:
        r.step(st)                                                         # the warm call
        a = Add(r.dmap, st)
        s = torch.cuda.Stream()
        before = r.dmap.stats()
        g = _capture(s, lambda: a.run(stream=s))
        after = r.dmap.stats()
        assert after["launches"] == before["launches"] + LAUNCHES and after["adds"] == before["adds"] + 1
        assert (a.result == -1).all() and (a.ids[1:-1] == SENT32).all()    # nothing ran
        r._check_map(r.oracle.state(), "after the capture")
        for k in range(2):
            a.prefill()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = a.read()
            want = M.apply(r.oracle, st)
            got["state"] = _state(r.dmap)
            print("replay %d: result %s, expected %s" % (k, got["result"], want["result"]))
            assert M.problems(want, got) == []
        assert int(got["after"].max()) == 3 * int(np.bincount(val).max())
        r._check_map(r.oracle.state(), "after two replays")
        # a find: one launch, one kernel node
        n = st.n
        ids, count = _guarded(n), _guarded(n)
        f0 = r.dmap.stats()
        gf = _capture(s, lambda: r.dmap.find_device(a.digests, ids[1:1 + n], count=count[1:1 + n], stream=s))
        f1 = r.dmap.stats()
        assert (f1["launches"] - f0["launches"], f1["finds"] - f0["finds"]) == (1, 1)
        assert (_inside("ids", ids) == M.SENTINEL).all()
        gf.replay()
        torch.cuda.synchronize()
        want = r.oracle.find(st.digests(), None)
        assert np.array_equal(_inside("ids", ids), want["ids"]) and np.array_equal(_inside("count", count), want["count"])
        r._check_map(r.oracle.state(), "after the captured find")
    engine.device_status()


@gpu
def test_captured_add_is_a_linear_chain_of_seven_kernel_nodes(engine):
    """The graph the runtime captures from an add: seven nodes, all kernels, six edges, and
    the edges make one path through all of them. A find: one kernel node, no edge."""
    import torch
    KERNEL = 0                                                             # hipGraphNodeTypeKernel
    st = M.add(np.arange(600) % 50, threshold=3)
    with Runner(engine, M.Sequence("chain", 64, [st])) as r:
        r.step(st)                                                         # the warm call
        a = Add(r.dmap, st)
        s = torch.cuda.Stream()
        types, edges = _captured_graph(s, lambda: a.run(stream=s))
        print("add: node types %s, edges %s" % (types, edges))
        assert types == [KERNEL] * LAUNCHES and len(edges) == LAUNCHES - 1
        nxt = dict(edges)
        assert len(nxt) == LAUNCHES - 1 and len(set(nxt.values())) == LAUNCHES - 1     # one in, one out
        (at,) = set(range(LAUNCHES)) - set(nxt.values())                              # the one root
        walk = [at]
        while walk[-1] in nxt:
            walk.append(nxt[walk[-1]])
        assert sorted(walk) == list(range(LAUNCHES))
        n = st.n
        ids = _guarded(n)
        types, edges = _captured_graph(s, lambda: r.dmap.find_device(a.digests, ids[1:1 + n], stream=s))
        assert types == [KERNEL] and edges == []
        assert (a.result == -1).all() and (_inside("ids", ids) == M.SENTINEL).all()    # nothing ran
        r._check_map(r.oracle.state(), "after the captures")


@gpu
def test_capture_without_a_workspace_fails_cleanly():
    """A map on a fresh context has no workspace, and may allocate none while the stream is
    being captured: MSHA_ERR_INVALID_ARG and the documented message, the map unchanged;
    the same call outside the capture then works, and a larger one is refused in a
    capture again (the workspace would have to grow)."""
    import torch
    from mirbft_amd import Engine, MshaError
    with Engine(1) as eng:
        small, big = M.add(np.arange(300) % 11, threshold=2), M.add(np.arange(5000) % 13 + 100, threshold=2)
        with Runner(eng, M.Sequence("fresh", 64, [small, big])) as r:
            for k, st in enumerate((small, big)):
                a = Add(r.dmap, st)
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
                assert ei.value.code == L.MSHA_ERR_INVALID_ARG and CAPTURE_MESSAGE in str(ei.value)
                assert "msha_dmap_add_device" in str(ei.value)
                assert r.dmap.stats()["adds"] == k and (a.result == -1).all()
                r._check_map(r.oracle.state(), "after the refused capture")
                r.step(st, k)
        eng.device_status()


@gpu
def test_stats_and_isolation(engine, monkeypatch):
    """Launches are seven an add, one a find, one a clear; last_kernel_ms is set only under
    MSHA_PARTS_TIMING=1; the group entry's counters, and every other entry's, do not move
    with map calls, and the device error word is untouched."""
    import torch
    others = (engine.stats(), engine.parts_stats(), engine.concat_stats(), engine.verify_stats(), engine.group_stats())
    st = M.add(np.arange(1000) % 33, threshold=2)
    with Runner(engine, M.Sequence("stats", 40, [st])) as r:
        s0 = r.dmap.stats()
        assert s0 == {"adds": 0, "finds": 0, "clears": 0, "digests": 0, "launches": 0, "capacity": 128,
                      "last_kernel_ms": 0.0}
        Add(r.dmap, st).run()
        s1 = r.dmap.stats()
        assert (s1["adds"], s1["digests"], s1["launches"], s1["last_kernel_ms"]) == (1, 1000, LAUNCHES, 0.0)
        _find(r.dmap, st.digests(), None)
        s2 = r.dmap.stats()
        assert (s2["finds"], s2["digests"], s2["launches"]) == (1, 2000, LAUNCHES + 1)
        r.dmap.clear_device(stream=_side())
        s3 = r.dmap.stats()
        assert (s3["clears"], s3["launches"]) == (1, LAUNCHES + 2)
        monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
        Add(r.dmap, st).run()
        monkeypatch.delenv("MSHA_PARTS_TIMING")
        s4 = r.dmap.stats()
        assert s4["last_kernel_ms"] > 0 and s4["launches"] == 2 * LAUNCHES + 2
        Add(r.dmap, st).run()
        assert r.dmap.stats()["last_kernel_ms"] == 0.0 and r.dmap.size() == 33
        torch.cuda.synchronize()
    assert (engine.stats(), engine.parts_stats(), engine.concat_stats(), engine.verify_stats(),
            engine.group_stats()) == others
    engine.device_status()


@gpu
def test_acks_from_four_nodes_end_to_end(engine):
    """240 small acks, 80 requests acknowledged by up to 4 nodes, hashed on the GPU in 3
    calls of digest_batch_device and tallied into one map with quorum 3: ids, counts and
    the crossing slots of every call are hashlib's over a dict."""
    import torch
    from mirbft_amd import GPUHasher, tally_into_map_device
    rng = np.random.default_rng(0xACC5)
    reqs = [b"request %d from client %d" % (r, r % 5) + bytes(rng.integers(0, 256, r % 7, dtype=np.uint8)) for r in range(80)]
    votes = [(r, node) for r in range(80) for node in range(4) if (r + node) % 4 != 3 or r % 3 == 0]
    votes = [votes[i] for i in rng.permutation(len(votes))][:240]
    hasher = GPUHasher(engine=engine)
    dmap = hasher.new_device_digest_map(128)
    tally, ident = {}, {}
    for call in range(3):
        part = votes[80 * call:80 * call + 80]
        msgs = [reqs[r] for r, _ in part]
        scope = np.array([r % 5 for r, _ in part], dtype=np.uint32)       # the client
        lens = np.array([len(m) for m in msgs], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)[:-1]]).astype(np.int64)  # starts 16-byte aligned
        arena = np.frombuffer(b"".join(m + b"\0" * (-len(m) % 16) for m in msgs) + b"\0" * 64, dtype=np.uint8)
        out = torch.zeros(32 * len(part), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        engine.digest_batch_device(_dev(arena), _dev(offs), _dev(lens), out)
        engine.device_status()
        entries, added, full, crossed, ids, before, after = tally_into_map_device(
            dmap, out, scope=_dev(scope), quorum=3, stream=_side() if call == 1 else None)
        want_cross, was = [], dict(tally)
        for i, (r, _) in enumerate(part):
            key = (int(scope[i]), hashlib.sha256(reqs[r]).digest())
            ident.setdefault(key, len(ident))
            tally[key] = tally.get(key, 0) + 1
        seen = set()
        for i, (r, _) in enumerate(part):
            key = (int(scope[i]), hashlib.sha256(reqs[r]).digest())
            assert int(ids[i]) == ident[key] and int(before[i]) == was.get(key, 0) and int(after[i]) == tally[key], (call, i)
            if key not in seen and was.get(key, 0) < 3 <= tally[key]:
                want_cross.append(i)
            seen.add(key)
        assert not full and entries == len(tally) and added == len(tally) - len(was)
        assert crossed.cpu().tolist() == want_cross[:64] and len(want_cross) <= 64, call
    assert any(v >= 3 for v in tally.values()) and dmap.size() == len(tally)
    scope, digests, count = dmap.read()
    assert {(int(s), bytes(d)): int(c) for s, d, c in zip(scope, digests, count)} == tally
    dmap.close()
    engine.device_status()
