"""msha_verify_digests_device on the GPU (mirbft_amd/csrc/verify.hip): digests compared
with expected ones, the mismatch mask, the counts and the list left in device memory.
Every case compares the whole mask (0xFF-filled before the call, so a word that is not
rewritten shows), the whole list (sentinel-filled: entries at and past `listed` keep
it), the five result words and a guard word on each side of mask and list with
tests/verify_matrix.py's numpy oracle, written from the header. Shapes are the smallest
at which each piece can go wrong: the wave (64), workgroup (256) and scan-chunk
(64 scan_words) edges."""
import hashlib

import numpy as np
import pytest

import verify_matrix as M
from mirbft_amd import _lib as L

gpu = pytest.mark.gpu

GUARD64 = 0x5A5A5A5A5A5A5A5A
GUARD32 = 0x5A5A5A5A
CAPTURE_MESSAGE = "make one call of this size outside the capture first"


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


class Call:
    """One verify_digests_device call on uploaded copies of a case's arrays. The mask and
    the list are the inside of buffers with a guard word on each side."""

    def __init__(self, engine, case, run=True):
        import torch
        self.engine, self.case = engine, case
        got, expected = case.arrays()
        self.host = [got, expected]
        self.got, self.expected = _dev(got), _dev(expected)
        self.idx = None if case.idx is None else _dev(case.idx)
        self.words = (case.n + 63) // 64
        self.mask_full = torch.full((self.words + 2,), -1, dtype=torch.int64, device="cuda:0")
        self.mask_full[0] = self.mask_full[-1] = GUARD64
        self.list_full = torch.from_numpy(np.full(case.list_cap + 2, M.LIST_SENTINEL, np.uint32).view(np.int32)).to("cuda:0")
        self.list_full[0] = self.list_full[-1] = GUARD32
        self.result = torch.full((5,), -1, dtype=torch.int64, device="cuda:0")
        if run:
            self.run()

    def prefill(self):
        self.mask_full[1:-1] = -1
        self.list_full[1:-1] = int(np.uint32(M.LIST_SENTINEL).view(np.int32))
        self.result.fill_(-1)

    def run(self, stream=None):
        """On `stream`, or (None) on a side stream of torch's that is waited for, with
        everything torch did before waited for first."""
        import torch
        st = _side() if stream is None else stream
        if stream is None:
            torch.cuda.synchronize()
        cap = self.case.list_cap
        self.engine.verify_digests_device(self.got, self.expected, self.mask_full[1:1 + self.words], self.result,
                                          expected_idx=self.idx, bad_list=self.list_full[1:1 + cap] if cap else None,
                                          stream=st)
        if stream is None:
            st.synchronize()

    def read(self):
        mask = self.mask_full.cpu().numpy().view(np.uint64)
        lst = self.list_full.cpu().numpy().view(np.uint32)
        assert mask[0] == GUARD64 == mask[-1], "a word beside the mask was written"
        assert lst[0] == GUARD32 == lst[-1], "an entry beside the list was written"
        return mask[1:-1].copy(), tuple(int(x) for x in self.result.cpu().tolist()), lst[1:-1].copy()

    def want(self):
        return M.oracle(self.host[0], self.host[1], self.case.idx, self.case.n_expected, self.case.list_cap)

    def check(self):
        want, got = self.want(), self.read()
        print("%s: result %s, expected %s" % (self.case.name, got[1], want[1]))
        assert M.problems(want, got) == [], self.case.name
        return got


@gpu
def test_scan_words_is_the_headers(engine):
    """scan_words is a constant, valid from context creation."""
    from mirbft_amd import Engine
    assert engine.verify_stats()["scan_words"] == M.scan_words()
    with Engine(1) as fresh:
        s = fresh.verify_stats()
        assert s["scan_words"] == M.scan_words() and s["calls"] == 0 and s["launches"] == 0


@gpu
@pytest.mark.parametrize("k", range(len(M.sizes(M.scan_words()))))
def test_sizes_and_patterns(engine, k):
    """Every size with every pattern it has room for: none, all, slot 0, slot n - 1, the
    last bit of a word with the first of the next, a slot on each side of a scan-chunk
    edge, a random 1 %."""
    W = engine.verify_stats()["scan_words"]
    n = M.sizes(W)[k]
    cases = M.size_cases(n, W)
    assert {c.name.split("_", 1)[1] for c in cases} >= {"none", "all", "first", "last", "random"}
    for c in cases:
        Call(engine, c).check()
    engine.device_status()


@gpu
@pytest.mark.parametrize("b", range(32))
def test_whole_digest_is_compared(engine, b):
    """n = 65, one slot whose expected digest differs in byte b alone."""
    c = M.byte_cases()[b]
    assert c.flips == [(M.EXPECTED, 40, b)]
    _, res, lst = Call(engine, c).check()
    assert res == (65, 1, 40, 1, 0) and lst[0] == 40


@gpu
@pytest.mark.parametrize("n", [1, 65, 4097])
def test_mask_words_all_rewritten_and_tail_bits_zero(engine, n):
    """The 0xFF-filled mask after a call in which nothing differs is all zeros, and after
    one in which everything differs the bits at and past n of the last word are 0."""
    mask, res, _ = Call(engine, M._differ("none", n, [])).check()
    assert not mask.any() and res == (n, 0, n, 0, 0)
    mask, res, _ = Call(engine, M._differ("all", n, range(n))).check()
    assert res[:3] == (n, n, 0)
    tail = n % 64
    assert int(mask[-1]) == ((1 << tail) - 1 if tail else (1 << 64) - 1) and (mask[:-1] == np.uint64(2**64 - 1)).all()


@gpu
@pytest.mark.parametrize("k", range(7))
def test_list_caps(engine, k):
    """list_cap 0 (d_bad_list NULL), 1, bad - 1, bad, bad + 1; list_cap in the middle of a
    scan chunk and exactly on a chunk edge. Entries at and past listed keep the sentinel."""
    c = M.list_cases(engine.verify_stats()["scan_words"])[k]
    _, res, lst = Call(engine, c).check()
    assert res[3] == min(res[1], c.list_cap) and (lst[res[3]:] == M.LIST_SENTINEL).all()
    assert np.all(np.diff(lst[:res[3]].astype(np.int64)) > 0)


@gpu
@pytest.mark.parametrize("k", range(3))
def test_expected_indices(engine, k):
    """Four rows shared by 257 slots; a permutation; entries equal to n_expected and
    0xFFFFFFFF: bad_index counts them, msha_device_status() stays MSHA_OK, every other
    slot is exact."""
    c = M.index_cases()[k]
    _, res, _ = Call(engine, c).check()
    engine.device_status()
    if c.name == "idx_out_of_range":
        assert res[4] == 3 and res[1] == 5
    else:
        assert res[4] == 0 and res[1] >= 3


@gpu
def test_context_stream(engine):
    """stream NULL: the context's own stream."""
    import torch
    c = Call(engine, M.index_cases()[2], run=False)
    torch.cuda.synchronize()
    engine.verify_digests_device(c.got, c.expected, c.mask_full[1:1 + c.words], c.result, expected_idx=c.idx,
                                 bad_list=c.list_full[1:1 + c.case.list_cap])
    engine.device_status()
    torch.cuda.synchronize()
    c.check()


@gpu
def test_host_refusals(engine):
    """Each refusal is MSHA_ERR_INVALID_ARG with its text and launches nothing. n == 0 is
    OK, launches nothing and leaves d_result as it was."""
    import torch
    c = Call(engine, M._differ("refusals", 70, [3]), run=False)
    idx = _dev(np.arange(70, dtype=np.uint32))
    lib, ctx = engine._lib, engine._ctx
    got, exp, mask, lst, res = (c.got.data_ptr(), c.expected.data_ptr(), c.mask_full.data_ptr() + 8,
                                c.list_full.data_ptr() + 4, c.result.data_ptr())
    bad = L.MSHA_ERR_INVALID_ARG
    before = engine.verify_stats()
    f = lib.msha_verify_digests_device
    torch.cuda.synchronize()
    for args in ((None, 70, exp, 70, None, mask, lst, 16, res), (got, 70, None, 70, None, mask, lst, 16, res),
                 (got, 70, exp, 70, None, None, lst, 16, res), (got, 70, exp, 70, None, mask, lst, 16, None)):
        assert f(ctx, *args, None) == bad
        assert b"msha_verify_digests_device: null pointer" in lib.msha_last_error(ctx)
    assert f(ctx, got + 8, 69, exp, 69, None, mask, lst, 16, res, None) == bad
    assert b"msha_verify_digests_device: d_got must be 16-byte aligned" in lib.msha_last_error(ctx)
    assert f(ctx, got, 69, exp + 8, 69, None, mask, lst, 16, res, None) == bad
    assert b"d_expected must be 16-byte aligned" in lib.msha_last_error(ctx)
    assert f(ctx, got, 0xFFFFFFFF, exp, 0xFFFFFFFF, None, mask, lst, 16, res, None) == bad
    assert b"n must be below 2^32 - 1" in lib.msha_last_error(ctx)
    assert f(ctx, got, 70, exp, 69, None, mask, lst, 16, res, None) == bad
    assert b"must equal n_expected" in lib.msha_last_error(ctx)
    assert f(ctx, got, 70, exp, 70, None, mask, None, 16, res, None) == bad
    assert b"d_bad_list is null with list_cap > 0" in lib.msha_last_error(ctx)
    assert f(ctx, got, 0, exp, 70, idx.data_ptr(), mask, lst, 16, res, None) == L.MSHA_OK
    assert f(ctx, got, 0, exp, 0, None, mask, None, 0, res, None) == L.MSHA_OK
    assert engine.verify_stats() == before          # nothing was launched or counted
    engine.device_status()
    torch.cuda.synchronize()
    mask_h, res_h, lst_h = c.read()
    assert res_h == (-1,) * 5 and (mask_h == np.uint64(2**64 - 1)).all() and (lst_h == M.LIST_SENTINEL).all()
    # list_cap 0 with a NULL list is a good call
    assert f(ctx, got, 70, exp, 70, None, mask, None, 0, res, None) == L.MSHA_OK
    torch.cuda.synchronize()
    assert tuple(c.result.cpu().tolist()) == (70, 1, 3, 0, 0)


@gpu
def test_capturable_into_a_graph(engine):
    """After a warm call the call captures into a HIP graph on a side stream (two
    launches counted for the capture; nothing runs during it), and each replay verifies
    what the arrays hold by then."""
    import torch
    W = engine.verify_stats()["scan_words"]
    c = Call(engine, M._differ("graph", 64 * W + 1, [5, 64 * W]))          # the warm call
    c.check()
    torch.cuda.synchronize()
    c.prefill()
    before = engine.verify_stats()["launches"]
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
    assert engine.verify_stats()["launches"] == before + 2
    assert (c.result == -1).all() and (c.mask_full[1:-1] == -1).all()
    for row in (77, 64 * W - 1):
        fresh = c.host[1].copy()
        fresh[32 * row + 9] ^= 0x01                                        # one expected row changes
        c.host[1] = fresh
        c.expected.copy_(_dev(fresh))
        c.prefill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _, res, lst = c.check()
        assert row in lst[:res[3]].tolist()
    assert res[1] == 4
    engine.device_status()


@gpu
def test_capture_on_a_fresh_context_fails_cleanly():
    """A fresh context may not allocate its error word while the stream is being
    captured: MSHA_ERR_INVALID_ARG and the documented message, and the same call outside
    the capture then works."""
    import torch
    from mirbft_amd import Engine, MshaError
    with Engine(1) as eng:
        c = Call(eng, M._differ("fresh", 300, [1, 299]), run=False)
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.capture_begin()
            try:
                with pytest.raises(MshaError) as ei:
                    c.run(stream=s)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG and CAPTURE_MESSAGE in str(ei.value)
        assert eng.verify_stats()["calls"] == 0 and (c.result == -1).all()
        c.run()
        c.check()


def _batches(rng, n_batches=300):
    counts = rng.integers(0, 41, n_batches)
    table = rng.integers(0, 256, (int(counts.sum()), 32), dtype=np.uint8)
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    idx = np.arange(table.shape[0], dtype=np.uint32)
    digests = [hashlib.sha256(table[int(begin[i]):int(begin[i + 1])].tobytes()).digest() for i in range(n_batches)]
    return table, idx, begin, np.frombuffer(b"".join(digests), dtype=np.uint8).copy()


@gpu
def test_verify_batches_end_to_end(engine):
    """300 batches of 0 to 40 acks hashed with digest_of_digests_device, the expected
    digests from hashlib: the uncorrupted run returns (0, n, []), and with three expected
    digests corrupted exactly those three come back in ascending order."""
    from mirbft_amd import GPUHasher, verify_batches_device
    rng = np.random.default_rng(0xE2E)
    table, idx, begin, expected = _batches(rng)
    hasher = GPUHasher(engine=engine)
    d = [_dev(table.reshape(-1)), _dev(idx), _dev(begin)]
    reads = engine.stats()["d2h_bytes"]
    assert verify_batches_device(hasher, *d, _dev(expected)) == (0, 300, [])
    corrupt = expected.copy()
    for i, byte in ((211, 0), (7, 31), (64, 13)):
        corrupt[32 * i + byte] ^= 0x10
    assert verify_batches_device(hasher, *d, _dev(corrupt)) == (3, 7, [7, 64, 211])
    assert verify_batches_device(hasher, *d, _dev(corrupt), list_cap=2) == (3, 7, [7, 64])
    assert verify_batches_device(hasher, *d, _dev(corrupt), list_cap=0) == (3, 7, [])
    import torch
    torch.cuda.synchronize()
    assert verify_batches_device(hasher, *d, _dev(corrupt), stream=_side()) == (3, 7, [7, 64, 211])
    assert engine.stats()["d2h_bytes"] == reads         # the engine brought no digest down
    engine.device_status()


@gpu
def test_stats_and_other_counters(engine, monkeypatch):
    """calls, digests and launches (two a call) advance; last_kernel_ms is set only under
    MSHA_PARTS_TIMING=1; msha_stats, msha_parts_stats and msha_concat_stats do not move."""
    c = M._differ("stats", 1000, [10, 999])
    others = (engine.stats(), engine.parts_stats(), engine.concat_stats())
    q0 = engine.verify_stats()
    Call(engine, c).check()
    q1 = engine.verify_stats()
    assert (q1["calls"] - q0["calls"], q1["digests"] - q0["digests"], q1["launches"] - q0["launches"]) == (1, 1000, 2)
    assert q1["last_kernel_ms"] == 0.0
    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    Call(engine, c).check()
    monkeypatch.delenv("MSHA_PARTS_TIMING")
    q2 = engine.verify_stats()
    assert q2["last_kernel_ms"] > 0 and q2["launches"] - q0["launches"] == 4 and q2["scan_words"] == q0["scan_words"]
    Call(engine, c).check()
    assert engine.verify_stats()["last_kernel_ms"] == 0.0
    assert (engine.stats(), engine.parts_stats(), engine.concat_stats()) == others
    engine.device_status()
