"""msha_concat_lists_device on the GPU (mirbft_amd/csrc/parts_concat.hip): part lists
flattened into contiguous, 16-byte aligned messages. Every case compares all of d_dst
(0xA5-filled before the call, so a stray write shows), d_msg_off and d_msg_len with
tests/parts_concat_matrix.py's model, written from the header, then hashes the result
with digest_batch_device and compares with hashlib of the joined parts. Shapes are the
smallest at which each piece can go wrong: every step, window, threshold and scan edge."""
import hashlib

import numpy as np
import pytest

import parts_concat_matrix as M
import parts_matrix
from mirbft_amd import MshaError
from mirbft_amd import _lib as L

gpu = pytest.mark.gpu

CAPTURE_MESSAGE = "make one call of this size outside the capture first"
CONCAT_TEXT = "msha_concat_lists_device"
EMPTY = hashlib.sha256(b"").digest()


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


class Call:
    """One concat_lists_device call on uploaded copies. d_dst is the first dst_bytes
    bytes of a larger 0xA5-filled buffer, all of which is compared afterwards."""

    def __init__(self, engine, arena, off, ln, begin, select=None, dst_bytes=None, run=True):
        import torch
        self.engine = engine
        self.host = (arena, off, ln, begin, select)
        self.n = begin.size - 1 if select is None else select.size
        self.dst_bytes = M.concat_need(ln, begin, select) if dst_bytes is None else dst_bytes
        self.full = torch.full((self.dst_bytes + 2 * M.SLACK,), M.SENTINEL, dtype=torch.uint8, device="cuda:0")
        self.dev = [_dev(x) for x in (arena, off, ln, begin)]
        self.sel = None if select is None else _dev(select)
        self.msg_off = torch.full((self.n,), -1, dtype=torch.int64, device="cuda:0")
        self.msg_len = torch.full((self.n,), -1, dtype=torch.int64, device="cuda:0")
        if run:
            self.run()

    def run(self, stream=None):
        self.engine.concat_lists_device(*self.dev, self.full[:self.dst_bytes], self.msg_off, self.msg_len,
                                        select=self.sel, stream=stream)

    def model(self, arena=None):
        a, off, ln, begin, select = self.host
        return M.concat_model(a if arena is None else arena, off, ln, begin, select, self.dst_bytes)

    def check(self, model=None):
        """Everything the call wrote against the model, then the digests of the result."""
        model = model or self.model()
        want, mask, w_off, w_len, _ = model
        pad = np.full(2 * M.SLACK, M.SENTINEL, dtype=np.uint8)
        padded = (np.concatenate([want, pad]), np.concatenate([mask, np.zeros(pad.size, dtype=bool)]), w_off, w_len,
                  model[4])
        got_off = self.msg_off.cpu().numpy().view(np.uint64)
        got_len = self.msg_len.cpu().numpy().view(np.uint64)
        assert M.problems(padded, self.full.cpu().numpy(), got_off, got_len) == []
        self.check_digests(want, w_off, w_len)

    def check_digests(self, want, w_off, w_len):
        import torch
        out = torch.zeros((self.n, 32), dtype=torch.uint8, device="cuda:0")
        self.engine.digest_batch_device(self.full, self.msg_off, self.msg_len, out)
        self.engine.device_status()
        got = out.cpu().numpy()
        # hashlib of the joined parts: the model's bytes are the join (a refused message is the empty string)
        for k in _sample(self.n):
            o, n = int(w_off[k]), int(w_len[k])
            assert got[k].tobytes() == hashlib.sha256(want[o:o + n].tobytes()).digest(), k
        self.digests = got


def _sample(n, most=3000):
    return range(n) if n <= most else sorted(set(np.linspace(0, n - 1, most).astype(int).tolist()))


def _status_raises_concat(engine):
    with pytest.raises(MshaError) as ei:
        engine.device_status()
    assert ei.value.code == L.MSHA_ERR_INVALID_ARG
    text = str(ei.value)
    assert CONCAT_TEXT in text and "does not fit" in text and ">= n_lists" in text and "decreases" in text
    engine.device_status()                      # reported once, then clean


@gpu
def test_boundary_matrix_as_lists(engine):
    """tests/parts_matrix.py's batch as 1,009 lists of 0..6 parts, every source residue
    mod 16, empty parts: 1,009 workgroups of one short step each, digests equal its `want`."""
    arena, off, ln, begin, want, seen = parts_matrix.boundary_matrix()
    assert seen == set(range(16)) and begin.size - 1 == 1009
    c = Call(engine, arena, off, ln, begin)
    engine.device_status()
    c.check()
    assert np.array_equal(c.digests, want)


@gpu
def test_step_and_carry_edges(engine):
    """Lists of S-1 .. 2S+1 and 63, 64, 65 parts, lengths cycling 1..17 so that every
    destination phase occurs at a step boundary, odd source offsets, a list of empty
    parts only and one of zero parts."""
    c = Call(engine, *M.step_edges())
    engine.device_status()
    c.check()


@gpu
def test_threshold_edges(engine):
    """Parts of T-1, T, T+1 bytes at source phases 0, 1, 15 between one-byte neighbours;
    steps that sum to the image size - 1, the size, + 1; one 70,001-byte part."""
    c = Call(engine, *M.threshold_edges())
    engine.device_status()
    c.check()


@gpu
def test_epoch_change_lists_reach_the_chain_kernels(engine):
    """Three scattered EpochChanges (3,017, 5,669 and 1,817 parts; the longest 91,312
    bytes, 1,427 blocks). Once contiguous, digest_batch_device's default policy takes
    them to the cooperative chain kernel: launches_coop advances."""
    from mirbft_amd.workloads import epoch_change_parts_pool, scatter_parts
    parts = epoch_change_parts_pool(count=3, max_set=1000)
    assert [len(m) for m in parts] == [3017, 5669, 1817] and max(len(b"".join(m)) for m in parts) == 91312
    arena, off, ln, begin = scatter_parts(parts, slack=M.SLACK)
    c = Call(engine, arena, off, ln, begin)
    engine.device_status()
    before = engine.stats()["launches_coop"]
    c.check()
    assert engine.stats()["launches_coop"] > before
    assert [d.tobytes() for d in c.digests] == [hashlib.sha256(b"".join(m)).digest() for m in parts]


def _triples(rng, n_real):
    """n_real real lists at ids 0, 3, 6, ...; the two lists after each are never
    selected by the clean cases, and the begin entry only they read is poisoned (it
    decreases). -> (arena, off, ln, begin, lists)."""
    lists = [[rng.bytes(int(rng.integers(0, 90))) for _ in range(int(rng.integers(0, 6)))] for _ in range(n_real)]
    arena, off, ln, b = M._lists_to_arrays(rng, lists, lambda j: (7 * j + 2) % 16)
    begin = np.zeros(3 * n_real + 1, dtype=np.uint64)
    begin[0::3] = b
    begin[1::3] = b[1:]            # list 3i = [b[i], b[i+1])
    begin[2::3] = 0                # read by lists 3i+1 and 3i+2 only; 3i+1 decreases wherever b[i+1] > 0
    return arena, off, ln, begin, lists


@gpu
def test_select_permutation_repeats_and_subset(engine):
    rng = np.random.default_rng(0x5E1)
    arena, off, ln, begin, lists = _triples(rng, 40)
    real = 3 * np.arange(40, dtype=np.uint32)
    for sel in (real[::-1].copy(),                                      # a reversed permutation
                np.array([9, 30, 9, 3, 9, 117], dtype=np.uint32),       # an id three times
                real[5:33:3].copy()):                                   # a subset
        c = Call(engine, arena, off, ln, begin, select=sel)
        engine.device_status()                                          # poisoned unselected lists: clean
        c.check()
        assert [d.tobytes() for d in c.digests] == [hashlib.sha256(b"".join(lists[s // 3])).digest() for s in sel]


@gpu
def test_invalid_selections_are_refused_and_flagged(engine):
    """One id equal to n_lists and one selected list whose range decreases: those two
    get off = len = 0, bit 16 is reported once with INVALID_ARG and the text, every
    other message is exact; a clean call afterwards reports nothing."""
    rng = np.random.default_rng(0x5E2)
    arena, off, ln, begin, lists = _triples(rng, 40)
    n_lists = begin.size - 1
    assert begin[3 * 7 + 1] > begin[3 * 7 + 2]                          # list 22 decreases
    sel = (3 * rng.integers(0, 40, 100)).astype(np.uint32)
    sel[17], sel[60] = n_lists, 22
    c = Call(engine, arena, off, ln, begin, select=sel)
    _status_raises_concat(engine)
    model = c.model()
    assert model[4] and model[2][17] == model[3][17] == 0 == model[2][60] == model[3][60]
    c.check(model)
    assert c.digests[17].tobytes() == EMPTY == c.digests[60].tobytes()
    clean = Call(engine, arena, off, ln, begin, select=sel[:17].copy())
    engine.device_status()
    clean.check()


@gpu
def test_fit_rule(engine):
    """dst_bytes exactly the need: everything fits. One byte less: the last message is
    refused (off = len = 0, its bytes stay sentinel, the bit raised), the others exact.
    dst_bytes = 0: everything refused, nothing written."""
    rng = np.random.default_rng(0xF17)
    lists = [[rng.bytes(int(rng.integers(1, 200))) for _ in range(1 + i % 4)] for i in range(50)]
    arena, off, ln, begin = M._lists_to_arrays(rng, lists, lambda j: (3 * j) % 16)
    need = M.concat_need(ln, begin)
    c = Call(engine, arena, off, ln, begin, dst_bytes=need)
    engine.device_status()
    assert c.model()[3].all() and not c.model()[4]
    c.check()
    c = Call(engine, arena, off, ln, begin, dst_bytes=need - 1)
    _status_raises_concat(engine)
    model = c.model()
    assert model[3][:-1].all() and model[3][-1] == 0 and model[2][-1] == 0
    c.check(model)
    c = Call(engine, arena, off, ln, begin, dst_bytes=0)
    _status_raises_concat(engine)
    model = c.model()
    assert not model[2].any() and not model[3].any()
    c.check(model)
    assert (c.full.cpu().numpy() == M.SENTINEL).all()


@gpu
@pytest.mark.parametrize("n", M.scan_edge_counts())
def test_scan_edges(engine, n):
    """n one-part lists of 0..40 bytes: offsets are numpy.cumsum of round16(len)."""
    arena, off, ln, begin = M.one_part_lists(n)
    c = Call(engine, arena, off, ln, begin)
    engine.device_status()
    r16 = (ln.astype(np.int64) + 15) & ~15
    assert np.array_equal(c.msg_off.cpu().numpy(), np.concatenate([[0], np.cumsum(r16)[:-1]]))
    assert np.array_equal(c.msg_len.cpu().numpy(), ln.astype(np.int64))
    c.check()


@gpu
def test_host_refusals(engine):
    """A misaligned d_dst, n_select != n_lists without d_select, a null pointer: each
    MSHA_ERR_INVALID_ARG with its text. n_select == 0 is OK and launches nothing."""
    import torch
    rng = np.random.default_rng(0x4E)
    lists = [[rng.bytes(10), rng.bytes(9)] for _ in range(20)]
    arena, off, ln, begin = M._lists_to_arrays(rng, lists, lambda j: j % 16)
    d = [_dev(x) for x in (arena, off, ln, begin)]
    dst = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    mo = torch.zeros(20, dtype=torch.int64, device="cuda:0")
    ml = torch.zeros(20, dtype=torch.int64, device="cuda:0")
    lib, ctx = engine._lib, engine._ctx
    args = [t.data_ptr() for t in d]
    bad = L.MSHA_ERR_INVALID_ARG
    before = engine.concat_stats()
    f = lib.msha_concat_lists_device
    assert f(ctx, *args, 20, None, 20, dst.data_ptr() + 8, 4000, mo.data_ptr(), ml.data_ptr(), None) == bad
    assert b"msha_concat_lists_device: d_dst must be 16-byte aligned" in lib.msha_last_error(ctx)
    assert f(ctx, args[0] + 4, *args[1:], 20, None, 20, dst.data_ptr(), 4096, mo.data_ptr(), ml.data_ptr(), None) == bad
    assert b"d_arena must be 16-byte aligned" in lib.msha_last_error(ctx)
    assert f(ctx, *args, 20, None, 19, dst.data_ptr(), 4096, mo.data_ptr(), ml.data_ptr(), None) == bad
    assert b"must equal n_lists" in lib.msha_last_error(ctx)
    assert f(ctx, *args, 20, None, 20, dst.data_ptr(), 4096, None, ml.data_ptr(), None) == bad
    assert b"msha_concat_lists_device: null pointer" in lib.msha_last_error(ctx)
    assert f(ctx, *args, 20, None, 20, None, 4096, mo.data_ptr(), ml.data_ptr(), None) == bad
    assert b"null pointer" in lib.msha_last_error(ctx)
    assert f(ctx, *args, 0xFFFFFFFF, _dev(np.zeros(1, np.uint32)).data_ptr(), 1, dst.data_ptr(), 4096, mo.data_ptr(),
             ml.data_ptr(), None) == bad
    assert b"below 2^32 - 1" in lib.msha_last_error(ctx)
    sel = _dev(np.zeros(1, np.uint32))
    assert f(ctx, *args, 20, sel.data_ptr(), 0, dst.data_ptr(), 4096, mo.data_ptr(), ml.data_ptr(), None) == L.MSHA_OK
    assert engine.concat_stats() == before          # nothing was launched or counted
    engine.device_status()
    assert not dst.any()


@gpu
def test_capturable_into_a_graph(engine):
    """After a warm call the call captures into a HIP graph (a linear chain of three
    kernels on the caller's stream; nothing runs during the capture), and each replay
    flattens what the arena holds by then."""
    import torch
    rng = np.random.default_rng(0x6B)
    S = M.step_parts()
    lists = [[rng.bytes(int(rng.integers(0, 60))) for _ in range(int(rng.integers(0, 9)))] for _ in range(150)]
    lists[40] = [rng.bytes(int(rng.integers(0, 40))) for _ in range(S + 5)]
    lists[90] = [rng.bytes(3), rng.bytes(M.large_part() + 77)]
    arena, off, ln, begin = M._lists_to_arrays(rng, lists, lambda j: (11 * j + 5) % 16)
    c = Call(engine, arena, off, ln, begin)                             # the warm call
    engine.device_status()
    c.check()
    c.full.fill_(M.SENTINEL)
    c.msg_off.fill_(-1)
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
    assert (c.full == M.SENTINEL).all() and (c.msg_off == -1).all()
    for seed in (1, 2):
        fresh = np.random.default_rng(seed).integers(0, 256, arena.size, dtype=np.uint8)
        c.dev[0].copy_(_dev(fresh))
        c.full.fill_(M.SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        engine.device_status()
        c.check(c.model(fresh))


@gpu
def test_capture_on_a_fresh_context_fails_cleanly():
    """A fresh context has no error word and may not allocate one while the stream is
    being captured: MSHA_ERR_INVALID_ARG and the documented message, the capture ends
    empty, and the same call outside capture then works."""
    import torch
    from mirbft_amd import Engine
    rng = np.random.default_rng(0x6C)
    lists = [[rng.bytes(40), rng.bytes(41)] for _ in range(70)]
    arena, off, ln, begin = M._lists_to_arrays(rng, lists, lambda j: (j * 3) % 16)
    with Engine(1) as eng:
        s = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        c = Call(eng, arena, off, ln, begin, run=False)
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
        assert eng.concat_stats()["calls"] == 0 and (c.full == M.SENTINEL).all()
        c.run()
        eng.device_status()
        c.check()


@gpu
def test_stats(engine, monkeypatch):
    """calls, lists (messages asked for) and launches (three a call) advance; under
    MSHA_PARTS_TIMING=1 last_bytes is the model's last valid message's end and
    last_kernel_ms is set, otherwise both are 0. The other counters do not move."""
    rng = np.random.default_rng(0x57)
    lists = [[rng.bytes(int(rng.integers(0, 70))) for _ in range(3)] for _ in range(70)]
    lists[-1] = []                                                      # a valid empty message last
    arena, off, ln, begin = M._lists_to_arrays(rng, lists, lambda j: (j * 9 + 1) % 16)
    sel = np.array([5, 5, 69, 70, 2], dtype=np.uint32)                  # 70 is out of range
    others = (engine.parts_stats(), engine.parts_plan_stats())
    q0 = engine.concat_stats()
    c = Call(engine, arena, off, ln, begin)
    engine.device_status()
    c.check()
    q1 = engine.concat_stats()
    assert (q1["calls"] - q0["calls"], q1["lists"] - q0["lists"], q1["launches"] - q0["launches"]) == (1, 70, 3)
    assert (q1["last_bytes"], q1["last_kernel_ms"]) == (0, 0.0)
    monkeypatch.setenv("MSHA_PARTS_TIMING", "1")
    c = Call(engine, arena, off, ln, begin)
    q2 = engine.concat_stats()
    c2 = Call(engine, arena, off, ln, begin, select=sel)
    q3 = engine.concat_stats()
    monkeypatch.delenv("MSHA_PARTS_TIMING")
    assert c2.model()[4]
    _status_raises_concat(engine)                                       # id 70 was refused
    c.check()
    c2.check()
    assert q2["last_bytes"] == M.concat_need(ln, begin) - M.SLACK and q2["last_kernel_ms"] > 0
    m = c2.model()
    assert q3["last_bytes"] == int(m[2][4]) + M.round16(int(m[3][4])) and q3["lists"] - q2["lists"] == 5
    assert q3["calls"] - q0["calls"] == 3 and q3["launches"] - q0["launches"] == 9
    assert (engine.parts_stats(), engine.parts_plan_stats()) == others
