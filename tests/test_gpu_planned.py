"""GPU parity of msha_digest_batch_device_planned: the device-resident batch
whose lane order, alias folding and long-chain head are planned on the GPU
(plan.hip k_fold_*), checked bit-exact against the oracle (OpenSSL leg, every
distinct (off, len) hashed once) -- BASELINE config c5 at full size and per-rank
slices, the head routing forced and disabled, every kernel policy, edge cases
(one payload aliased n times, empty messages, messages past the exact block-
count buckets) and seeded fuzz."""
import os

import numpy as np
import pytest

import planned_matrix
from mirbft_amd import MshaError
from mirbft_amd import workloads as W
from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _lookback_checked(monkeypatch):
    """Every planned call here fails if a folded insert's tile look-back gave up
    waiting for an earlier tile (plan.hip tile_lookback: the digests would still be
    exact, with less folding, so only this check can see it)."""
    monkeypatch.setenv("MSHA_CHECK_LOOKBACK", "1")


def _dev(w):
    import torch
    dev = torch.device("cuda:0")
    return (torch.from_numpy(w.arena).to(dev), torch.from_numpy(w.off.view(np.int64)).to(dev),
            torch.from_numpy(w.len.view(np.int64)).to(dev))


def _expect(w, threads=16):
    if w.n == 0:
        return np.zeros((0, 32), np.uint8)
    key = np.stack([w.off, w.len], axis=1)
    uniq, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    d = oracle.openssl_digest_batch(w.arena, w.off[first], w.len[first], threads)
    return d[inv.reshape(-1)]


def _early(fold):
    """Does a planned call start an early head (read when the call is made)? Folded
    calls do, unless it is off or the head is held to the cooperative kernel
    (MSHA_HEAD_CHAIN2=0: the early head runs on the chain kernels)."""
    return (fold and os.environ.get("MSHA_EARLY_HEAD", "1") != "0"
            and os.environ.get("MSHA_HEAD_CHAIN2", "1") != "0")


def _ws(fold):
    """Does a planned call's lane kernel steal work (MSHA_LANE_WS: 1 folded calls, 2 all, 0 none)?"""
    v = os.environ.get("MSHA_LANE_WS", "1")
    return v == "2" or (v == "1" and fold)


def _chain8():
    """Does the early head run on the eight-lane kernel (k_digest_chain8)?"""
    return os.environ.get("MSHA_HEAD_CHAIN8", "1") != "0"


def _assert_head_kernels(before, after, fold):
    """Each head launch counted by its kernel (ABI 10): folded, the early head on
    k_digest_chain8 (k_digest_chain2 under MSHA_HEAD_CHAIN8=0) and the scan's cut on
    k_digest_chain2; unfolded, the cooperative kernel. A regression that routes the
    early head back to the two-lane kernel fails here."""
    c2, c8 = _delta(before, after, "launches_chain2"), _delta(before, after, "launches_chain8")
    if fold and _early(fold):
        assert (c8, c2) == ((1, 1) if _chain8() else (0, 2)), (c8, c2)
    elif fold:
        assert (c8, c2) == (0, 1), (c8, c2)
    else:
        assert (c8, c2) == (0, 0), (c8, c2)


def _run(engine, w, fold, stream=None):
    import torch
    d_arena, d_off, d_len = _dev(w)
    out = torch.full((w.n, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    engine.digest_batch_device_planned(d_arena, d_off, d_len, out, stream=stream, fold=fold)
    engine.device_status()
    return out.cpu().numpy()


def _delta(before, after, key):
    return after[key] - before[key]


@pytest.mark.parametrize("fold", [False, True])
def test_c5_full_size_planned(engine, fold):
    """BASELINE config c5 (2^23 mixed actions, aliased EpochChange pool) at full
    size, the form bench.py times as c5_planned / c5_folded: every digest."""
    import torch
    w = W.c5_storm()
    exp = _expect(w)
    before = engine.stats()
    got = _run(engine, w, fold)
    after = engine.stats()
    assert np.array_equal(got, exp)
    assert _delta(before, after, "planned_device_calls") == 1
    assert _delta(before, after, "launches_lane") == 1     # one lane launch over the whole order
    # folded: the work-stealing lane kernel (k_digest_batch_ws); unfolded: the static one
    assert _delta(before, after, "launches_lane_ws") == (1 if _ws(fold) else 0)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("fold", [False, True])
def test_c5_rank_slice_routes_long_chains(engine, world, fold):
    """A rank's slice of c5 over `world` GPUs: with folding, or at 8 GPUs, the
    longest EpochChange chains outlast the lane kernel's share and run on the
    cooperative kernel beside it (the head launch is queued whenever the batch
    is above the cooperative range; its size is decided on the GPU, MSHA_TRACE
    prints it); digests exact."""
    w = W.c5_storm(n=(1 << 23) // world)
    exp = _expect(w)
    before = engine.stats()
    got = _run(engine, w, fold)
    after = engine.stats()
    assert np.array_equal(got, exp)
    if fold or world == 8:
        # folded: the early head (the long payloads, k_fold_longs' list) and the scan's
        # cut (empty then) are two launches
        assert _delta(before, after, "launches_coop") == (2 if _early(fold) else 1)
        _assert_head_kernels(before, after, fold)
    assert _delta(before, after, "launches_lane") == 1


@pytest.mark.parametrize("chain8", [None, "0"])
def test_early_head_kernel_counted(engine, monkeypatch, chain8):
    """c5's rank slice over 8 GPUs, folded: the early head runs on k_digest_chain8
    by default and not at all under MSHA_HEAD_CHAIN8=0 (then k_digest_chain2)."""
    if chain8 is None:
        monkeypatch.delenv("MSHA_HEAD_CHAIN8", raising=False)
    else:
        monkeypatch.setenv("MSHA_HEAD_CHAIN8", chain8)
    w = W.c5_storm(n=(1 << 23) // 8, first=3)
    before = engine.stats()
    assert np.array_equal(_run(engine, w, True), _expect(w))
    after = engine.stats()
    c2, c8 = _delta(before, after, "launches_chain2"), _delta(before, after, "launches_chain8")
    assert (c8, c2) == ((1, 1) if chain8 is None else (0, 2)), (c8, c2)


@pytest.mark.parametrize("pct", ["1", "100000"])
def test_head_forced_and_empty(engine, monkeypatch, pct):
    """The head's cost term in the GPU planner's cut scaled to 1 % (a nearly
    free head: the cut takes as many lanes as pays) and to 1000x (no head)."""
    monkeypatch.setenv("MSHA_PLAN_HEAD_PCT", pct)
    w = W.c5_storm(n=1 << 18, first=12345)
    exp = _expect(w)
    for fold in (False, True):
        assert np.array_equal(_run(engine, w, fold), exp)


@pytest.mark.parametrize("chain2", ["0", "2"])
def test_head_kernel_either_way(engine, monkeypatch, chain2):
    """The head runs on the two-lane chain kernel (k_digest_chain2: folded calls
    by default) or the cooperative one (unfolded by default); force each the
    other way, with a large head (cost scaled down) and the default one."""
    monkeypatch.setenv("MSHA_HEAD_CHAIN2", chain2)
    w = W.c5_storm(n=1 << 17, first=4242)
    exp = _expect(w)
    for pct in ("1", "100"):
        monkeypatch.setenv("MSHA_PLAN_HEAD_PCT", pct)
        for fold in (False, True):
            assert np.array_equal(_run(engine, w, fold), exp)


def test_head_disabled(engine, monkeypatch):
    monkeypatch.setenv("MSHA_PLAN_HEAD", "0")
    w = W.c5_storm(n=1 << 17)
    before = engine.stats()
    assert np.array_equal(_run(engine, w, True), _expect(w))
    assert _delta(before, engine.stats(), "launches_coop") == 0


@pytest.mark.parametrize("policy", ["lane", "coop"])
def test_policies(engine, policy):
    engine.set_kernel_policy(policy)
    try:
        w = W.c5_storm(n=1 << 16, first=777)
        exp = _expect(w)
        for fold in (False, True):
            assert np.array_equal(_run(engine, w, fold), exp)
    finally:
        engine.set_kernel_policy("auto")


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 32768, 32769, 65536, 65537, 300_000])
def test_one_payload_aliased(engine, n):
    """n actions all naming one 5,000-byte payload: folded, one lane hashes it
    and the fill copies its digest everywhere; unfolded, every lane hashes it."""
    arena = W.random_bytes(W.SEED ^ 0x77, 0, 5000 + 64)
    w = W.Workload("aliased", arena, np.zeros(n, np.uint64), np.full(n, 5000, np.uint64))
    exp = np.tile(oracle.digest_batch(arena, np.zeros(1, np.uint64), np.full(1, 5000, np.uint64)), (n, 1))
    assert np.array_equal(_run(engine, w, True), exp)
    assert np.array_equal(_run(engine, w, False), exp)


def test_fold_table_grows_after_small_calls(monkeypatch):
    """The epoch-tagged alias table (plan.hip fold_claim) must be cleared whenever it
    grows, whatever address the new allocation gets (a regrown
    table at the old address kept its uncleared tail). Small folded calls move the
    epoch past 1, then a larger call grows the table; MSHA_POISON_FOLD_TABLE fills
    the fresh allocation with words tagged with the coming epoch, as recycled
    memory may hold, so a table left uncleared claims garbage indices. Every digest
    of every call must be exact."""
    from mirbft_amd import Engine
    monkeypatch.setenv("MSHA_POISON_FOLD_TABLE", "1")
    with Engine(1) as e:
        for n in (4096, 4096, 4096, 1 << 18, 1 << 18, 1 << 19):
            w = W.c5_storm(n)
            assert np.array_equal(_run(e, w, True), _expect(w)), n


def test_empty_and_boundary_lengths(engine):
    lens = np.array([0, 0, 1, 55, 56, 63, 64, 65, 119, 120, 0, 128, 4096 * 64 - 9, 4096 * 64,
                     300_000, 1 << 20, 0] * 50, dtype=np.uint64)
    off = np.zeros(lens.size, np.uint64)
    off[1:] = np.cumsum((lens + np.uint64(15)) // np.uint64(16) * np.uint64(16))[:-1]
    arena = W.random_bytes(W.SEED ^ 0x78, 0, int(off[-1] + lens[-1]) + 64)
    w = W.Workload("boundary", arena, off, lens)
    exp = _expect(w)
    for fold in (False, True):
        assert np.array_equal(_run(engine, w, fold), exp)


@pytest.mark.parametrize("ws", ["0", "2"])
@pytest.mark.parametrize("seed", range(4))
def test_fuzz_lane_kernels(engine, monkeypatch, seed, ws):
    """The static and the work-stealing lane kernels forced either way (MSHA_LANE_WS=0:
    static everywhere, 2: work stealing on unfolded calls too), over batches whose lane
    counts are not multiples of a tile, with long chains left on the lane kernel, heads
    and folded tails: every digest exact, the kernel counted."""
    monkeypatch.setenv("MSHA_LANE_WS", ws)
    rng = np.random.default_rng(7000 + seed)
    n = int(rng.choice([40_001, 77_777, 150_000, 300_003]))
    ln = rng.integers(0, 1200, n).astype(np.uint64)
    big = rng.random(n) < 0.002
    ln[big] = rng.integers(20_000, 200_000, int(big.sum())).astype(np.uint64)
    off, arena = _packed(ln, 0x7000 + seed)
    if seed % 2:  # 20 % alias an earlier message (folded tails of kNoLane positions)
        src = rng.integers(0, n, n)
        al = (rng.random(n) < 0.2) & (src < np.arange(n))
        off[al], ln[al] = off[src[al]], ln[src[al]]
    w = W.Workload(f"lanefuzz{seed}", arena, off, ln)
    exp = _expect(w, 8)
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for fold in (False, True):
        before = engine.stats()
        assert np.array_equal(_run(engine, w, fold), exp)
        # at most one wave per SIMD the pipelined kernel runs instead (kernels.hip pick_mode)
        ws_ran = _ws(fold) and n > cus * 4 * 64
        assert _delta(before, engine.stats(), "launches_lane_ws") == int(ws_ran), (n, fold)


@pytest.mark.parametrize("seed", range(12))
def test_fuzz(engine, seed):
    """Random sizes (mostly small, a few up to 400 KB), aligned starts, packed /
    aliased / reversed / overlapping-window layouts, folding on and off."""
    rng = np.random.default_rng(4000 + seed)
    n = int(rng.choice([1, 7, 100, 5000, 40_000, 120_000]))
    ln = rng.integers(0, 2000, n).astype(np.uint64)
    big = rng.random(n) < 0.005
    ln[big] = rng.integers(10_000, 400_000, int(big.sum())).astype(np.uint64)
    kind = int(rng.integers(0, 4))
    steps = (ln + np.uint64(15)) // np.uint64(16) * np.uint64(16)
    off = np.concatenate([[0], np.cumsum(steps)[:-1]]).astype(np.uint64)
    size = int(off[-1] + ln[-1])
    if kind == 1 and n > 1:                          # 30 % alias an earlier message
        src = rng.integers(0, n, n)
        al = (rng.random(n) < 0.3) & (src < np.arange(n))
        off[al], ln[al] = off[src[al]], ln[src[al]]
    elif kind == 2:                                  # reversed arena order
        off = off[::-1].copy()
        ln = ln[::-1].copy()
    elif kind == 3:                                  # overlapping windows, 16-B aligned
        size = int(ln.max()) + 8000
        off = (rng.integers(0, 500, n) * 16).astype(np.uint64)
    arena = W.random_bytes(W.SEED ^ (0x900 + seed), 0, size + 64)
    w = W.Workload(f"fuzz{seed}", arena, off, ln)
    exp = _expect(w, 8)
    for fold in (False, True):
        assert np.array_equal(_run(engine, w, fold), exp)


def test_on_a_caller_stream(engine):
    """Enqueued on the caller's stream (the head forked to the side stream and
    joined back): the digests are complete once that stream is synchronized."""
    import torch
    s = torch.cuda.Stream()
    w = W.c5_storm(n=1 << 20, first=99)
    d_arena, d_off, d_len = _dev(w)
    out = torch.zeros((w.n, 32), dtype=torch.uint8, device="cuda:0")
    engine.digest_batch_device_planned(d_arena, d_off, d_len, out, stream=s, fold=True)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), _expect(w))
    engine.device_status()


def test_calls_on_two_streams(engine):
    """Back-to-back planned calls on two streams share the context's planner
    scratch: the second waits for the first (ev_fdone), both digest sets exact."""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    w1 = W.c5_storm(n=1 << 19, first=5)
    w2 = W.c5_storm(n=(1 << 18) + 77, first=1 << 22)
    a1, o1, l1 = _dev(w1)
    a2, o2, l2 = _dev(w2)
    out1 = torch.zeros((w1.n, 32), dtype=torch.uint8, device="cuda:0")
    out2 = torch.zeros((w2.n, 32), dtype=torch.uint8, device="cuda:0")
    for _ in range(3):
        engine.digest_batch_device_planned(a1, o1, l1, out1, stream=s1, fold=True)
        engine.digest_batch_device_planned(a2, o2, l2, out2, stream=s2, fold=False)
    torch.cuda.synchronize()
    engine.device_status()
    assert np.array_equal(out1.cpu().numpy(), _expect(w1))
    assert np.array_equal(out2.cpu().numpy(), _expect(w2))


def test_misaligned_flagged(engine):
    import torch
    arena = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    off = torch.tensor([0, 8, 16], dtype=torch.int64, device="cuda:0")
    ln = torch.tensor([10, 10, 10], dtype=torch.int64, device="cuda:0")
    out = torch.full((3, 32), 0xAB, dtype=torch.uint8, device="cuda:0")
    engine.digest_batch_device_planned(arena, off, ln, out, fold=True)
    with pytest.raises(MshaError):
        engine.device_status()
    assert (out[1] == 0).all()


def test_bad_flags(engine):
    import torch
    from mirbft_amd import _lib as L
    t = torch.zeros(64, dtype=torch.uint8, device="cuda:0")
    o = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    rc = L.lib().msha_digest_batch_device_planned(engine._ctx, t.data_ptr(), o.data_ptr(), o.data_ptr(), 1,
                                                  2, t.data_ptr(), None)
    assert rc == L.MSHA_ERR_INVALID_ARG


@pytest.mark.parametrize("early", ["0", "1"])
def test_early_head(engine, monkeypatch, early):
    """Folded calls with the early head (MSHA_EARLY_HEAD=1: the distinct payloads of
    >= 256 blocks claimed and listed by the planner's first pass, before the alias
    insert, and started on the two-lane kernel right then) and without: c5 slices at 1 and 8 GPUs, a batch
    whose long payloads are too many for the early head (it stands down and the
    scan's cut decides), and long payloads first named by a fresh message; every
    digest exact, the two head launches counted."""
    monkeypatch.setenv("MSHA_EARLY_HEAD", early)
    for world in (1, 8):
        w = W.c5_storm(n=(1 << 23) // world // 4, first=world)
        before = engine.stats()
        assert np.array_equal(_run(engine, w, True), _expect(w))
        assert _delta(before, engine.stats(), "launches_coop") == (2 if _early(True) else 1)
    # 3,000 distinct 300-block payloads (> 256 CUs x 64 / 8): no early head
    rng = np.random.default_rng(300)
    n = 60_000
    ln = np.full(n, 512, np.uint64)
    longs = rng.choice(n, 3000, replace=False)
    ln[longs] = 300 * 64 - 20
    off = np.concatenate([[0], np.cumsum((ln + np.uint64(15)) // np.uint64(16) * np.uint64(16))[:-1]]).astype(np.uint64)
    # every long payload named again by a later message (aliases of fresh ones)
    alias = rng.choice(n, 3000, replace=False)
    off[alias], ln[alias] = off[longs], ln[longs]
    arena = W.random_bytes(W.SEED ^ 0x300, 0, int(off.max() + ln.max()) + 64)
    w = W.Workload("many-longs", arena, off, ln)
    assert np.array_equal(_run(engine, w, True), _expect(w))


def _packed(ln, seed):
    off = np.concatenate([[0], np.cumsum((ln + np.uint64(15)) // np.uint64(16) * np.uint64(16))[:-1]]).astype(np.uint64)
    arena = W.random_bytes(W.SEED ^ seed, 0, int(off[-1] + ln[-1]) + 64)
    return off, arena


@pytest.mark.parametrize("case", ["clustered", "many_in_one_tile", "huge"])
def test_early_head_batches(engine, monkeypatch, case):
    """Folded batches around the early head's list (k_fold_longs): long payloads
    named only inside a few tiles of 4,096 messages each (the early head runs);
    600 distinct long payloads in the first tile with the two-lane early head
    (cap 2,048: it runs on 600 chains); a 16 MiB + 100 B payload named four
    times among 50,000 requests. Every digest exact."""
    rng = np.random.default_rng(0xE4)
    if case == "clustered":
        n = 200_000
        ln = np.full(n, 512, np.uint64)
        src = rng.choice(n, 300, replace=False)
        ln[src] = rng.integers(260 * 64, 700 * 64, src.size).astype(np.uint64)
        off, arena = _packed(ln, 0xE41)
        for s in src:  # four more names of each, within 6,000 messages of it
            near = np.clip(s + rng.integers(-6000, 6000, 4), 0, n - 1)
            near = near[near != s]
            off[near], ln[near] = off[s], ln[s]
    elif case == "many_in_one_tile":
        monkeypatch.setenv("MSHA_HEAD_CHAIN8", "0")
        n = 50_000
        ln = np.full(n, 512, np.uint64)
        src = rng.choice(4096, 600, replace=False)
        ln[src] = 257 * 64
        off, arena = _packed(ln, 0xE42)
        dup = rng.choice(np.arange(4096, n), 600, replace=False)
        off[dup], ln[dup] = off[src], ln[src]
    else:
        n = 50_000
        ln = np.full(n, 512, np.uint64)
        ln[7] = (1 << 24) + 100
        ln[9000] = 300 * 64
        off, arena = _packed(ln, 0xE43)
        for d in (20_000, 30_000, 40_000):
            off[d], ln[d] = off[7], ln[7]
        off[45_000], ln[45_000] = off[9000], ln[9000]
    w = W.Workload(f"early-head {case}", arena, off, ln)
    before = engine.stats()
    assert np.array_equal(_run(engine, w, True), _expect(w))
    _assert_head_kernels(before, engine.stats(), True)


@pytest.fixture(scope="module")
def backrefs():
    """Every tile of 4,096 messages names payloads of the tile before it again (10 %)."""
    rng = np.random.default_rng(0x1B)
    n = 300_000
    ln = rng.integers(0, 700, n).astype(np.uint64)
    off, arena = _packed(ln, 0xE44)
    back = rng.random(n) < 0.1
    src = np.clip(np.arange(n) - 4096 - rng.integers(0, 4096, n), 0, n - 1)
    off[back], ln[back] = off[src[back]], ln[src[back]]
    w = W.Workload("tile-backrefs", arena, off, ln)
    return w, _expect(w)


def test_tile_backrefs(engine, backrefs):
    """Candidates-first folding across tiles: a message skips the alias table only when its offset
    is above every earlier message's, carried from tile to tile by the insert's look-back."""
    assert np.array_equal(_run(engine, backrefs[0], True), backrefs[1])


def _model_lanes(w):
    """The folded planner's lane count on the host: the rule lives in tests/planned_matrix.py
    (fresh messages, plus one claimant per distinct key among the rest; a call of this size
    tries an early head, so a long message is never fresh)."""
    return planned_matrix.model_lanes(w.off, w.len, early_on=True)


@pytest.mark.parametrize("case", ["backrefs", "c5"])
def test_lanes_match_host_model(engine, monkeypatch, capfd, backrefs, case):
    """A folded call's lane count (MSHA_TRACE_PLAN prints the GPU's plan) equals the host
    model's, digests exact: the tile-backrefs workload, the only one here whose earlier tiles
    demote messages in the insert's second pass (297,895 lanes = 269,840 fresh + 28,055
    claimants), and a c5 slice (996,126 lanes; 50,434 long messages fold to 100 claimants)."""
    w = backrefs[0] if case == "backrefs" else W.c5_storm(n=1 << 20)
    want = _model_lanes(w)
    assert want == {"backrefs": 297_895, "c5": 996_126}[case]
    monkeypatch.setenv("MSHA_TRACE_PLAN", "1")
    capfd.readouterr()
    assert np.array_equal(_run(engine, w, True), backrefs[1] if case == "backrefs" else _expect(w))
    lines = [l for l in capfd.readouterr().err.splitlines() if "planned device call" in l]
    assert len(lines) == 1 and int(lines[0].split(",")[1].split()[0]) == want, lines


def test_lookback_give_up_exact(engine, monkeypatch):
    """The tile look-back's give-up path (plan.hip tile_lookback: after a bounded wait a
    tile takes the largest threshold, so none of its messages -- nor, through its post,
    any later tile's -- is fresh and every one claims in the alias table): the digests
    stay exact, and MSHA_CHECK_LOOKBACK reports it. The product kernels only take it
    when a wait outlasts 2^16 polls, so a -DMSHA_LOOKBACK_GIVEUP_TEST build forces it on
    every third tile (tools/r06_race.sh). A c5 slice."""
    from mirbft_amd import _lib
    if "-DMSHA_LOOKBACK_GIVEUP_TEST" not in _lib.build_id()["flags"].split():
        pytest.skip("needs a -DMSHA_LOOKBACK_GIVEUP_TEST build (tools/r06_race.sh)")
    w = W.c5_storm(n=(1 << 23) // 8)
    exp = _expect(w)
    monkeypatch.setenv("MSHA_CHECK_LOOKBACK", "0")
    assert np.array_equal(_run(engine, w, True), exp)
    monkeypatch.setenv("MSHA_CHECK_LOOKBACK", "1")
    with pytest.raises(MshaError, match="look-back gave up"):
        _run(engine, w, True)


@pytest.mark.parametrize("world", [2, 8])
def test_early_head_insert_claims_first(engine, monkeypatch, world):
    """The planner's defensive check (k_fold_scatter resolves the heads): should the
    early head's list ever miss a long lane, nothing is skipped. The product kernels cannot reach that state
    (k_fold_longs claims every long message, so it lists every claimant: ADVICE r5),
    so it is forced in a test build only (-DMSHA_FOLD_RACE_TEST; tools/r06_race.sh
    runs this test on one): MSHA_FOLD_LONGS_SKIP_ODD=1 leaves about half the long
    payloads unlisted, and the late head and the lane kernel must hash every lane.
    c5 slices; every digest exact."""
    from mirbft_amd import _lib
    if "-DMSHA_FOLD_RACE_TEST" not in _lib.build_id()["flags"].split():
        pytest.skip("needs a -DMSHA_FOLD_RACE_TEST build (tools/r06_race.sh); the product kernels cannot "
                    "leave a long lane off the list")
    monkeypatch.setenv("MSHA_FOLD_LONGS_SKIP_ODD", "1")
    w = W.c5_storm(n=(1 << 23) // world // 2, first=3 * world)
    assert np.array_equal(_run(engine, w, True), _expect(w))


def test_big_bucket_messages_head(engine, monkeypatch):
    """Messages of 4,096 blocks or more share power-of-two block-count classes;
    the planner's head cost model reads each class's real longest chain and
    block sum (k_fold_keys). A batch whose longest chains sit in those classes
    (5,000 - 9,000 blocks, one class) among many small requests: every digest
    exact, folded and not, with the head on either kernel."""
    rng = np.random.default_rng(4096)
    n = 40_000
    ln = np.full(n, 512, np.uint64)
    longs = rng.choice(n, 24, replace=False)
    ln[longs] = rng.integers(5000 * 64, 9000 * 64, longs.size).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum((ln + np.uint64(15)) // np.uint64(16) * np.uint64(16))[:-1]]).astype(np.uint64)
    arena = W.random_bytes(W.SEED ^ 0x4096, 0, int(off[-1] + ln[-1]) + 64)
    w = W.Workload("big-bucket", arena, off, ln)
    exp = _expect(w)
    for chain2 in ("0", "2"):
        monkeypatch.setenv("MSHA_HEAD_CHAIN2", chain2)
        for fold in (False, True):
            before = engine.stats()
            assert np.array_equal(_run(engine, w, fold), exp)
            # the long chains got a head (folded on the two-lane kernel: the early
            # head and the scan's cut, two launches)
            assert _delta(before, engine.stats(), "launches_coop") == (2 if _early(fold) else 1)


def test_graph_capture_refused_cleanly(engine):
    """The planned call cannot be captured into a HIP graph (mirsha.h): on a
    capturing stream it fails with MSHA_ERR_INVALID_ARG and names the reason,
    and the context keeps working afterwards."""
    import torch
    from mirbft_amd import _lib as L
    w = W.c5_storm(n=1 << 12, first=3)
    d_arena, d_off, d_len = _dev(w)
    out = torch.zeros((w.n, 32), dtype=torch.uint8, device="cuda:0")
    assert np.array_equal(_run(engine, w, True), _expect(w))   # scratch allocated outside the capture
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    err = None
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            engine.digest_batch_device_planned(d_arena, d_off, d_len, out, stream=s, fold=True)
        except MshaError as e:
            err = e
        finally:
            g.capture_end()
    assert err is not None and err.code == L.MSHA_ERR_INVALID_ARG and "graph" in str(err)
    torch.cuda.synchronize()
    assert np.array_equal(_run(engine, w, True), _expect(w))
