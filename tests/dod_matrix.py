"""Digest-of-digests matrix: case generator and runner (not collected by pytest).

k_digest_of_digests and the DigestSrc form of k_digest_split (mirbft_amd/csrc/
kernels.hip) hash the Batch / VerifyBatch digests: out[i] = SHA-256 of the table
rows idx[begin[i] : begin[i+1]] joined. The code decides per wave how the indices
are read (staged in LDS or straight from idx), per wave how the final block is
built (padded on the SALU for a wave of one even count, per lane otherwise), per
count how the pair loop ends (four digests a step, then two, then one), per surplus
chain how its blocks are cut into segments, and per host call how a batch is cut
into shards. This module builds batches from COUNT PATTERNS that sit on those
decisions, crosses them with INDEX PATTERNS, and aims them at TARGETS: an entry
point, a batch size as a function of the CU count, a policy and an environment,
and the msha_stats counter deltas that prove which kernel ran.

tests/test_dod_matrix_cpu.py checks from `begin` alone that the cases reach every
cell they promise, that every n gives the kernel its target claims, and that a
model of the kernel with one seeded fault at a time changes a digest of some case;
tests/test_gpu_dod_matrix.py runs the cases, bit-exact. The expected digests never
come from the engine: hashlib over the joined rows up to HASHLIB_MAX messages, the
oracle's scalar leg above (the CPU test checks that the two agree).

Not reached by any case: a `begin` past 2^32. k0 and the span of a wave travel
through pairs of 32-bit readfirstlane / readlane, and their high halves are
nonzero only with more than 2^32 indices, 16 GiB of idx.

No GPU code here; torch is imported only when a case runs.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import kernel_matrix as KM  # noqa: E402 -- plan_split, the batch launcher's ladder, _salt, check_deltas

WAVE = 64
PARTIAL_LANES = 37              # every n is 64 k - 27
COUNTERS = KM.COUNTERS + ("launches_dod", "small_calls")
HASHLIB_MAX = 4096              # messages; above, the oracle computes the expected digests

U_EVEN, U_ODD, NEAR0, NEAR_OTHER, RAGGED = range(5)
KIND_NAMES = ("uniform-even", "uniform-odd", "near-uniform (lane 0 odd)", "near-uniform (another lane odd)",
              "ragged")


# ---------------------------------------------------------------------------
# The launch rules, restated
# ---------------------------------------------------------------------------
MAX_SEGMENTS_DOD = 12           # kernels.hpp:63 kMaxSegmentsDod
IDX_STAGE = 1536                # kernels.hip:700 DigestSrc::kIdxStage
PER_LANE = IDX_STAGE // WAVE    # kernels.hip:715 kPer: 24 staged indices a lane
SMALL_MSGS = 65536              # host_plan.hpp small_msgs()
SMALL_DOD_BYTES = 1 << 20       # host_plan.hpp kSmallDodBytes
SMALL_BYTES = 4 << 20           # host_plan.hpp small_bytes(), MSHA_SMALL_BYTES


def plan_split(n, c, policy="auto"):
    """kernels.hip:1770 plan_split() with cap kMaxSegmentsDod (the split_for calls of
    host_entries.cpp msha_digest_of_digests and device_batch.cpp msha_digest_of_digests_device):
    None, or n_main, chains, segments and groups."""
    sp = KM.plan_split(n, c, policy)
    if sp is None:
        return None
    n_main, r = sp
    return {"n_main": n_main, "chains": r, "segments": min(MAX_SEGMENTS_DOD, max(2, 4 * c // r)),
            "groups": ((r + 3) // 4 + 7) // 8 * 8}


def is_staged(span, act):
    """kernels.hip:716: a wave of `act` active lanes stages its span of idx in LDS."""
    return span <= PER_LANE * act


def host_small(n, n_idx, small_bytes=SMALL_BYTES):
    """host_entries.cpp msha_digest_of_digests (host_plan.hpp small_call): the host entry packs the rows and hashes
    them as plain messages."""
    return small_bytes > 0 and n <= SMALL_MSGS and 32 * n_idx <= small_bytes and 32 * n_idx <= SMALL_DOD_BYTES


def chain_blocks(cnt):
    """kernels.hip:749: nb = cnt / 2 + 1 (also host_plan.hpp blocks_for(32 cnt))."""
    return np.asarray(cnt, dtype=np.int64) // 2 + 1


def segment_bounds(nb, seg, segments):
    """kernels.hip:797-798: segment seg hashes blocks [b0, b1)."""
    return nb * seg // segments, nb * (seg + 1) // segments


def shard_bounds(counts, k):
    """host_plan.hpp partition(): bounds[s] = the first message whose block
    range's midpoint reaches s / k of all blocks."""
    b = chain_blocks(counts)
    n = len(b)
    if k == 1:
        return [0, n]
    acc = np.cumsum(b) - b
    total = int(b.sum())
    out = [0]
    for s in range(1, k):
        hit = np.nonzero(2 * k * acc + k * b >= 2 * s * total)[0]
        out.append(int(hit[0]) if hit.size else n)
    return out + [n]


def small_launch(n, c):
    """The launch counters of a small call's one batch kernel (run_small passes no
    split; kernels.hip:1839-1874 launch_digest_batch under policy auto)."""
    if KM.uses_coop(n, c, "auto"):
        if n <= c * KM.CHAIN8_PER_WG:
            return {"launches_coop": 1, "launches_chain8": 1}
        if n <= c * KM.CHAIN2_PER_WG:
            return {"launches_coop": 1, "launches_chain2": 1}
        return {"launches_coop": 1}
    return {"launches_pipe": 1} if KM.pick_mode(n, c) == 3 else {"launches_lane": 1}


# ---------------------------------------------------------------------------
# Cells (what a launch exercises, from `begin` alone)
# ---------------------------------------------------------------------------
def _counts(begin, n):
    b = np.asarray(begin, dtype=np.uint64)[:n + 1].astype(np.int64)
    return b[1:] - b[:-1]


def final_kind(w):
    """The final-block kind of one wave's counts (kernels.hip:683-692): only a wave
    of one even count pads on the SALU."""
    if (w == w[0]).all():
        return U_EVEN if w[0] % 2 == 0 else U_ODD
    if len(w) > 2 and (w[1:] == w[1]).all():
        return NEAR0
    if (w != w[0]).sum() == 1:
        return NEAR_OTHER
    return RAGGED


def wave_cells(begin, n):
    """Per 64-message wave of the lanes [0, n) that run DigestSrc::full: (staged,
    final-block kind, partial wave, wave slot in its workgroup)."""
    cnt = _counts(begin, n)
    out = []
    for k, s in enumerate(range(0, n, WAVE)):
        w = cnt[s:s + WAVE]
        out.append((is_staged(int(w.sum()), len(w)), final_kind(w), len(w) < WAVE, k % 4))
    return out


def edge_cells(begin, n):
    """{(active lanes, span - 24 act, who holds the span)} of the waves on the stage
    edge (span - 24 act in {0, 1}): "spread" (no lane above 25), or one lane holding
    all of it, "first", "middle" or "last" of the wave."""
    cnt = _counts(begin, n)
    out = set()
    for s in range(0, n, WAVE):
        w = cnt[s:s + WAVE]
        d = int(w.sum()) - PER_LANE * len(w)
        if d not in (0, 1):
            continue
        nz = np.nonzero(w)[0]
        if w.max() <= PER_LANE + 1:
            who = "spread"
        elif nz.size == 1:
            who = "first" if nz[0] == 0 else ("last" if nz[0] == len(w) - 1 else "middle")
        else:
            who = "other"
        out.add((len(w), d, who))
    return out


def count_cell(cnt):
    return (int(cnt) % 4, int(cnt) >= 4, int(cnt) == 0)


def count_cells(begin, n):
    """{(cnt mod 4, cnt >= 4, cnt == 0)} over the counts present."""
    return {count_cell(v) for v in np.unique(_counts(begin, n))}


def segment_cells(begin, n, c, policy="auto"):
    """Per surplus chain lane of a split launch of n messages: (nb against the
    segment count: -1 less, 0 equal, 1 greater; cnt parity; some segment empty)."""
    sp = plan_split(n, c, policy)
    if sp is None:
        return []
    cnt = _counts(begin, n)[sp["n_main"]:]
    segs = sp["segments"]
    out = []
    for v in cnt:
        nb = int(v) // 2 + 1
        empty = any(b0 == b1 for b0, b1 in (segment_bounds(nb, s, segs) for s in range(segs)))
        out.append(((nb > segs) - (nb < segs), int(v) % 2, empty))
    return out


# ---------------------------------------------------------------------------
# Count patterns. Each builder fills a region of lanes that run DigestSrc::full (a
# whole unsplit launch with its partial last wave, or a split launch's main
# workgroups) and says in its docstring which cells it promises;
# tests/test_dod_matrix_cpu.py restates those promises and compares.
# ---------------------------------------------------------------------------
UNIFORM_COUNTS = 34             # 0..33: every cnt mod 4 below and from 4, both sides of 24 a lane
NEAR_BASE = (0, 1, 2, 20, 21, 24)
NEAR_LANES = (0, 1, 37, 63)     # lane 0: readfirstlane returns the odd count
FILL_MOD = 16                   # the filler after a pattern's designed waves: ragged, 7.5 digests a message


def ragged(n, start=0, mod=48):
    """Message i has count (i * 7919) mod 48 (7919 = -1 mod 48: the counts walk
    down through 47..0), mean 23.5: no wave is uniform or near-uniform, and a wave's
    span runs from 1,248 to 1,760 with its start, either side of the 1,536 staged.
    Promises: ragged waves staged and direct in every wave slot, every count cell."""
    i = np.arange(start, start + n, dtype=np.int64)
    return (i * 7919) % mod


def uniform_waves(n, down, tail):
    """Wave k is entirely of count k mod 34 (down: 33 - k mod 34), the partial last
    wave (if n has one) of `tail`. Promises: uniform-even and uniform-odd waves,
    staged up to count 24 and direct from 25, every count cell of 0..33; between
    the two directions also on a device with fewer than 34 waves."""
    k = np.arange(n, dtype=np.int64) // WAVE % UNIFORM_COUNTS
    cnt = UNIFORM_COUNTS - 1 - k if down else k
    if n % WAVE:
        cnt[n - n % WAVE:] = tail
    return cnt


def near_odd_counts(base):
    return sorted({base + 1, base + 2, 0} - {base})


def near_combos(lane):
    """(base, odd lane, odd count) of near_uniform's waves for one odd lane: 17."""
    return [(b, lane, o) for b in NEAR_BASE for o in near_odd_counts(b)]


def near_uniform(n, lane, start=0, tail=None):
    """Wave w is 64 messages of base count with lane `lane` of the odd count, over
    near_combos(lane); then the filler. 63 x 20 with one 22 is the wave of even
    counts that differ; 63 x 24 with one 25 the first direct wave. Promises:
    near-uniform waves with lane 0 odd (lane == 0) or another lane odd, staged (and,
    base 24, direct)."""
    cnt = ragged(n, start, FILL_MOD)
    for w, (b, j, o) in enumerate(near_combos(lane)):
        cnt[w * WAVE:(w + 1) * WAVE] = b
        cnt[w * WAVE + j] = o
    if tail is not None and n % WAVE:
        cnt[n - n % WAVE:] = tail
    return cnt


def edge_wave(act, delta, who):
    """One wave of `act` lanes with span 24 act + delta: spread evenly (delta 1: the
    middle lane holds one more), or all of it in the first, middle or last lane."""
    w = np.zeros(act, dtype=np.int64)
    if who == "spread":
        w[:] = PER_LANE
        w[act // 2] += delta
    else:
        w[{"first": 0, "middle": act // 2, "last": act - 1}[who]] = PER_LANE * act + delta
    return w


EDGE_FORMS = [(d, who) for who in ("spread", "first", "middle", "last") for d in (0, 1)]


def stage_edges(n, tail_form=None, start=0):
    """Waves 0..7 are the eight full-wave forms of EDGE_FORMS (span exactly 24 x 64
    and one more; spread, and one lane holding everything); the partial last wave,
    if any, is form `tail_form` at 37 lanes; the filler between. Promises: both
    stage edges at 64 lanes (and at 37), uniform-even, near-uniform (lane 0 and
    another) on either side of the edge."""
    cnt = ragged(n, start, FILL_MOD)
    for w, (d, who) in enumerate(EDGE_FORMS):
        cnt[w * WAVE:(w + 1) * WAVE] = edge_wave(WAVE, d, who)
    if tail_form is not None:
        assert n % WAVE == PARTIAL_LANES
        cnt[n - PARTIAL_LANES:] = edge_wave(PARTIAL_LANES, *EDGE_FORMS[tail_form])
    return cnt


def segments(c, r):
    """The surplus lanes of a split launch of r chains on c CUs: lane j has parity
    j mod 2 and nb = 1 + (j / 2) mod (segments + 2) blocks, so nb walks 1 ..
    segments + 2 in both parities within 2 (segments + 2) <= 28 lanes. Promises:
    every segment cell: nb below (empty segments), at and above the segment count,
    the final block holding an odd digest or the length alone."""
    segs = min(MAX_SEGMENTS_DOD, max(2, 4 * c // r))
    j = np.arange(r * WAVE - (WAVE - PARTIAL_LANES), dtype=np.int64)
    return 2 * ((j // 2) % (segs + 2)) + j % 2


def zero_runs():
    """Three ragged stretches of 200 messages with runs of 3,000 empty messages
    between them: with three shards both boundaries (at 1/3 and 2/3 of the blocks)
    fall inside a run."""
    z = np.zeros(3000, dtype=np.int64)
    return np.concatenate([ragged(200), z, ragged(200, 200), z, ragged(200, 400)])


# ---------------------------------------------------------------------------
# Index patterns
# ---------------------------------------------------------------------------
INDEX_PATTERNS = ("contiguous", "random", "one_row", "table1")
RANDOM_ROWS = 4099


def build_index(index_pattern, n_idx, salt):
    """(table, idx). Table rows are random and pairwise distinct (the row number in
    the first four bytes). contiguous: idx = arange, the Batch shape; random: over
    4,099 rows, no two neighbouring entries equal, so a lane that reads one index off
    gets another row; one_row: every index the table's last row; table1: a table of
    exactly one row."""
    rng = np.random.default_rng(salt)
    if index_pattern == "contiguous":
        rows, idx = max(n_idx, 1), np.arange(n_idx, dtype=np.uint32)
    elif index_pattern == "random":
        rows = RANDOM_ROWS
        idx = (np.cumsum(rng.integers(1, rows, n_idx, dtype=np.int64)) % rows).astype(np.uint32)
    elif index_pattern == "one_row":
        rows, idx = RANDOM_ROWS, np.full(n_idx, RANDOM_ROWS - 1, dtype=np.uint32)
    elif index_pattern == "table1":
        rows, idx = 1, np.zeros(n_idx, dtype=np.uint32)
    else:
        raise KeyError(index_pattern)
    table = rng.integers(0, 256, size=(rows, 32), dtype=np.uint8)
    table[:, :4] = np.arange(rows, dtype="<u4").view(np.uint8).reshape(rows, 4)
    return table, idx


# ---------------------------------------------------------------------------
# Targets
# ---------------------------------------------------------------------------
N_UNSPLIT = 64 * 250 - 27       # 250 waves: no split on 8 CUs (r = 26 > 16) nor from 64 CUs on (q = 0)
N_SMALL = 64 * 20 - 27          # 1,253 ragged Batches: 29,445 indices, under the small path's 1 MiB of rows

FULL_PATTERNS = ("uniform_up", "uniform_down", "near_uniform_l0", "near_uniform_l1", "near_uniform_l37",
                 "near_uniform_l63") + tuple("stage_edges_p%d" % k for k in range(8)) + ("ragged", "ragged12")
MAIN_PATTERNS = ("uniform_up", "uniform_down", "near_uniform_l0", "near_uniform_l1", "near_uniform_l37",
                 "near_uniform_l63", "stage_edges", "ragged")


def _rotate(patterns, shift=0, extra=(), width=1):
    """Every pattern with `width` index patterns, taken in turn; `extra` crossed in
    full."""
    out = [(p, INDEX_PATTERNS[(k + shift + j) % 4]) for k, p in enumerate(patterns) for j in range(width)]
    for p in extra:
        out += [(p, ip) for ip in INDEX_PATTERNS if (p, ip) not in out]
    return out


def _t(name, entry, n, kernel, cases, policy="auto", env=None, fresh=False):
    return {"name": name, "entry": entry, "n": n, "kernel": kernel, "cases": list(cases), "policy": policy,
            "env": dict(env or {}), "fresh": fresh}


def n_split(r_of, rounds=1):
    return lambda c: rounds * 4 * c * 64 + r_of(4 * c) * 64 - 27


SPLIT_R = (("r1", lambda S: 1, 12), ("s5", lambda S: S // 5, 5), ("s3", lambda S: S // 3, 3),
           ("s2", lambda S: S // 2, 2))       # tag, r as a function of S = 4 CUs, its segment count


def targets():
    """Every target: its entry (device or host), n as a function of the CU count (a
    dict: per pattern), the kernel it claims ("dod", "split", "small", or "shards":
    per shard as plan_split says), its (count pattern, index pattern) cases, policy
    and environment. fresh: a context of its own per case (MSHA_VIRTUAL_SHARDS is
    read when a context is made)."""
    T = [
        _t("dod_device", "device", lambda c: N_UNSPLIT, "dod", _rotate(FULL_PATTERNS, extra=("ragged",), width=2)),
        _t("dod_device_coop_policy", "device", n_split(lambda S: 1), "dod",
           [("ragged", "random"), ("uniform_up", "contiguous")], policy="coop"),
    ]
    for k, (tag, r_of, _) in enumerate(SPLIT_R):
        T.append(_t("dod_split_" + tag, "device", n_split(r_of), "split", _rotate(MAIN_PATTERNS, shift=k, width=2)))
    T += [
        _t("dod_split_r1_x2", "device", n_split(lambda S: 1, rounds=2), "split",
           [("near_uniform_l0", "random"), ("stage_edges", "contiguous")]),
        _t("dod_host_small", "host", {"ragged": lambda c: N_SMALL, "limit": lambda c: N_SMALL, "two": lambda c: 2},
           "small", _rotate(("limit", "two"), extra=("ragged",))),
        # one index past the small path's limit, the environment untouched
        _t("dod_host_over_limit", "host", lambda c: N_SMALL, "dod", [("over_limit", "random")]),
        _t("dod_host_pipeline", "host", lambda c: N_UNSPLIT, "dod",
           [("ragged", "contiguous"), ("uniform_up", "random"), ("stage_edges_p3", "one_row")],
           env={"MSHA_SMALL_BYTES": "0"}),
        _t("dod_host_pipeline_split", "host", n_split(lambda S: S // 5), "split",
           [("ragged", "random"), ("near_uniform_l63", "contiguous")], env={"MSHA_SMALL_BYTES": "0"}),
        _t("dod_host_sharded", "host",
           {"ragged": lambda c: 64 * 30 - 27, "zero_runs": lambda c: 6600, "two": lambda c: 2}, "shards",
           [("ragged", "random"), ("ragged", "contiguous"), ("zero_runs", "random"), ("zero_runs", "contiguous"),
            ("two", "random")],
           env={"MSHA_SMALL_BYTES": "0", "MSHA_VIRTUAL_SHARDS": "3"}, fresh=True),
    ]
    return T


def target(name):
    return next(t for t in targets() if t["name"] == name)


def cases():
    """(target, count pattern, index pattern) of every case."""
    return [(t["name"], p, ip) for t in targets() for p, ip in t["cases"]]


def n_of(t, pattern, c):
    n = t["n"]
    return (n[pattern] if isinstance(n, dict) else n)(c)


def shards_of(t):
    return int(t["env"].get("MSHA_VIRTUAL_SHARDS", "1"))


def full_region(pattern, m, start=0):
    """The counts of m lanes that run DigestSrc::full under `pattern` (m a multiple
    of 64 in a split launch; else with a partial last wave of 37)."""
    if pattern in ("uniform_up", "uniform_down"):
        return uniform_waves(m, pattern == "uniform_down", 25 if pattern == "uniform_down" else 24)
    if pattern.startswith("near_uniform_l"):
        lane = int(pattern[len("near_uniform_l"):])
        return near_uniform(m, lane, start, {0: 23, 1: 26}.get(lane))   # the other two: a filler partial wave
    if pattern == "stage_edges":
        return stage_edges(m, None, start)
    if pattern.startswith("stage_edges_p"):
        return stage_edges(m, int(pattern[len("stage_edges_p"):]), start)
    if pattern == "ragged":
        return ragged(m, start)
    if pattern == "ragged12":
        return ragged(m, start + 12)    # its partial wave spans 666 <= 888: staged (ragged's 1,062: direct)
    raise KeyError(pattern)


def case_counts(t, pattern, c):
    """The digest counts of the case's n messages."""
    n = n_of(t, pattern, c)
    if pattern == "two":
        return np.array([5, 0], dtype=np.int64)     # three shards: the first stays empty
    if pattern == "zero_runs":
        cnt = zero_runs()
    elif pattern in ("limit", "over_limit"):
        cnt = ragged(n)
        cnt[-1] += SMALL_DOD_BYTES // 32 + (pattern == "over_limit") - int(cnt.sum())
    else:
        sp = plan_split(n, c, t["policy"]) if shards_of(t) == 1 else None
        if sp is None:
            cnt = full_region(pattern, n)
        else:
            cnt = np.concatenate([full_region(pattern, sp["n_main"]), segments(c, sp["chains"])])
    assert len(cnt) == n and cnt.min() >= 0
    return cnt


def to_begin(cnt):
    begin = np.zeros(len(cnt) + 1, dtype=np.uint64)
    begin[1:] = np.cumsum(cnt)
    return begin


def case_begin(t, pattern, c):
    return to_begin(case_counts(t, pattern, c))


def launches(t, pattern, c, begin=None):
    """The digest-of-digests launches of a case: [(lo, hi, split plan or None)], one
    per non-empty shard; none for a small call."""
    n = n_of(t, pattern, c)
    if t["entry"] == "host":
        begin = case_begin(t, pattern, c) if begin is None else begin
        if host_small(n, int(begin[-1]), int(t["env"].get("MSHA_SMALL_BYTES", SMALL_BYTES))):
            return []
        if shards_of(t) > 1:
            b = shard_bounds(_counts(begin, n), shards_of(t))
            return [(lo, hi, plan_split(hi - lo, c, t["policy"])) for lo, hi in zip(b[:-1], b[1:]) if hi > lo]
    return [(0, n, plan_split(n, c, t["policy"]))]


def expected_kernel(t, pattern, c):
    """What the restated rules give the case: "small", "dod", "split", or "shards"."""
    ls = launches(t, pattern, c)
    if not ls:
        return "small"
    if shards_of(t) > 1:
        return "shards"
    return "split" if ls[0][2] else "dod"


def expected_deltas(t, pattern, c):
    """The exact msha_stats deltas of the case's one call: every launch counter."""
    ls = launches(t, pattern, c)
    if not ls:
        return KM._only(launches_dod=0, small_calls=1, **small_launch(n_of(t, pattern, c), c))
    split = sum(1 for _, _, sp in ls if sp)
    return KM._only(launches_dod=len(ls) - split, launches_split=split, small_calls=0)


def case_cells(t, pattern, c):
    """(wave cells, edge cells, count cells, segment cells) of a case, over its
    launches (a shard's begin rebased, as the host entry does)."""
    begin = case_begin(t, pattern, c)
    waves, edges, counts, segs = set(), set(), set(), set()
    for lo, hi, sp in launches(t, pattern, c, begin):
        b = begin[lo:hi + 1] - begin[lo]
        m = hi - lo
        full = sp["n_main"] if sp else m
        waves |= set(wave_cells(b, full))
        edges |= edge_cells(b, full)
        counts |= count_cells(b, m)
        segs |= set(segment_cells(b, m, c, t["policy"]))
    return waves, edges, counts, segs


def table_bytes(t, pattern, c):
    """What a case hands the oracle: 32 bytes per index."""
    return 32 * int(case_counts(t, pattern, c).sum())


# ---------------------------------------------------------------------------
# Expected digests and the runner
# ---------------------------------------------------------------------------
def expected_hashlib(table, idx, begin):
    rows = table[idx].tobytes() if len(idx) else b""
    out = np.empty((len(begin) - 1, 32), dtype=np.uint8)
    for i in range(len(begin) - 1):
        d = hashlib.sha256(rows[32 * int(begin[i]):32 * int(begin[i + 1])]).digest()
        out[i] = np.frombuffer(d, dtype=np.uint8)
    return out


def expected(table, idx, begin):
    if len(begin) - 1 <= HASHLIB_MAX:
        return expected_hashlib(table, idx, begin)
    from oracle import oracle
    return oracle.digest_of_digests(table, idx, begin)


def mismatch(what, begin, got, exp, ls):
    """None when equal; else the case, how many digests differ, and for the first few
    their shard, wave, lane, count and how the lane read its indices (staged or direct
    in DigestSrc::full, or as a surplus chain's lane)."""
    bad = np.nonzero(np.any(got != exp, axis=1))[0]
    if bad.size == 0:
        return None
    first = []
    for i in bad[:6]:
        i = int(i)
        f = {"message": i, "count": int(begin[i + 1] - begin[i]), "path": "small call (batch kernel)"}
        for s, (lo, hi, sp) in enumerate(ls):
            if not lo <= i < hi:
                continue
            j = i - lo
            f.update(shard=s, wave=j // WAVE, lane=j % WAVE)
            if sp and j >= sp["n_main"]:
                f.update(path="chain lane", chain=(j - sp["n_main"]) // WAVE, segments=sp["segments"])
            else:
                w0 = j // WAVE * WAVE
                w1 = min(w0 + WAVE, sp["n_main"] if sp else hi - lo)
                f.update(path="staged" if is_staged(int(begin[lo + w1] - begin[lo + w0]), w1 - w0) else "direct",
                         wave_kind=KIND_NAMES[final_kind(_counts(begin[lo + w0:], w1 - w0))])
        first.append(f)
    return {"what": what, "bad": int(bad.size), "of": int(len(exp)), "first": first}


def _dev(a):
    import torch
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _deltas(st0, st1):
    return {k: st1[k] - st0[k] for k in COUNTERS}


def run_call(eng, entry, table, idx, begin):
    """One call -> (counter deltas, digests). The device API takes no null pointer:
    a batch without indices passes one unread entry."""
    st0 = eng.stats()
    if entry == "host":
        got = eng.digest_of_digests(table, idx, begin)
    else:
        import torch
        out = torch.full((len(begin) - 1, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
        eng.digest_of_digests_device(_dev(table), _dev(idx if len(idx) else np.zeros(1, np.uint32)), _dev(begin),
                                     out)
        eng.device_status()
        got = out.cpu().numpy()
    eng.device_status()
    return _deltas(st0, eng.stats()), got


def run_case(eng, name, pattern, index_pattern, cus):
    """One case: the environment is the caller's to set (target(name)["env"]); the
    policy is set here and restored. Asserts the kernel the target claims, the exact
    counter deltas and every digest. eng None (a target with fresh): a context of
    its own."""
    t = target(name)
    n = n_of(t, pattern, cus)
    what = "%s / %s / %s (n = %d)" % (name, pattern, index_pattern, n)
    assert expected_kernel(t, pattern, cus) == t["kernel"], \
        "%s: on %d CUs this n gives %s" % (what, cus, expected_kernel(t, pattern, cus))
    begin = case_begin(t, pattern, cus)
    table, idx = build_index(index_pattern, int(begin[-1]), KM._salt(name, pattern, index_pattern))
    exp = expected(table, idx, begin)
    own = None
    if eng is None:
        from mirbft_amd import Engine
        eng = own = Engine(1)
    try:
        eng.set_kernel_policy(t["policy"])
        d, got = run_call(eng, t["entry"], table, idx, begin)
    finally:
        if own:
            own.close()
        else:
            eng.set_kernel_policy("auto")
    KM.check_deltas(expected_deltas(t, pattern, cus), d, what)
    bad = mismatch(what, begin, got, exp, launches(t, pattern, cus, begin))
    assert bad is None, bad
