"""The cases and the model of the planned device call's PLAN
(msha_digest_batch_device_planned, mirbft_amd/csrc/plan.hip k_fold_*), shared by the CPU
check (tests/test_planned_matrix_cpu.py) and the GPU test
(tests/test_gpu_planned_matrix.py), which reads the plan back with
msha_planned_read_plan and holds it against check_plan().

Pure numpy and hashlib: nothing here calls the code under test. The model is written from
the contract in kernels.hpp ("Classes, ascending ...") and the "Candidates first" rule in
plan.hip:

  blocks(len)   SHA-256 blocks of a message, padding included
  klass(len)    the exact length below kFoldExactLen bytes; the exact block count up to
                4,095 blocks; floor(log2 blocks) above. Lanes come back by DESCENDING klass
                and that is the only order the contract gives: inside a class any passes.
  fresh[i]      off[i] strictly above every earlier offset (message 0 counts as above),
                and, when the call tried an early head (long_cap != 0), not long
                (< kLongBlocks blocks). A fresh message is a lane without a claim.
  lanes         the fresh messages plus exactly ONE claimant for each distinct (off, len)
                among the others. Which claimant wins is a race on the GPU and every
                choice passes. (A key first named by a fresh message and then by others is
                hashed twice: the fresh one never enters the table.)

The head's cost model (plan.hip head_cost) is NOT restated: cases force the head to 0 or
to at least 1 with the knobs, and place the early head an order of magnitude inside its
gate's inequality (early_margin()).

The direct planner's cases (k_plan_*, through msha_digest_batch on a pinned arena) have
no read-back: they are checked by digests and msha_stats only (direct_cases())."""
import hashlib
import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirbft_amd", "csrc")

NO_LANE = 0xFFFFFFFF            # kernels.hpp kNoLane
PREFILL = 0xA5                  # every digest buffer is prefilled with it
NOMINAL_CUS = 256               # what the CPU check builds the cases for
U = np.uint64


def _constant(name, header="kernels.hpp"):
    text = open(os.path.join(CSRC, header)).read()
    m = re.search(r"constexpr (?:uint32_t|uint64_t|unsigned) (?:\w+ = [^,;]+, )*%s = ([^,;]+)[,;]" % name, text)
    expr = m.group(1).strip()
    tokens = re.findall(r"[A-Za-z_]\w*|\d+|[*+\-()]", expr)
    assert "".join(tokens) == expr.replace(" ", ""), expr
    return int(eval("".join(str(_constant(t, header)) if re.match(r"[A-Za-z_]", t) else t for t in tokens)))


kPlanItems = _constant("kPlanItems")
kPlanTile = _constant("kPlanTile")
kFoldExactLen = _constant("kFoldExactLen")
kFoldLowBlocks = _constant("kFoldLowBlocks")
kFoldBigBuckets = _constant("kFoldBigBuckets")
kGridGroups = _constant("kGridGroups")
kCoopMsgsPerWg = _constant("kCoopMsgsPerWg")
kChain2MsgsPerWg = _constant("kChain2MsgsPerWg")
kChain8MsgsPerWg = _constant("kChain8MsgsPerWg")
kLongBlocks = _constant("kLongBlocks", "host_plan.hpp")
T = kPlanTile
EXACT_BLOCKS = 4096             # block counts below it have a class each (kernels.hpp)
# the planner's cycle figures a call passes to the early head's gate (kernels.hpp FoldArgs
# wave_block_cycles; device_batch.cpp early_cycles on the eight-lane kernel)
WAVE_BLOCK_CYCLES, EARLY_CYCLES = 6500, 3250


# --------------------------------------------------------------------------- the model

def blocks(ln):
    ln = np.asarray(ln, dtype=U)
    return (ln >> U(6)) + np.where((ln & U(63)) < U(56), U(1), U(2))


def _floor_log2(b):
    """Exact on uint64 (no floating point): b >= 1."""
    b = np.asarray(b, dtype=U)
    lg = np.zeros(b.shape, dtype=np.int64)
    for s in range(1, 64):
        lg += (b >> U(s)) != 0
    return lg


def klass(ln):
    """Ascending class of a message; monotone in len."""
    ln = np.asarray(ln, dtype=U)
    b = blocks(ln).astype(np.int64)
    exact_len = ln.astype(np.int64)
    exact_blk = kFoldExactLen + (b - kFoldLowBlocks)
    big = kFoldExactLen + (EXACT_BLOCKS - kFoldLowBlocks) + _floor_log2(b) - 12
    return np.where(ln < U(kFoldExactLen), exact_len, np.where(b < EXACT_BLOCKS, exact_blk, big))


def fresh(off, ln, early_on):
    off = np.asarray(off, dtype=U).astype(np.int64)    # arena offsets are far below 2^63
    f = off > np.r_[np.int64(-1), np.maximum.accumulate(off)[:-1]]
    if early_on:
        f &= blocks(ln) < U(kLongBlocks)
    return f


def keys(off, ln):
    """One integer per (off, len), equal exactly when both are."""
    off, ln = np.asarray(off, dtype=U), np.asarray(ln, dtype=U)
    if off.size == 0 or (int(off.max()) < (1 << 40) and int(ln.max()) < (1 << 24)):
        return (off << U(24)) | ln
    _, inv = np.unique(np.stack([off, ln], axis=1), axis=0, return_inverse=True)
    return inv.reshape(-1).astype(U)


def model_lanes(off, ln, early_on=True):
    """The folded planner's lane count: fresh messages + distinct keys among the rest."""
    f = fresh(off, ln, early_on)
    return int(f.sum()) + int(np.unique(keys(off, ln)[~f]).size)


def reference_fold(off, ln, early_on):
    """The same count by a dict-based O(n) walk (tests check it against model_lanes)."""
    top, lanes, seen = -1, 0, set()
    b = blocks(ln)
    for i in range(len(off)):
        o = int(off[i])
        if o > top and not (early_on and int(b[i]) >= kLongBlocks):
            lanes += 1
        elif (o, int(ln[i])) not in seen:
            seen.add((o, int(ln[i])))
            lanes += 1
        top = max(top, o)
    return lanes


def digests(arena, off, ln):
    """uint8[n, 32]: each distinct (off, len) hashed once with hashlib."""
    k = keys(off, ln)
    _, first, inv = np.unique(k, return_index=True, return_inverse=True)
    mv = memoryview(arena)
    d = np.empty((first.size, 32), np.uint8)
    for j, i in enumerate(first):
        o = int(off[i])
        d[j] = np.frombuffer(hashlib.sha256(mv[o:o + int(ln[i])]).digest(), np.uint8)
    return d[inv.reshape(-1)]


def early_margin(n_short_blocks, long_blocks_each, n_long, simds):
    """How far inside the early head's inequality a batch is (plan.hip k_fold_longs_gate and
    k_fold_longs: blocks x wave_block_cycles / (64 simds) < longest chain x early_cycles):
    the head's side over the body's, with every distinct long payload on the body's."""
    t_body = (n_short_blocks + n_long * long_blocks_each) * WAVE_BLOCK_CYCLES // (64 * simds)
    return long_blocks_each * EARLY_CYCLES / max(t_body, 1)


# --------------------------------------------------------------------------- the check

def check_plan(off, ln, fold, plan, order, longs, expect=None):
    """The problems of a plan read back after a call on (off, len), in words ([]: none).
    plan: Engine.planned_read_plan()'s dict; order: its n positions; longs: the early
    head's list. expect: a case's forced figures (head / head_min / early / gate)."""
    bad = []
    n = len(off)
    order = np.asarray(order, dtype=np.uint32)
    longs = np.asarray(longs, dtype=np.uint32)
    if plan["n"] != n or order.size != n:
        return ["the plan is of %d messages (order %d), the call had %d" % (plan["n"], order.size, n)]
    if bool(plan["folded"]) != bool(fold):
        bad.append("folded = %d on a call with fold = %s" % (plan["folded"], fold))
    lanes = int(plan["lanes"])
    early_on = plan["long_cap"] != 0
    f = fresh(off, ln, early_on) if fold else np.ones(n, bool)
    k = keys(off, ln)
    want = int(f.sum()) + int(np.unique(k[~f]).size)
    if lanes != want:
        bad.append("lanes = %d, the model has %d" % (lanes, want))
    if lanes > n:
        return bad + ["lanes past n"]
    L = order[:lanes].astype(np.int64)
    if (order[:lanes] == NO_LANE).any():
        bad.append("kNoLane inside the lanes at position %d" % int(np.argmax(order[:lanes] == NO_LANE)))
    elif (L >= n).any():
        bad.append("a lane names message %d of %d" % (int(L.max()), n))
    else:
        if np.unique(L).size != lanes:
            bad.append("a message is listed twice: %d positions, %d distinct" % (lanes, np.unique(L).size))
        lf = f[L]
        if int(lf.sum()) != int(f.sum()) or np.unique(L[lf]).size != int(f.sum()):
            bad.append("%d of the %d fresh messages are lanes" % (np.unique(L[lf]).size, int(f.sum())))
        ck = k[L[~lf]]
        if np.unique(ck).size != ck.size:
            bad.append("a candidate key has two claimants")
        if not np.array_equal(np.unique(ck), np.unique(k[~f])):
            bad.append("the claimants' keys are not the candidates' distinct keys")
        c = klass(np.asarray(ln, dtype=U)[L])
        if (np.diff(c) > 0).any():
            p = int(np.argmax(np.diff(c) > 0))
            bad.append("class rises at position %d: %d then %d" % (p + 1, int(c[p]), int(c[p + 1])))
        b = blocks(np.asarray(ln, dtype=U)[L])
        if plan["early"]:
            e = int(plan["early"])
            if not (e == plan["long_lanes"] == plan["long_listed"] <= plan["long_cap"]):
                bad.append("early %d, long_lanes %d, long_listed %d, long_cap %d" %
                           (e, plan["long_lanes"], plan["long_listed"], plan["long_cap"]))
            elif e > lanes or longs.size < e:
                bad.append("early %d with %d lanes and %d listed" % (e, lanes, longs.size))
            else:
                head, listed = set(L[:e].tolist()), set(longs[:e].tolist())
                is_long = set(L[b >= U(kLongBlocks)].tolist())
                if head != listed:
                    bad.append("the first %d positions are not the early head's list (%d differ)" %
                               (e, len(head ^ listed)))
                if head != is_long:
                    bad.append("the early head is not exactly the long lanes (%d differ)" % len(head ^ is_long))
    if (order[lanes:] != NO_LANE).any():
        bad.append("position %d past the lanes is not kNoLane" % (lanes + int(np.argmax(order[lanes:] != NO_LANE))))
    if not fold and lanes != n:
        bad.append("unfolded: %d lanes of %d messages" % (lanes, n))
    if plan["head"] != (plan["early"] or plan["late"]):
        bad.append("head %d, early %d, late %d" % (plan["head"], plan["early"], plan["late"]))
    if plan["head"] > min(lanes, plan["head_cap"]):
        bad.append("head %d above min(lanes %d, head_cap %d)" % (plan["head"], lanes, plan["head_cap"]))
    if not plan["early"]:
        late = int(plan["late"])
        if late and not (late % max(int(plan["head_per_wg"]), 1) == 0 or late in (lanes, plan["head_cap"])):
            bad.append("late head %d is no multiple of %d, nor the lanes, nor head_cap" %
                       (late, plan["head_per_wg"]))
    if plan["gave_up"]:
        bad.append("%d look-backs gave up" % plan["gave_up"])
    for name, v in (expect or {}).items():
        if name == "head_min":
            if plan["head"] < v:
                bad.append("head %d, forced to at least %d" % (plan["head"], v))
        elif name == "early_on":
            if early_on != v:
                bad.append("long_cap %d, early head tried: expected %s" % (plan["long_cap"], v))
        elif plan[name] != v:
            bad.append("%s = %d, expected %d" % (name, plan[name], v))
    return bad


# --------------------------------------------------------------------------- the cases

@dataclass
class Batch:
    off: object
    len: object
    arena_bytes: int
    seed: int

    @property
    def n(self):
        return int(self.off.size)

    def arena(self):
        """The payload bytes (+ the device entry's 64 bytes of slack), from the seed."""
        return np.random.default_rng(self.seed).integers(0, 256, self.arena_bytes + 64, dtype=np.uint8)


@dataclass
class Case:
    name: str
    make: object                                    # () -> Batch
    fold: bool
    policy: str = "lane"                            # "lane" / "auto"
    env: dict = field(default_factory=dict)
    unaligned: tuple = (False, False)               # d_off, d_len 8 bytes off a 16-byte boundary
    expect: dict = field(default_factory=dict)      # check_plan(expect=)
    edge: dict = field(default_factory=dict)        # what the CPU check asserts of the batch
    doc: str = ""


def _packed(ln):
    ln = np.asarray(ln, dtype=U)
    step = np.maximum((ln + U(15)) // U(16) * U(16), U(16))    # (an empty message takes a start of its own)
    off = np.zeros(ln.size, U)
    off[1:] = np.cumsum(step)[:-1]
    return off


def _small_lens(rng, n):
    return rng.integers(0, 65, n).astype(U)


def _batch(off, ln, seed):
    off, ln = np.ascontiguousarray(off, dtype=U), np.ascontiguousarray(ln, dtype=U)
    assert off.size == ln.size and not (off % U(16)).any()
    return Batch(off, ln, int((off + ln).max()) if off.size else 0, seed)


def p_rising(n, seed):
    """Packed rising offsets: every message is fresh."""
    ln = _small_lens(np.random.default_rng(seed), n)
    return _batch(_packed(ln), ln, seed)


def p_one(n, seed):
    """One 40-byte payload n times: folded, message 0 is fresh and never enters the table,
    one of the others claims the key, and the kNoLane tail is the other n - 2."""
    return _batch(np.zeros(n, U), np.full(n, 40, U), seed)


def p_falling(n, seed):
    """Offsets strictly falling: everything after message 0 is a candidate, every key is
    distinct; a full tile lists all 4,096 and its claim loop runs 16 rounds."""
    ln = _small_lens(np.random.default_rng(seed), n)
    return _batch(U(64) * np.arange(n - 1, -1, -1, dtype=U), ln, seed)


def p_backrefs(n, seed):
    """Rising, but the first 8 messages of every tile after the first name payloads 100,
    200 .. 800 of the tile before: above everything earlier in their OWN tile, so fresh
    after the insert's first pass and demoted by its second; and every 64th message names
    message 20 of its run of 256 (first-pass candidates, four to a key: three fold)."""
    ln = _small_lens(np.random.default_rng(seed), n)
    off = _packed(ln)
    src_off, src_len = off.copy(), ln.copy()
    i = np.arange(n)
    mid = (i % 64 == 63)
    off[mid], ln[mid] = src_off[i[mid] // 256 * 256 + 20], src_len[i[mid] // 256 * 256 + 20]
    for t0 in range(T, n, T):
        for j in range(min(8, n - t0)):
            off[t0 + j], ln[t0 + j] = src_off[t0 - T + 100 * (j + 1)], src_len[t0 - T + 100 * (j + 1)]
    return _batch(off, ln, seed)


def p_never(n, seed):
    """Equal offset with different lengths, equal length with different offsets: message i
    is (64 (i // 65), i % 65). Offsets do not rise strictly, so 64 of every 65 probe the
    table, and no two keys are equal: nothing folds."""
    i = np.arange(n, dtype=U)
    return _batch(U(64) * (i // U(65)), i % U(65), seed)


def p_zero(n, seed):
    """Zero lengths at five offsets, cycling."""
    return _batch(U(16) * (np.arange(n, dtype=U) % U(5)), np.zeros(n, U), seed)


def p_straddle(n, seed):
    """Duplicates that straddle every tile edge e: messages e - 1 and e both name message
    e - 3's payload (two candidates of one key in two tiles: one claims, one folds), and
    e + 1 names e - 2's (hashed again: a fresh message never enters the table)."""
    ln = _small_lens(np.random.default_rng(seed), n)
    off = _packed(ln)
    src_off, src_len = off.copy(), ln.copy()
    for e in range(T, n, T):
        for dst, src in ((e - 1, e - 3), (e, e - 3), (e + 1, e - 2)):
            if dst < n:
                off[dst], ln[dst] = src_off[src], src_len[src]
    return _batch(off, ln, seed)


def p_mixed(n, seed):
    """Rising, every 5th message naming message i // 20, four to a key (the unaligned cases:
    folds at 17 messages too, and across the tile edge at T + 1)."""
    ln = _small_lens(np.random.default_rng(seed), n)
    off = _packed(ln)
    src_off, src_len = off.copy(), ln.copy()
    i = np.arange(4, n, 5)
    off[i], ln[i] = src_off[i // 20], src_len[i // 20]
    return _batch(off, ln, seed)


PATTERNS = [("rising", p_rising), ("one_payload", p_one), ("falling", p_falling), ("backrefs", p_backrefs),
            ("never_fold", p_never), ("zero_len", p_zero), ("straddle", p_straddle)]


def _with_longs(base, windows, names, long_len, seed):
    """base's short messages plus `windows` long payloads of long_len bytes, each a window
    into one buffer (16 bytes apart) BELOW the short payloads, so that naming one never
    raises the largest offset so far, and each named `names` times, spread evenly over the
    batch from message 1 on (replacing short messages)."""
    n = base.off.size
    room = U((16 * windows + long_len + 15) // 16 * 16)
    off, ln = base.off + room, base.len.copy()
    at = np.linspace(1, n - 1, windows * names).astype(np.int64)
    assert np.unique(at).size == at.size
    for j, p in enumerate(at):
        off[p], ln[p] = 16 * (j % windows), long_len
    return _batch(off, ln, seed)


LONG_LEN = (kLongBlocks - 1) * 64        # exactly kLongBlocks blocks: 255 whole ones and the padding's
BIG_LEN = 4094 * 64 + 56                 # exactly 4,096 blocks


def sizes_lane():
    return [1, 15, 16, 17, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1, 16 * T, 17 * T - 1, 33 * T + 5]


def sizes_auto(cus):
    """all-cooperative | head + lanes | the gate's 64-workgroup grid (more tiles than CUs,
    44 past a multiple of 64) | a look-back's second 64-tile step and a grid of tiles that
    is no multiple of kGridGroups (130 tiles; more when that is no more than C * 128)."""
    coop = cus * kCoopMsgsPerWg
    many = (max(cus, 64) + 63) // 64 * 64 + 44
    steps = max(130, coop // T + 2)
    if steps % kGridGroups == 0:
        steps += 2
    return [coop, coop + 1, many * T, steps * T - 7]


def probe_case(cus):
    """A folded `auto` call just above the cooperative range: its read-back tells long_cap."""
    n = cus * kCoopMsgsPerWg + 1
    return Case("probe", lambda: p_rising(n, 1), True, "auto")


def cases(cus=NOMINAL_CUS, long_cap=None):
    """Every single-call case. cus: the device's CU count; long_cap: the early head's list
    size as a read-back of probe_case() gave it (None: the nominal cus * 16 / 8)."""
    if long_cap is None:
        long_cap = cus * kChain8MsgsPerWg // 8
    simds = 4 * cus
    out = []
    seed = 100
    # sizes x patterns, under policy lane (the lane kernels; folded: work stealing, no head)
    for n in sizes_lane():
        for pname, pat in PATTERNS:
            for fold in (True, False):
                seed += 1
                out.append(Case("lane-%s-%d-%s" % (pname, n, "fold" if fold else "plain"),
                                (lambda pat=pat, n=n, s=seed: pat(n, s)), fold, "lane",
                                expect={"head": 0, "early_on": False}, edge={"pattern": pname, "n": n}))
    # sizes x patterns under auto
    coop = cus * kCoopMsgsPerWg
    for n in sizes_auto(cus):
        for pname, pat in PATTERNS:
            for fold in (True, False):
                seed += 1
                exp = {"head": 0, "early_on": False} if n <= coop else {"early_on": fold, "early": 0}
                out.append(Case("auto-%s-%d-%s" % (pname, n, "fold" if fold else "plain"),
                                (lambda pat=pat, n=n, s=seed: pat(n, s)), fold, "auto", expect=exp,
                                edge={"pattern": pname, "n": n, "auto": True}))
        if n > coop:
            # two payloads of 4,096 blocks, each named twice, among the short ones: the gate
            # and the list both reduce over this grid and the early head must fire
            seed += 1
            m = early_margin(2 * n, 4096, 2, simds)         # (a short message: at most 2 blocks)
            out.append(Case("auto-early-%d" % n,
                            (lambda n=n, s=seed: _with_longs(p_rising(n, s), 2, 2, BIG_LEN, s)), True, "auto",
                            expect={"early": 2, "gate": 1, "early_on": True},
                            edge={"n": n, "auto": True, "margin": m},
                            doc="early head %.0fx inside its inequality" % m))
    big = coop + 1
    # unaligned d_off / d_len: each alone, then both, at T + 1 and 17 (the GPU test holds
    # the plan against the aligned run's as well)
    for n in (T + 1, 17):
        for fold in (True, False):
            for ua in ((True, False), (False, True), (True, True)):
                seed += 1
                out.append(Case("unaligned-%d-%s-off%d-len%d" % (n, "fold" if fold else "plain", ua[0], ua[1]),
                                (lambda n=n: p_mixed(n, 77)), fold, "lane",
                                unaligned=ua, expect={"head": 0}, edge={"n": n}))
    seed += 1
    out.append(Case("unaligned-early-%d" % big, (lambda s=seed: _with_longs(p_rising(big, s), 1, 2, LONG_LEN, s)),
                    True, "auto", unaligned=(True, True), expect={"early": 1, "gate": 1},
                    edge={"n": big, "auto": True, "margin": early_margin(2 * big, kLongBlocks, 1, simds)}))
    # class edges, n = C * 128 + 1, folded and not, the head on either kernel
    for fold in (True, False):
        for chain2 in ("0", "2"):
            out.append(Case("class-edges-%s-chain2=%s" % ("fold" if fold else "plain", chain2),
                            (lambda: class_edges(big, 900)), fold, "auto", env={"MSHA_HEAD_CHAIN2": chain2},
                            expect={"early_on": fold and chain2 == "2"}, edge={"n": big, "class_edges": True}))
    # the early head's list around its capacity: the last must stand down
    for L in sorted({1, long_cap - 1, long_cap, long_cap + 1}):
        if L < 1:
            continue
        seed += 1
        m = early_margin(2 * big, kLongBlocks, L, simds)
        out.append(Case("early-list-%s" % {1: "1", long_cap - 1: "cap-1", long_cap: "cap", long_cap + 1: "cap+1"}[L],
                        (lambda L=L, s=seed: _with_longs(p_rising(big, s), L, 2, LONG_LEN, s)), True, "auto",
                        expect={"early": L if L <= long_cap else 0, "gate": 1, "long_listed": L, "long_cap": long_cap},
                        edge={"n": big, "auto": True, "margin": m, "longs": L},
                        doc="%d distinct payloads of kLongBlocks blocks, each named twice; %.0fx inside the "
                            "early head's inequality" % (L, m)))
    # the head forced to 0 and to at least 1
    one_chain = lambda: _with_longs(p_rising(big, 555), 1, 1, BIG_LEN, 555)   # noqa: E731
    for fold in (True, False):
        f = "fold" if fold else "plain"
        out.append(Case("head-off-%s" % f, one_chain, fold, "auto", env={"MSHA_PLAN_HEAD": "0"},
                        expect={"head": 0, "early_on": False, "head_cap": 0}))
        out.append(Case("head-pct-100000-%s" % f, one_chain, fold, "auto",
                        env={"MSHA_PLAN_HEAD_PCT": "100000", "MSHA_EARLY_HEAD": "0"},
                        expect={"head": 0, "early_on": False}))
    out.append(Case("head-pct-1-plain", one_chain, False, "auto", env={"MSHA_PLAN_HEAD_PCT": "1"},
                    expect={"head_min": 1}, doc="one 4,096-block chain above %d one-block messages" % big))
    return out


def class_edges(n, seed):
    """Mostly 32-byte messages; a few at 1023 | 1024 bytes and on each side of the 16 | 17
    block edge, 4,095 | 4,096 blocks, 2^13 - 1 | 2^13 blocks and kLongBlocks - 1 |
    kLongBlocks blocks. The big ones are overlapping windows of one 600 KiB buffer, and
    each is named three times."""
    ln = np.full(n, 32, U)
    off = _packed(ln)
    buf = (int(off[-1]) + 32 + 15) // 16 * 16
    edge_lens = [1015, 1016, 1023, 1024, 1079, 1080,
                 4094 * 64 + 55, 4094 * 64 + 56, 8190 * 64 + 55, 8190 * 64 + 56,
                 (kLongBlocks - 2) * 64 + 55, (kLongBlocks - 2) * 64 + 56]
    assert [int(x) for x in blocks(edge_lens)] == [16, 17, 17, 17, 17, 18, 4095, 4096, 8191, 8192,
                                                   kLongBlocks - 1, kLongBlocks]
    at = np.linspace(3, n - 3, 2 * 3 * len(edge_lens)).astype(np.int64)
    assert np.unique(at).size == at.size
    rng = np.random.default_rng(seed)
    rng.shuffle(at)
    j = 0
    for e, el in enumerate(edge_lens):
        for w in range(2):                      # two windows of each length
            o = buf + 16 * (2 * e + w)
            assert o + el <= buf + 600 * 1024
            for _ in range(3):                  # each named three times
                off[at[j]], ln[at[j]] = o, el
                j += 1
    b = _batch(off, ln, seed)
    b.arena_bytes = buf + 600 * 1024
    return b


@dataclass
class Step:
    make: object
    fold: bool
    stream: int = 0            # 0: the context's own; 1, 2: streams of the test's
    wait: bool = True          # read the plan back (a host wait) after the call


def sequence():
    """Calls on ONE context: folded at 17 T with heavy aliasing; folded at 300 with the same
    offsets (the alias table's slots of the larger call's epoch must read as empty, and the
    order's words past n are stale); unfolded at T + 1; folded at 17 T again on another
    stream with no host wait after the third."""
    def heavy(n, seed):
        rng = np.random.default_rng(seed)
        ln = _small_lens(rng, n)
        off = _packed(ln)
        src = rng.integers(0, 256, n)                   # a pool of 256 payloads named over and over
        al = (rng.random(n) < 0.6) & (src < np.arange(n))
        off[al], ln[al] = off[src[al]], ln[src[al]]
        return _batch(off, ln, seed)

    def head300():
        b = heavy(17 * T, 31)
        return _batch(b.off[:300], b.len[:300], 31)
    return [Step(lambda: heavy(17 * T, 31), True), Step(head300, True),
            Step(lambda: p_straddle(T + 1, 32), False, stream=1, wait=False),
            Step(lambda: heavy(17 * T, 33), True, stream=2)]


# --------------------------------------------------------------------------- the direct planner

DIRECT_ENV = {"MSHA_SMALL_BYTES": "0", "MSHA_DIRECT_PIECE_SHIFT": "16"}
DIRECT_PIECE = 1 << 16
DIRECT_BUCKETS = 1 << 20           # host_direct.cpp: more (group, block count) buckets: groups only


def _direct_base(seed):
    ln = np.random.default_rng(seed).integers(0, 4096, 3 * T).astype(U)
    return _packed(ln), ln


def direct_a():
    """3 T messages, lengths uniform in [0, 4096), packed: > 1,024 keys in a tile."""
    off, ln = _direct_base(41)
    return _batch(off, ln, 41)


def direct_b():
    """(a) with 10 % aliases into earlier messages: the alias table path."""
    off, ln = _direct_base(42)
    rng = np.random.default_rng(4242)
    n = off.size
    src = rng.integers(0, n, n)
    al = (rng.random(n) < 0.1) & (src < np.arange(n))
    off[al], ln[al] = off[src[al]], ln[src[al]]
    return _batch(off, ln, 42)


def direct_c():
    """(a) plus one 1 MiB message: groups x (bmax + 1) > 2^20, so B == 1."""
    off, ln = _direct_base(43)
    ln = np.r_[ln, U(1 << 20)]
    return _batch(_packed(ln), ln, 43)


def direct_d():
    """(a) plus 5 messages of kLongBlocks blocks: a long region."""
    _, ln = _direct_base(44)
    ln[np.linspace(10, ln.size - 10, 5).astype(int)] = LONG_LEN
    return _batch(_packed(ln), ln, 44)


def direct_cases():
    """(name, make, shards): digests and stats only -- the direct planner has no read-back."""
    return [("%s-shards%d" % (f.__name__, s), f, s) for f in (direct_a, direct_b, direct_c, direct_d) for s in (1, 3)]


def direct_shape(b):
    """What the host gives the direct planner for b on one shard, from the case's own
    numbers: (pieces, groups, bmax, B) -- a packed batch touches every 64 KiB granule up to
    its end, so the device arena is its span rounded up to a piece."""
    bl = blocks(b.len)
    bmax = int(bl.max())
    pieces = max(1, (b.arena_bytes + DIRECT_PIECE - 1) // DIRECT_PIECE)
    groups = 2 * pieces if bmax >= kLongBlocks else pieces
    B = bmax + 1 if groups * (bmax + 1) <= DIRECT_BUCKETS else 1
    return pieces, groups, bmax, B


def direct_keys(b):
    """The bucket key of every message of b as a lane (plan.hip lane_key) on one shard:
    (region, piece of the payload's end) * B + bmax - blocks."""
    pieces, groups, bmax, B = direct_shape(b)
    bl = blocks(b.len).astype(np.int64)
    end = (b.off + np.maximum(b.len, U(1)) - U(1)).astype(np.int64)
    piece = np.minimum(end // DIRECT_PIECE, pieces - 1)
    region = np.where((groups > pieces) & (bl < kLongBlocks), 1, 0)
    return (region * (groups - pieces) + piece) * B + (bmax - bl if B > 1 else 0)
