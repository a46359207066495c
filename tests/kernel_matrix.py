"""Per-kernel length matrix: case generator and runner (not collected by pytest).

Every hash kernel of mirbft_amd/csrc/kernels.hip has its own block loop, tail
handling and end-of-message fast paths. This module builds batches from LENGTH
PATTERNS (whole waves of one length, waves uniform but for one lane, ragged
waves, block counts around the chain kernels' pairing threshold) and aims them at
KERNEL TARGETS: an entry point, a batch size as a function of the CU count, the
policy and environment that route the call to one kernel, and the msha_stats
launch counters that prove that kernel ran. tests/test_kernel_matrix_cpu.py checks
from the lengths alone that the patterns hit every cell they promise and that every
n stays inside its kernel's range; tests/test_gpu_kernel_matrix.py runs the cases,
bit-exact against the oracle's scalar FIPS 180-4 leg.

`python tests/kernel_matrix.py --child` runs, in a process of its own, the cases
that depend on MSHA_LOAD_MODE (read once per process by the library), one JSON line
per case.

No GPU code here; torch is imported only when a case runs.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WAVE = 64
# Every r = len % 64 with nfull = len // 64 from 0 to 5: all four exits of the
# pipelined loop's 4-step rotation, its nfull == 0 path, both kPair parities.
LENS = np.arange(0, 384, dtype=np.uint64)
PARTIAL_LANES = 37          # every lane-kernel n is 64 k - 27: the last wave holds 37 messages

NEAR_BASE = (0, 56, 63, 64, 120, 128, 192)
NEAR_LANES = (0, 1, 37, 63)  # lane 0: readfirstlane returns the odd length

PLANNED_UNIFORM = (0, 63, 128, 191, 256, 319)   # block counts 1..6, every length on the uniform-pad path
PLANNED_R0 = (0, 64, 128, 192, 256)             # the r == 0 spellings

UNIFORM_LENS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 183, 192)
# (msg_len, stride) launches of the uniform layout, in groups of about equal bytes;
# the last one has a stride larger than needed (its gaps hold random bytes)
UNIFORM_GROUPS = {
    "le56": [(0, 16), (1, 16), (55, 64), (56, 64)],
    "le65": [(63, 64), (64, 64), (65, 80)],
    "le128": [(119, 128), (120, 128), (127, 128), (128, 128)],
    "le192": [(183, 192), (192, 192), (120, 256)],
}

PAIR_NB = (1, 62, 63, 64, 65, 66, 127, 128, 129)
COUNTERS = ("launches_lane", "launches_lane_ws", "launches_pipe", "launches_coop", "launches_split",
            "launches_chain2", "launches_chain8")
KIND_NAMES = ("ragged", "uniform", "near-uniform (lane 0 odd)", "near-uniform (another lane odd)")
RAGGED, UNIFORM, NEAR0, NEAR_OTHER = range(4)


# ---------------------------------------------------------------------------
# The launchers' thresholds, restated (mirbft_amd/csrc/kernels.hip; the constants
# kCoopMsgsPerWg / kChain2MsgsPerWg / kChain8MsgsPerWg are kernels.hpp's).
# ---------------------------------------------------------------------------
COOP_PER_WG, CHAIN2_PER_WG, CHAIN8_PER_WG = 128, 64, 16


def pick_mode(n, cus, forced=-1):
    """kernels.hip pick_mode(): 0 kSingle, 1 kPrefetch, 2 kPair, 3 kPipe."""
    if 0 <= forced <= 3:
        return forced
    if n <= cus * 4 * 64:
        return 3
    return 1 if n < cus * 4 * 64 * 3 else 2


def uses_coop(n, cus, policy):
    """kernels.hip uses_coop()."""
    if policy == "coop":
        return True
    if policy == "lane":
        return False
    return n <= cus * COOP_PER_WG


def plan_split(n, cus, policy):
    """kernels.hip plan_split(): (n_main, chains) or None."""
    if policy == "coop":
        return None
    simds = cus * 4
    waves = (n + 63) // 64
    q, r = divmod(waves, simds)
    if q < 1 or r == 0 or r > simds // 2:
        return None
    return q * simds * 64, r


def split_mode(n_main, cus, forced=-1):
    """kernels.hip split_mode(): the main workgroups' load mode (never kPipe)."""
    if 0 <= forced <= 2:
        return forced
    return 1 if n_main < cus * 4 * 64 * 3 else 2


def batch_kernel(n, cus, policy="auto", small8=True, forced=-1):
    """(kernel, load mode) of msha_digest_batch_device: split_for() first, then
    launch_digest_batch()'s order of tests (kernels.hip)."""
    sp = plan_split(n, cus, policy)
    if sp:
        return "split", split_mode(sp[0], cus, forced)
    if uses_coop(n, cus, policy):
        if policy == "auto" and n <= cus * CHAIN8_PER_WG and small8:
            return "chain8", 1
        if policy == "auto" and n <= cus * CHAIN2_PER_WG:
            return "chain2", 1
        return "coop", 1
    mode = pick_mode(n, cus, forced)
    return ("pipe", 3) if mode == 3 else ("lane", mode)


def planned_kernel(n, cus, policy, ws):
    """The body launch of msha_digest_batch_device_planned (gated: neither the
    cooperative kernel nor a split), read_plan_knobs()' k.ws."""
    if uses_coop(n, cus, policy):
        return "coop", 1
    mode = pick_mode(n, cus)
    if mode == 3:
        return "pipe", 3
    return ("lane_ws" if ws else "lane"), mode


def uniform_kernel(n, cus, forced=-1):
    """launch_digest_uniform()."""
    mode = pick_mode(n, cus, forced)
    return ("pipe", 3) if mode == 3 else ("lane", mode)


# ---------------------------------------------------------------------------
# Length patterns
# ---------------------------------------------------------------------------
def blocks(lens):
    lens = np.asarray(lens, dtype=np.uint64)
    return (lens >> np.uint64(6)).astype(np.int64) + np.where((lens & np.uint64(63)) < 56, 1, 2)


def ragged(n, start=0):
    """Message i has length LENS[(i * 7919) % 384]: 7919 % 384 = 239 is coprime to
    384, so the 64 lanes of a wave all differ."""
    i = np.arange(start, start + n, dtype=np.int64)
    return LENS[(i * 7919) % 384].copy()


def uniform_waves(n, partial_len):
    """Wave k is entirely of one LENS entry; the partial last wave of partial_len.
    The variant with a partial wave of 64 walks LENS upward (wave k: LENS[k % 384]),
    the one with 56 downward (LENS[383 - k % 384]), so that a launch of fewer than
    384 waves still sees all of LENS between the two."""
    assert n % WAVE == PARTIAL_LANES and partial_len in (64, 56)
    k = np.arange(n, dtype=np.int64) // WAVE
    idx = k % 384 if partial_len == 64 else 383 - k % 384
    lens = LENS[idx].copy()
    lens[n - PARTIAL_LANES:] = partial_len
    return lens


def near_odd_lengths(L):
    """The odd lane's lengths for base length L: a block more, the neighbour across
    the 55|56 or the 63|64 edge, and empty."""
    c = {L + 64, 0}
    if L > 0 and L % 64 in (0, 56):
        c.add(L - 1)
    if L % 64 in (55, 63):
        c.add(L + 1)
    c.discard(L)
    return sorted(c)


def near_combos():
    return [(L, j, o) for L in NEAR_BASE for j in NEAR_LANES for o in near_odd_lengths(L)]


def near_uniform(n):
    """One wave per (L, j, L'): 64 messages of L with lane j of L'; then ragged
    waves up to n (the last one partial). A launch too small for every combination
    (a device with few CUs) holds the first ones that fit before its partial wave."""
    lens = ragged(n)
    full = n // WAVE
    for w, (L, j, o) in enumerate(near_combos()[:full]):
        lens[w * WAVE:(w + 1) * WAVE] = L
        lens[w * WAVE + j] = o
    return lens


def planned_classes(n, lengths):
    """Message i has length lengths[i % k]: thousands of messages at each length,
    interleaved, so the planner's sort (by exact length below 1,024 B) has work to
    do and gives each length whole waves, with mixed waves at the class boundaries."""
    return np.asarray(lengths, dtype=np.uint64)[np.arange(n) % len(lengths)].copy()


def pair_spellings():
    """(nb, length-only last block, lengths): nb = 1, and for each nb >= 62 a tail
    with r < 56 and one with r >= 56, whose last block holds the length alone. Each
    spelling has several r, all of the same block count."""
    out = []
    for nb in PAIR_NB:
        if nb == 1:
            out.append((1, False, (0, 1, 37, 55)))
            continue
        out.append((nb, False, tuple((nb - 1) * 64 + r for r in (0, 1, 17, 55))))
        out.append((nb, True, tuple((nb - 2) * 64 + r for r in (56, 60, 63))))
    return out


def pair_edges(n, per_wg, mixed):
    """Block counts around the chain kernels' pairing threshold (kC2PairMinBlocks =
    64). mixed False: workgroup w's messages all have spelling w % 17's block count.
    mixed True: its messages cycle through nb = 1, an odd nb and an even nb, the odd
    and the even spelling walking all 8 x 8 combinations over 64 workgroups."""
    sp = pair_spellings()
    odd = [s for s in sp if s[0] % 2 == 1 and s[0] > 1]
    even = [s for s in sp if s[0] % 2 == 0]
    assert len(sp) == 17 and len(odd) == 8 and len(even) == 8
    lens = np.zeros(n, dtype=np.uint64)
    for i in range(n):
        w, m = divmod(i, per_wg)
        if not mixed:
            s = sp[w % len(sp)]
        else:
            s = (sp[0], odd[w % 8], even[(w // 8 + w) % 8])[m % 3]
        lens[i] = s[2][(m // 3 if mixed else m) % len(s[2])]
    return lens


# ---------------------------------------------------------------------------
# Cells (what a batch exercises, from its lengths alone)
# ---------------------------------------------------------------------------
def r_class(length):
    r = int(length) % 64
    return 0 if r == 0 else (1 if r < 56 else 2)


def len_cell(length):
    """(r class, nfull mod 4, nfull == 0) of one message length."""
    nfull = int(length) // 64
    return (r_class(length), nfull % 4, nfull == 0)


def wave_kinds(lens):
    """Kind of every 64-message wave: uniform, uniform but for lane 0, uniform but
    for one other lane, ragged."""
    lens = np.asarray(lens)
    kinds = []
    for s in range(0, len(lens), WAVE):
        w = lens[s:s + WAVE]
        if (w == w[0]).all():
            kinds.append(UNIFORM)
        elif len(w) > 2 and (w[1:] == w[1]).all():
            kinds.append(NEAR0)
        elif (w != w[0]).sum() == 1:
            kinds.append(NEAR_OTHER)
        else:
            kinds.append(RAGGED)
    return kinds


def lane_cells(lens):
    """{(r class, nfull mod 4, nfull == 0, wave kind, partial wave)} over the messages."""
    lens = np.asarray(lens)
    cells = set()
    for k, kind in enumerate(wave_kinds(lens)):
        w = lens[k * WAVE:(k + 1) * WAVE]
        for L in np.unique(w):
            cells.add(len_cell(L) + (kind, len(w) < WAVE))
    return cells


def pair_cells(lens, per_wg):
    """{(NB parity, NB vs 64, a shorter message present, length-only last block)}
    per workgroup, NB its longest message's block count, over its longest messages."""
    lens = np.asarray(lens, dtype=np.uint64)
    nb = blocks(lens)
    cells = set()
    for s in range(0, len(lens), per_wg):
        b, l = nb[s:s + per_wg], lens[s:s + per_wg]
        NB = int(b.max())
        for L in np.unique(l[b == NB]):
            cells.add((NB % 2, (NB > 64) - (NB < 64), bool((b < NB).any()), int(L) % 64 >= 56))
    return cells


# ---------------------------------------------------------------------------
# Kernel targets
# ---------------------------------------------------------------------------
LANE_PATTERNS = ("uniform64", "uniform56", "ragged", "near_uniform")


def _t(name, entry, n, want, patterns, policy="auto", env=None, order=False, fold=False, per_wg=0,
       fixed_n=False):
    return {"name": name, "entry": entry, "n": n, "want": want, "patterns": tuple(patterns), "policy": policy,
            "env": dict(env or {}), "order": order, "fold": fold, "per_wg": per_wg, "fixed_n": fixed_n}


def _only(**kw):
    """Counter deltas: the named ones, every other launch counter still."""
    d = dict.fromkeys(COUNTERS, 0)
    d.update(kw)
    return d


def targets():
    """Every in-process target. n is a function of the CU count (S = 4 CUs SIMDs);
    `want` the launch-counter deltas of the one call (None: not asserted -- a planned
    call also queues its head launches, whose size is decided on the GPU)."""
    def n_prefetch(c):
        return 64 * (4 * c + 2 * c + 3) - 27        # S + S/2 + 3 waves: the surplus exceeds S/2, no split

    def n_pair(c):
        return 64 * (12 * c + 2 * c + 3) - 27       # 3S + S/2 + 3 waves

    def n_pipe(c):
        return 64 * 300 - 27

    T = [
        _t("lane_prefetch", "batch", n_prefetch, _only(launches_lane=1), LANE_PATTERNS),
        _t("lane_pair", "batch", n_pair, _only(launches_lane=1), LANE_PATTERNS),
    ]
    for tag, fn in (("s5", lambda c: 64 * (4 * c + 5) - 27), ("half", lambda c: 64 * (4 * c + 2 * c) - 27)):
        for order in (False, True):
            T.append(_t("split_%s%s" % (tag, "_ordered" if order else ""), "batch", fn, _only(launches_split=1),
                        LANE_PATTERNS, order=order))
    # Policy lane: on a device of 256 CUs the cooperative range (n <= 128 CUs) holds
    # 64 x 300 - 27 under AUTO; uniform lengths: tests/test_gpu_policies.py
    T.append(_t("pipe", "batch", n_pipe, _only(launches_pipe=1), ("ragged", "near_uniform"), policy="lane",
                fixed_n=True))
    for fold in (False, True):
        for ws in ("0", "2"):
            want = dict.fromkeys(COUNTERS)
            want.update(launches_lane=1, launches_lane_ws=int(ws == "2"), launches_pipe=0, launches_split=0)
            T.append(_t("planned_%s_%s" % ("fold" if fold else "nofold", "ws" if ws == "2" else "static"),
                        "planned", n_prefetch, want, ("planned_uniform", "planned_r0", "ragged"),
                        env={"MSHA_LANE_WS": ws}, fold=fold))
    for g in UNIFORM_GROUPS:
        T.append(_t("uniform_prefetch_" + g, "uniform", n_prefetch, _only(launches_lane=1), (g,)))
        T.append(_t("uniform_pair_" + g, "uniform", n_pair, _only(launches_lane=1), (g,)))
    pair = ("pair_same", "pair_mixed")
    T += [
        _t("chain8", "batch", lambda c: 16 * c - 5, _only(launches_coop=1, launches_chain8=1), pair, per_wg=16),
        _t("chain2", "batch", lambda c: 64 * c - 5, _only(launches_coop=1, launches_chain2=1), pair, per_wg=64),
        _t("coop", "batch", lambda c: 128 * c - 5, _only(launches_coop=1), pair, per_wg=128),
        _t("coop_policy", "batch", lambda c: 64 * 300, _only(launches_coop=1), pair, policy="coop", per_wg=128,
           fixed_n=True),
        # k_digest_chain2's latency form (n <= 16 CUs, 64 KiB of dynamic LDS, EXCL false)
        _t("chain2_latency", "batch", lambda c: 16 * c - 5, _only(launches_coop=1, launches_chain2=1), pair,
           env={"MSHA_SMALL_CHAIN8": "0"}, per_wg=64),
    ]
    return T


def expected_kernel(t, cus, forced=-1):
    """(kernel, load mode) the restated thresholds give target t on `cus` CUs."""
    n = t["n"](cus)
    if t["entry"] == "planned":
        return planned_kernel(n, cus, t["policy"], t["env"].get("MSHA_LANE_WS") == "2")
    if t["entry"] == "uniform":
        return uniform_kernel(n, cus, forced)
    return batch_kernel(n, cus, t["policy"], t["env"].get("MSHA_SMALL_CHAIN8", "1") != "0", forced)


# (kernel, load mode) every target is meant to reach
TARGET_KERNEL = {"lane_prefetch": ("lane", 1), "lane_pair": ("lane", 2), "pipe": ("pipe", 3),
                 "chain8": ("chain8", 1), "chain2": ("chain2", 1), "coop": ("coop", 1), "coop_policy": ("coop", 1),
                 "chain2_latency": ("chain2", 1)}


def target_kernel(t):
    name = t["name"]
    if name in TARGET_KERNEL:
        return TARGET_KERNEL[name]
    if name.startswith("split_"):
        return ("split", 1)
    if name.startswith("planned_"):
        return ("lane_ws" if name.endswith("_ws") else "lane", 1)
    return ("lane", 1 if name.startswith("uniform_prefetch") else 2)


def pattern_lengths(t, pattern, cus):
    """The lengths of target t's batch under `pattern` (batch and planned targets)."""
    n = t["n"](cus)
    if pattern in ("uniform64", "uniform56"):
        return uniform_waves(n, int(pattern[-2:]))
    if pattern == "ragged":
        return ragged(n)
    if pattern == "near_uniform":
        return near_uniform(n)
    if pattern == "planned_uniform":
        return planned_classes(n, PLANNED_UNIFORM)
    if pattern == "planned_r0":
        return planned_classes(n, PLANNED_R0)
    if pattern in ("pair_same", "pair_mixed"):
        return pair_edges(n, t["per_wg"], pattern == "pair_mixed")
    raise KeyError(pattern)


def cases():
    """(target name, pattern) of every in-process case."""
    return [(t["name"], p) for t in targets() for p in t["patterns"]]


def target(name):
    return next(t for t in targets() if t["name"] == name)


# ---------------------------------------------------------------------------
# Inputs and the runner
# ---------------------------------------------------------------------------
def _salt(*what):
    import zlib
    return zlib.crc32(repr(what).encode()) << 8


def build_arena(lens, salt, min_stride=0):
    """A packed arena of random bytes: message i at a 16-byte aligned offset, 64
    bytes of slack after the last (as tests/test_gpu_parity.py _arena_from);
    min_stride 16 gives empty messages offsets of their own."""
    from mirbft_amd import workloads as W
    lens = np.asarray(lens, dtype=np.uint64)
    stride = np.maximum((lens + np.uint64(15)) // np.uint64(16) * np.uint64(16), np.uint64(min_stride))
    off = np.zeros(len(lens), dtype=np.uint64)
    off[1:] = np.cumsum(stride)[:-1]
    arena = W.random_bytes(W.SEED ^ 0xA7, salt, int(stride.sum()) + 64)
    return arena, off, lens


def uniform_arena(msg_len, stride, n, salt):
    from mirbft_amd import workloads as W
    arena = W.random_bytes(W.SEED ^ 0xA8, salt, n * stride + 64)
    off = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    return arena, off, np.full(n, msg_len, dtype=np.uint64)


def expected(arena, off, lens):
    from oracle import oracle
    return oracle.digest_batch(arena, off, lens)


def mismatch(what, lens, got, exp, waves_by_input=True, per_wg=0):
    """None when equal; else what a failed comparison tells: the target and pattern,
    how many digests differ, and for the first few the wave, lane, length and the
    kind of the wave (by input position: a planned call sorts its lanes); for the
    chain kernels also the workgroup and its longest message's block count."""
    bad = np.nonzero(np.any(got != exp, axis=1))[0]
    if bad.size == 0:
        return None
    kinds = wave_kinds(lens)
    first = [{"message": int(i), "wave": int(i) // WAVE, "lane": int(i) % WAVE, "len": int(lens[i]),
              "blocks": int(blocks(lens[i:i + 1])[0]),
              "wave_kind": KIND_NAMES[kinds[int(i) // WAVE]] if waves_by_input else "sorted by the planner"}
             for i in bad[:6]]
    if per_wg:
        nb = blocks(lens)
        for f in first:
            w = f["message"] // per_wg
            f.update(workgroup=w, workgroup_NB=int(nb[w * per_wg:(w + 1) * per_wg].max()))
    return {"what": what, "bad": int(bad.size), "of": int(len(lens)), "first": first}


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to("cuda:0")


def _deltas(st0, st1):
    return {k: st1[k] - st0[k] for k in COUNTERS}


def run_batch(eng, lens, what, order=False, salt=0, min_stride=0, per_wg=0):
    """One msha_digest_batch_device call -> (counter deltas, mismatch or None)."""
    import torch
    arena, off, lens = build_arena(lens, salt, min_stride)
    out = torch.full((len(lens), 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_order = None
    if order:
        from mirbft_amd.engine import order_by_blocks
        d_order = _dev(order_by_blocks(lens).view(np.int32))
    st0 = eng.stats()
    eng.digest_batch_device(_dev(arena), _dev(off), _dev(lens), out, order=d_order)
    eng.device_status()
    got = out.cpu().numpy()
    return _deltas(st0, eng.stats()), mismatch(what, lens, got, expected(arena, off, lens), not order, per_wg)


def run_planned(eng, lens, what, fold, salt=0):
    import torch
    arena, off, lens = build_arena(lens, salt, min_stride=16)   # distinct offsets: nothing folds
    out = torch.full((len(lens), 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    st0 = eng.stats()
    eng.digest_batch_device_planned(_dev(arena), _dev(off), _dev(lens), out, fold=fold)
    eng.device_status()
    got = out.cpu().numpy()
    return _deltas(st0, eng.stats()), mismatch(what, lens, got, expected(arena, off, lens), False)


def run_uniform(eng, msg_len, stride, n, what, salt=0):
    """One msha_digest_uniform_device launch."""
    import torch
    arena, off, lens = uniform_arena(msg_len, stride, n, salt)
    out = torch.full((n, 32), 0xA5, dtype=torch.uint8, device="cuda:0")
    st0 = eng.stats()
    eng.digest_uniform_device(_dev(arena), stride, msg_len, n, out)
    eng.device_status()
    got = out.cpu().numpy()
    return _deltas(st0, eng.stats()), mismatch(what, lens, got, expected(arena, off, lens))


def check_deltas(want, got, what):
    """The launch counters that prove which kernel ran (None: not asserted)."""
    diff = {k: (got[k], v) for k, v in want.items() if v is not None and got[k] != v}
    assert not diff, "%s: launch counters (got, want) %s; all deltas %s" % (what, diff, got)


def run_case(eng, name, pattern, cus):
    """One in-process case: the engine's policy and the environment are the
    caller's to set (target(name)["policy"] / ["env"]). Asserts the kernel's range,
    its launch counters and every digest."""
    t = target(name)
    what = "%s / %s (n = %d)" % (name, pattern, t["n"](cus))
    assert expected_kernel(t, cus) == target_kernel(t), \
        "%s: on %d CUs this n is outside its kernel's range (%s)" % (what, cus, expected_kernel(t, cus))
    n = t["n"](cus)
    if t["entry"] == "uniform":
        for msg_len, stride in UNIFORM_GROUPS[pattern]:
            w = "%s, msg_len %d stride %d" % (what, msg_len, stride)
            d, bad = run_uniform(eng, msg_len, stride, n, w, _salt(name, msg_len, stride))
            check_deltas(t["want"], d, w)
            assert bad is None, bad
        return
    lens = pattern_lengths(t, pattern, cus)
    if t["entry"] == "planned":
        d, bad = run_planned(eng, lens, what, t["fold"], _salt(name, pattern))
    else:
        d, bad = run_batch(eng, lens, what, t["order"], _salt(name, pattern), per_wg=t["per_wg"])
    check_deltas(t["want"], d, what)
    assert bad is None, bad


# ---------------------------------------------------------------------------
# Forced load modes (MSHA_LOAD_MODE), in a process of their own
# ---------------------------------------------------------------------------
CHILD_N = 64 * 300 - 27     # below one wave per SIMD on 256 CUs: no split; policy lane: no cooperative kernel
CHILD_PATTERNS = ("uniform64", "uniform56", "near_uniform", "ragged")


def child_split_n(cus):
    return 64 * (4 * cus + 5) - 27


def child_lengths(pattern, n):
    if pattern in ("uniform64", "uniform56"):
        return uniform_waves(n, int(pattern[-2:]))
    return near_uniform(n) if pattern == "near_uniform" else ragged(n)


def child_expected(case, mode, cus):
    """The kernel the restated thresholds give a child case under forced mode."""
    if case == "split":
        return batch_kernel(child_split_n(cus), cus, "lane", forced=mode)
    if case.startswith("uniform_len"):
        return uniform_kernel(CHILD_N, cus, mode)
    return batch_kernel(CHILD_N, cus, "lane", forced=mode)


def child_main():
    mode = int(os.environ["MSHA_LOAD_MODE"])
    import torch  # one HIP runtime per process: torch's, loaded before libmirsha (see mirbft_amd/_lib.py)
    torch.cuda.init()
    from mirbft_amd import Engine, _lib
    _lib.require_tree_build("tests/kernel_matrix.py --child")   # conftest.py's rule
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def emit(case, deltas, bad):
        print(json.dumps({"case": case, "mode": mode, "cus": cus, "deltas": deltas, "mismatch": bad}), flush=True)

    with Engine(1) as eng:
        eng.set_kernel_policy("lane")
        for p in CHILD_PATTERNS:
            emit(p, *run_batch(eng, child_lengths(p, CHILD_N), "mode %d / %s" % (mode, p), salt=_salt("child", p)))
        for g in UNIFORM_GROUPS.values():
            for msg_len, stride in g:
                case = "uniform_len%d_stride%d" % (msg_len, stride)
                emit(case, *run_uniform(eng, msg_len, stride, CHILD_N, "mode %d / %s" % (mode, case),
                                        _salt("child", case)))
        n = child_split_n(cus)
        emit("split", *run_batch(eng, ragged(n), "mode %d / split ragged" % mode, salt=_salt("child", "split")))
    return 0


def child_cases():
    return list(CHILD_PATTERNS) + ["uniform_len%d_stride%d" % ls for g in UNIFORM_GROUPS.values() for ls in g] + \
        ["split"]


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        sys.exit(child_main())
    sys.exit("usage: MSHA_LOAD_MODE=0..3 python tests/kernel_matrix.py --child")
