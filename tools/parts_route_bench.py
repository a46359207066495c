#!/usr/bin/env python3
"""What msha_hash_actions_device_routed gains on batches with long lists, what it costs on
batches without, and which long_blocks threshold should be its default; kernel-resident.

    python3 tools/parts_route_bench.py [--reps 7] [--out profiles/parts_routed/parts_route_bench.jsonl]

The shapes and seeds are tools/parts_concat_bench.py's, and so is the timing: all entries
alternate in one process, warm-up repetitions for 300 ms so the clock settles, then
`reps` timed ones, a repetition being `inner` calls back to back between one pair of HIP
events.
  c5_ec     the storm: `--lanes` actions, 5 % of them EpochChanges that name the pool's
            100 lists through action_list. `routed`: one hash_actions_device_routed call,
            default options. `planned`: one hash_actions_device_planned call (the
            yardstick, re-measured here). `split`: what a caller who knows the long
            lists does today -- the own lists planned, the pool through
            concat_lists_device, two index-selects, digest_batch_device_planned(fold)
            and a scatter of the digests (parts_concat_bench.py storm_split).
            `routed_lb16` .. `routed_lb1024`: the routed call at that long_blocks.
  pool      the 100 EpochChange lists alone: `routed`, `concat_digest` (concat, then
            digest_batch_device), `planned`, and the same sweep.
  uniform   `--lanes` lists of one 512-byte part, nothing long: `routed` and `planned`.
            The difference is what routing costs when there is nothing to route.
Prints one JSON line an entry (ms of every repetition, the median, (max - min) / median,
the library's build id), one line a comparison with `noise`: true when the larger
spread, in ms, is at least the difference of the medians, and one line with the default
the sweep's rule gives: the lowest storm median; values within the larger spread of it
tie, and the largest threshold of a tie wins, because it routes least. Every digest of
every entry is compared with the oracle or hashlib once, outside the timed window.
A measurement, not a threshold. Needs the GPU; no fallback.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP = (16, 64, 256, 1024)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lanes", type=int, default=1 << 20, help="lists of the uniform case, actions of c5_ec")
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--min-warmup-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parts_routed", "parts_route_bench.jsonl"),
                    help="the JSON lines are written to this file too (replacing it; '' for none)")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    import torch
    from mirbft_amd import Engine, _lib
    from mirbft_amd.workloads import SEED, epoch_change_parts_pool, scatter_parts, splitmix64
    from oracle import oracle
    build = _lib.require_tree_build("parts_route_bench")
    dev = torch.device("cuda:0")
    SLACK = _lib.MSHA_DEVICE_ARENA_SLACK

    def up(x):
        x = np.ascontiguousarray(x)
        if x.dtype == np.uint64:
            x = x.view(np.int64)
        if x.dtype == np.uint32:
            x = x.view(np.int32)
        return torch.from_numpy(x.copy()).to(dev)

    def r16(x):
        return (x + 15) & ~15

    g = torch.Generator(device=dev)
    g.manual_seed(5)
    n = a.lanes

    # -- pool: the 100 EpochChange lists, scattered
    pool = epoch_change_parts_pool()
    p_arena, p_off, p_len, p_begin = scatter_parts(pool)
    pool_bytes = np.array([sum(len(p) for p in m) for m in pool], dtype=np.int64)
    pool_blocks = pool_bytes // 64 + np.where(pool_bytes % 64 < 56, 1, 2)
    p_need = int(r16(pool_bytes).sum()) + SLACK
    dp_arena, dp_off, dp_len, dp_begin = up(p_arena), up(p_off), up(p_len), up(p_begin)
    p_dst = torch.zeros(p_need, dtype=torch.uint8, device=dev)
    p_moff = torch.zeros(len(pool), dtype=torch.int64, device=dev)
    p_mlen = torch.zeros(len(pool), dtype=torch.int64, device=dev)
    pool_names = ["routed", "concat_digest", "planned"] + ["routed_lb%d" % v for v in SWEEP]
    p_out = {w: torch.zeros((len(pool), 32), dtype=torch.uint8, device=dev) for w in pool_names}

    # -- uniform: one 512-byte part a list
    stride = 528
    u_arena = torch.randint(0, 256, (n * stride + 64,), dtype=torch.uint8, device=dev, generator=g)
    u_off = torch.arange(n, dtype=torch.int64, device=dev) * stride + 8      # parts at phase 8
    u_len = torch.full((n,), 512, dtype=torch.int64, device=dev)
    u_begin = torch.arange(n + 1, dtype=torch.int64, device=dev)
    u_out = {w: torch.zeros((n, 32), dtype=torch.uint8, device=dev) for w in ("routed", "planned")}

    # -- c5_ec: kinds and k drawn as tools/parts_plan_bench.py draws them
    u = splitmix64(SEED ^ 0xC5, 0, n)
    kind_r = (u >> np.uint64(32)).astype(np.float64) / 2.0 ** 32
    is_req = kind_r < 0.70 / 0.95
    k = ((u & np.uint64(0xFFFF)) % np.uint64(20) + np.uint64(1)).astype(np.int64)
    nparts = np.where(is_req, 1, k)
    c_begin = np.zeros(n + 1, dtype=np.uint64)
    c_begin[1:] = np.cumsum(nparts)
    total_parts = int(c_begin[-1])
    c_len = np.repeat(np.where(is_req, 512, 32), nparts).astype(np.uint64)
    c_off = np.zeros(total_parts, dtype=np.uint64)
    c_off[1:] = np.cumsum(c_len)[:-1]
    own_bytes = int(c_off[-1] + c_len[-1])
    base = (own_bytes + 15) & ~15
    c_arena = torch.cat([torch.randint(0, 256, (base,), dtype=torch.uint8, device=dev, generator=g), dp_arena])
    d_coff, d_clen, d_cbegin = up(c_off), up(c_len), up(c_begin)
    e_off = torch.cat([d_coff, up(p_off + np.uint64(base))])
    e_len = torch.cat([d_clen, dp_len])
    e_begin = torch.cat([d_cbegin, up(p_begin[1:] + np.uint64(total_parts))])
    pick = (((u >> np.uint64(16)) & np.uint64(0xFFFF)) % np.uint64(len(pool))).astype(np.int64)
    is_ec = ((u >> np.uint64(48)) % np.uint64(20)) == 0
    e_al_host = np.where(is_ec, n + pick, np.arange(n, dtype=np.int64)).astype(np.uint32)
    e_al = up(e_al_host)
    storm_names = ["routed", "planned", "split"] + ["routed_lb%d" % v for v in SWEEP]
    e_out = {w: torch.zeros((n, 32), dtype=torch.uint8, device=dev) for w in storm_names}
    ec_rows = up(np.nonzero(is_ec)[0].astype(np.int64))          # the EpochChange actions' rows ...
    ec_pick = up(pick[is_ec])                                    # ... and the pool list each names
    n_ec = int(is_ec.sum())
    s_dst = torch.zeros(p_need, dtype=torch.uint8, device=dev)
    s_moff = torch.zeros(len(pool), dtype=torch.int64, device=dev)
    s_mlen = torch.zeros(len(pool), dtype=torch.int64, device=dev)
    s_out = torch.zeros((n_ec, 32), dtype=torch.uint8, device=dev)
    own_blocks_max = int((np.where(is_req, 512, 32 * k) // 64 + 1).max())

    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    entries = {}      # (case, name) -> callable

    with Engine(1) as eng:
        def concat_pool(dst, moff, mlen):
            eng.concat_lists_device(dp_arena, dp_off, dp_len, dp_begin, dst, moff, mlen, stream=stream)

        def pool_route():
            concat_pool(p_dst, p_moff, p_mlen)
            eng.digest_batch_device(p_dst, p_moff, p_mlen, p_out["concat_digest"], stream=stream)

        def pool_routed(name, lb):
            return lambda: eng.hash_actions_device_routed(dp_arena, dp_off, dp_len, dp_begin, p_out[name],
                                                          stream=stream, long_blocks=lb)

        def storm_routed(name, lb):
            return lambda: eng.hash_actions_device_routed(c_arena, e_off, e_len, e_begin, e_out[name],
                                                          action_list=e_al, stream=stream, long_blocks=lb)

        def storm_planned():
            eng.hash_actions_device_planned(c_arena, e_off, e_len, e_begin, e_out["planned"], action_list=e_al,
                                            stream=stream)

        def storm_split():
            eng.hash_actions_device_planned(c_arena, d_coff, d_clen, d_cbegin, e_out["split"], stream=stream)
            concat_pool(s_dst, s_moff, s_mlen)
            with torch.cuda.stream(stream):
                off = s_moff.index_select(0, ec_pick)
                ln = s_mlen.index_select(0, ec_pick)
            eng.digest_batch_device_planned(s_dst, off, ln, s_out, stream=stream, fold=True)
            with torch.cuda.stream(stream):
                e_out["split"].index_copy_(0, ec_rows, s_out)

        entries[("c5_ec", "routed")] = storm_routed("routed", 0)
        entries[("c5_ec", "planned")] = storm_planned
        entries[("c5_ec", "split")] = storm_split
        entries[("pool", "routed")] = pool_routed("routed", 0)
        entries[("pool", "concat_digest")] = pool_route
        entries[("pool", "planned")] = lambda: eng.hash_actions_device_planned(
            dp_arena, dp_off, dp_len, dp_begin, p_out["planned"], stream=stream)
        entries[("uniform", "routed")] = lambda: eng.hash_actions_device_routed(
            u_arena, u_off, u_len, u_begin, u_out["routed"], stream=stream)
        entries[("uniform", "planned")] = lambda: eng.hash_actions_device_planned(
            u_arena, u_off, u_len, u_begin, u_out["planned"], stream=stream)
        for v in SWEEP:
            entries[("c5_ec", "routed_lb%d" % v)] = storm_routed("routed_lb%d" % v, v)
            entries[("pool", "routed_lb%d" % v)] = pool_routed("routed_lb%d" % v, v)

        def run(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.inner):
                fn()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) / a.inner

        times = {key: [] for key in entries}
        t_start, rep, warm = time.perf_counter(), 0, 0
        while rep < a.reps:                    # warm-up repetitions first (at least one), untimed
            warming = warm == 0 or (time.perf_counter() - t_start) * 1e3 < a.min_warmup_ms
            if warming and rep == 0:
                warm += 1
            else:
                rep += 1
            for key, fn in entries.items():
                ms = run(fn)
                if rep:
                    times[key].append(ms)
        eng.device_status()
        # one more call of each routed default under MSHA_PARTS_TIMING=1, for what it routed
        os.environ["MSHA_PARTS_TIMING"] = "1"
        routed_stats = {}
        for case in ("c5_ec", "pool", "uniform"):
            entries[(case, "routed")]()
            routed_stats[case] = eng.parts_route_stats()
        del os.environ["MSHA_PARTS_TIMING"]
        eng.device_status()
        torch.cuda.synchronize()

    # what was timed computed the right thing: every digest of every entry
    pool_digest = [hashlib.sha256(b"".join(m)).digest() for m in pool]
    table = np.frombuffer(b"".join(pool_digest), dtype=np.uint8).reshape(-1, 32)
    for w in pool_names:
        bad = np.nonzero((p_out[w].cpu().numpy() != table).any(axis=1))[0]
        assert bad.size == 0, ("pool", w, bad[:8].tolist())
    host_arena = c_arena[:base + SLACK].cpu().numpy()
    lo = c_off[c_begin[:-1].astype(np.int64)]
    own_len = np.diff(np.concatenate([c_off, [np.uint64(own_bytes)]]).astype(np.uint64)[c_begin.astype(np.int64)])
    want = oracle.digest_batch(host_arena, lo.astype(np.uint64), own_len.astype(np.uint64)).copy()
    want[is_ec] = table[pick[is_ec]]
    for w in storm_names:
        bad = np.nonzero((e_out[w].cpu().numpy() != want).any(axis=1))[0]
        assert bad.size == 0, ("c5_ec", w, bad[:8].tolist())
    host_u = u_arena.cpu().numpy()
    want_u = oracle.digest_batch(host_u, (np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(8)),
                                 np.full(n, 512, dtype=np.uint64))
    for w in ("routed", "planned"):
        bad = np.nonzero((u_out[w].cpu().numpy() != want_u).any(axis=1))[0]
        assert bad.size == 0, ("uniform", w, bad[:8].tolist())
    assert routed_stats["uniform"]["last_routed"] == 0 and routed_stats["uniform"]["last_lanes"] == n
    named_pool = len(set(pick[is_ec].tolist()))
    long_default = int((pool_blocks >= _lib.MSHA_ROUTE_LONG_BLOCKS_DEFAULT).sum())
    assert routed_stats["pool"]["last_routed"] == long_default

    shapes = {"pool": {"lists": len(pool), "parts": int(p_off.size), "bytes": int(pool_bytes.sum()),
                       "flat_bytes": int(r16(pool_bytes).sum()),
                       "blocks_min": int(pool_blocks.min()), "blocks_max": int(pool_blocks.max()),
                       "longest_list": {"parts": int(np.diff(p_begin).max()), "bytes": int(pool_bytes.max())}},
              "uniform": {"lists": n, "part_bytes": 512, "bytes": n * 512},
              "c5_ec": {"actions": n, "own_lists": n, "own_parts": total_parts, "own_blocks_max": own_blocks_max,
                        "pool_actions": n_ec, "pool_lists_named": named_pool}}
    lines, med, spread_ms = [], {}, {}
    for key, ts in times.items():
        med[key] = statistics.median(ts)
        spread_ms[key] = max(ts) - min(ts)
        lines.append({"case": key[0], "entry": key[1], "shape": shapes[key[0]], "reps": a.reps,
                      "inner": a.inner, "warmup_reps": warm,
                      "ms": [round(t, 4) for t in ts], "median_ms": round(med[key], 4),
                      "spread": round(spread_ms[key] / med[key], 4), "spread_ms": round(spread_ms[key], 4),
                      "build": build["id"]})

    def compare(case, x, y, what):
        kx, ky = (case, x), (case, y)
        diff = med[kx] - med[ky]
        lines.append({"case": case, "compare": what, "%s_minus_%s_ms" % (x, y): round(diff, 4),
                      "ratio": round(med[kx] / med[ky], 4),
                      "noise": bool(max(spread_ms[kx], spread_ms[ky]) >= abs(diff)), "build": build["id"]})
    compare("c5_ec", "routed", "planned", "the routed storm against one planned call (negative: routed is faster)")
    compare("c5_ec", "routed", "split", "the routed storm against the caller's split (negative: routed is faster)")
    compare("pool", "routed", "planned", "the routed pool against the parts path (negative: routed is faster)")
    compare("pool", "routed", "concat_digest", "the routed pool against concat + digest (negative: routed is faster)")
    compare("uniform", "routed", "planned", "what routing costs when nothing is long (positive: routed is slower)")

    # the default: the lowest storm median; ties within the larger spread; the largest of a tie
    keys = [("c5_ec", "routed_lb%d" % v) for v in SWEEP]
    best = min(keys, key=lambda kk: med[kk])
    tie = [v for v, kk in zip(SWEEP, keys) if abs(med[kk] - med[best]) <= max(spread_ms[kk], spread_ms[best])]
    lines.append({"sweep": "long_blocks", "storm_median_ms": {str(v): round(med[kk], 4) for v, kk in zip(SWEEP, keys)},
                  "pool_median_ms": {str(v): round(med[("pool", "routed_lb%d" % v)], 4) for v in SWEEP},
                  "lowest": int(best[1].split("lb")[1]), "tie": tie, "default_by_rule": max(tie),
                  "default_in_header": _lib.MSHA_ROUTE_LONG_BLOCKS_DEFAULT, "build": build["id"]})
    lines.append({"timed_call_stats": routed_stats, "build": build["id"]})
    for ln in lines:
        print(json.dumps(ln))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
