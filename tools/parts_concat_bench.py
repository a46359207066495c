#!/usr/bin/env python3
"""What msha_concat_lists_device costs, and what the long-list route gains, kernel-resident.

    python3 tools/parts_concat_bench.py [--reps 7] [--out profiles/parts_concat/parts_concat_bench.jsonl]

Cases (each entry a callable; all alternate in one process, as tools/parts_plan_bench.py
times its entries: warm-up repetitions for 300 ms so the clock settles, then `reps` timed
ones, a repetition being `inner` calls back to back between one pair of HIP events):
  pool      the 100 lists of workloads.epoch_change_parts_pool(), scattered: `concat` (the
            new entry alone), `copy` (a device-to-device copy_ of the same byte count: the
            yardstick), `concat_digest` (the long-list route: concat, then
            digest_batch_device over the result) and `planned` (the same 100 lists through
            hash_actions_device_planned: the parts path)
  uniform   `--lanes` lists of one 512-byte part: `concat`, `copy`, `measure_scan` (the
            entry under MSHA_CONCAT_SCAN_ONLY=1) and `scan` (=2: k_concat_scan alone, one
            call a repetition over lengths put back before it)
  c5_ec     tools/parts_plan_bench.py's storm: `--lanes` actions, 5 % of them
            EpochChanges that name the pool's lists through action_list. `planned`: one
            hash_actions_device_planned call. `split`: the own lists through
            hash_actions_device_planned (action i = list i), the pool through
            concat_lists_device, msg_off[idx] / msg_len[idx] by a device index-select per
            EpochChange action, digest_batch_device_planned(fold=True) over those, and the
            digests scattered to their actions' rows
Prints one JSON line an entry (ms of every repetition, the median, (max - min) / median)
and one line a comparison with `noise`: true when the larger spread, in ms, is at least
the difference of the medians. Every digest of the two c5_ec forms and of the pool
routes is compared with the oracle or hashlib once, outside the timed window; the
concat outputs are compared with a host concatenation. A measurement, not a threshold.
Needs the GPU; no fallback.
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lanes", type=int, default=1 << 20, help="lists of the uniform case, actions of c5_ec")
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--min-warmup-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "parts_concat", "parts_concat_bench.jsonl"),
                    help="the JSON lines are written to this file too (replacing it; '' for none)")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("at least 7 repetitions")
    import torch
    from mirbft_amd import Engine, _lib
    from mirbft_amd.workloads import SEED, epoch_change_parts_pool, scatter_parts, splitmix64
    from oracle import oracle
    build = _lib.require_tree_build("parts_concat_bench")
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
    p_need = int(r16(pool_bytes).sum()) + SLACK
    dp_arena, dp_off, dp_len, dp_begin = up(p_arena), up(p_off), up(p_len), up(p_begin)
    p_dst = torch.zeros(p_need, dtype=torch.uint8, device=dev)
    p_moff = torch.zeros(len(pool), dtype=torch.int64, device=dev)
    p_mlen = torch.zeros(len(pool), dtype=torch.int64, device=dev)
    p_out = {w: torch.zeros((len(pool), 32), dtype=torch.uint8, device=dev) for w in ("concat_digest", "planned")}
    p_src = torch.randint(0, 256, (p_need - SLACK,), dtype=torch.uint8, device=dev, generator=g)
    p_cpy = torch.zeros_like(p_src)

    # -- uniform: one 512-byte part a list
    stride = 528
    u_arena = torch.randint(0, 256, (n * stride + 64,), dtype=torch.uint8, device=dev, generator=g)
    u_off = torch.arange(n, dtype=torch.int64, device=dev) * stride + 8      # parts at phase 8
    u_len = torch.full((n,), 512, dtype=torch.int64, device=dev)
    u_begin = torch.arange(n + 1, dtype=torch.int64, device=dev)
    u_dst = torch.zeros(n * 512 + SLACK, dtype=torch.uint8, device=dev)
    u_moff = torch.zeros(n, dtype=torch.int64, device=dev)
    u_mlen = torch.zeros(n, dtype=torch.int64, device=dev)
    u_src = torch.randint(0, 256, (n * 512,), dtype=torch.uint8, device=dev, generator=g)
    u_cpy = torch.zeros_like(u_src)

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
    e_out = {w: torch.zeros((n, 32), dtype=torch.uint8, device=dev) for w in ("planned", "split")}
    ec_rows = up(np.nonzero(is_ec)[0].astype(np.int64))          # the EpochChange actions' rows ...
    ec_pick = up(pick[is_ec])                                    # ... and the pool list each names
    n_ec = int(is_ec.sum())
    s_dst = torch.zeros(p_need, dtype=torch.uint8, device=dev)
    s_moff = torch.zeros(len(pool), dtype=torch.int64, device=dev)
    s_mlen = torch.zeros(len(pool), dtype=torch.int64, device=dev)
    s_out = torch.zeros((n_ec, 32), dtype=torch.uint8, device=dev)

    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    entries = {}      # (case, name) -> (callable, env, prepare or None)

    with Engine(1) as eng:
        def concat_pool(dst, moff, mlen):
            eng.concat_lists_device(dp_arena, dp_off, dp_len, dp_begin, dst, moff, mlen, stream=stream)

        def pool_route():
            concat_pool(p_dst, p_moff, p_mlen)
            eng.digest_batch_device(p_dst, p_moff, p_mlen, p_out["concat_digest"], stream=stream)

        def concat_uniform():
            eng.concat_lists_device(u_arena, u_off, u_len, u_begin, u_dst, u_moff, u_mlen, stream=stream)

        def copy(dst, src):
            def f():
                with torch.cuda.stream(stream):
                    dst.copy_(src)
            return f

        def scan_prepare():
            with torch.cuda.stream(stream):
                u_moff.zero_()
                u_mlen.fill_(512)

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

        entries[("pool", "concat")] = (lambda: concat_pool(p_dst, p_moff, p_mlen), {}, None)
        entries[("pool", "copy")] = (copy(p_cpy, p_src), {}, None)
        entries[("pool", "concat_digest")] = (pool_route, {}, None)
        entries[("pool", "planned")] = (
            lambda: eng.hash_actions_device_planned(dp_arena, dp_off, dp_len, dp_begin, p_out["planned"],
                                                    stream=stream), {}, None)
        entries[("uniform", "concat")] = (concat_uniform, {}, None)
        entries[("uniform", "copy")] = (copy(u_cpy, u_src), {}, None)
        entries[("uniform", "measure_scan")] = (concat_uniform, {"MSHA_CONCAT_SCAN_ONLY": "1"}, None)
        entries[("uniform", "scan")] = (concat_uniform, {"MSHA_CONCAT_SCAN_ONLY": "2"}, scan_prepare)
        entries[("c5_ec", "planned")] = (storm_planned, {}, None)
        entries[("c5_ec", "split")] = (storm_split, {}, None)

        def run(fn, env, prepare):
            for k_, v in env.items():
                os.environ[k_] = v
            try:
                inner = 1 if prepare else a.inner
                if prepare:
                    prepare()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(inner):
                    fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / inner
            finally:
                for k_ in env:
                    del os.environ[k_]

        times = {key: [] for key in entries}
        t_start, rep, warm = time.perf_counter(), 0, 0
        while rep < a.reps:                    # warm-up repetitions first (at least one), untimed
            warming = warm == 0 or (time.perf_counter() - t_start) * 1e3 < a.min_warmup_ms
            if warming and rep == 0:
                warm += 1
            else:
                rep += 1
            for key, (fn, env, prepare) in entries.items():
                ms = run(fn, env, prepare)
                if rep:
                    times[key].append(ms)
        # what is checked below comes from full calls made last
        for key in (("pool", "concat_digest"), ("pool", "planned"), ("uniform", "concat"), ("c5_ec", "planned"),
                    ("c5_ec", "split")):
            entries[key][0]()
        os.environ["MSHA_PARTS_TIMING"] = "1"          # one more pool call, for its bytes and kernel time
        concat_pool(p_dst, p_moff, p_mlen)
        del os.environ["MSHA_PARTS_TIMING"]
        eng.device_status()
        stats = eng.concat_stats()

    # what was timed computed the right thing
    want_off = np.concatenate([[0], np.cumsum(r16(pool_bytes))[:-1]])
    assert np.array_equal(p_moff.cpu().numpy(), want_off) and np.array_equal(p_mlen.cpu().numpy(), pool_bytes)
    assert stats["last_bytes"] == p_need - SLACK
    host_dst = p_dst.cpu().numpy()
    pool_digest = [hashlib.sha256(b"".join(m)).digest() for m in pool]
    for i, m in enumerate(pool):
        o = int(want_off[i])
        assert host_dst[o:o + int(pool_bytes[i])].tobytes() == b"".join(m), ("pool concat", i)
        assert not host_dst[o + int(pool_bytes[i]):o + int(r16(pool_bytes[i]))].any(), ("pool pad", i)
        for w in ("concat_digest", "planned"):
            assert bytes(p_out[w][i].cpu().numpy()) == pool_digest[i], ("pool", w, i)
    assert np.array_equal(u_moff.cpu().numpy(), np.arange(n, dtype=np.int64) * 512)
    for i in [0, 1, 63, 64, n // 2, n - 1]:
        assert torch.equal(u_dst[i * 512:(i + 1) * 512], u_arena[i * stride + 8:i * stride + 520]), ("uniform", i)
    # every digest of both storm forms: the own actions against the oracle (their parts are back to
    # back, a contiguous message each), the EpochChange actions against hashlib of the pool
    host_arena = c_arena[:base + SLACK].cpu().numpy()
    lo = c_off[c_begin[:-1].astype(np.int64)]
    own_len = np.diff(np.concatenate([c_off, [np.uint64(own_bytes)]]).astype(np.uint64)[c_begin.astype(np.int64)])
    want = oracle.digest_batch(host_arena, lo.astype(np.uint64), own_len.astype(np.uint64)).copy()
    table = np.frombuffer(b"".join(pool_digest), dtype=np.uint8).reshape(-1, 32)
    want[is_ec] = table[pick[is_ec]]
    for w in ("planned", "split"):
        bad = np.nonzero((e_out[w].cpu().numpy() != want).any(axis=1))[0]
        assert bad.size == 0, ("c5_ec", w, bad[:8].tolist())

    shapes = {"pool": {"lists": len(pool), "parts": int(p_off.size), "bytes": int(pool_bytes.sum()),
                       "longest_list": {"parts": int(np.diff(p_begin).max()), "bytes": int(pool_bytes.max())}},
              "uniform": {"lists": n, "part_bytes": 512, "bytes": n * 512},
              "c5_ec": {"actions": n, "own_lists": n, "own_parts": total_parts, "pool_actions": n_ec}}
    lines, med, spread_ms = [], {}, {}
    for key, ts in times.items():
        med[key] = statistics.median(ts)
        spread_ms[key] = max(ts) - min(ts)
        lines.append({"case": key[0], "entry": key[1], "shape": shapes[key[0]], "reps": a.reps,
                      "inner": 1 if entries[key][2] else a.inner, "warmup_reps": warm,
                      "ms": [round(t, 4) for t in ts], "median_ms": round(med[key], 4),
                      "spread": round(spread_ms[key] / med[key], 4), "build": build["id"]})

    def compare(case, x, y, what):
        kx, ky = (case, x), (case, y)
        diff = med[kx] - med[ky]
        lines.append({"case": case, "compare": what, "%s_minus_%s_ms" % (x, y): round(diff, 4),
                      "ratio": round(med[kx] / med[ky], 4),
                      "noise": bool(max(spread_ms[kx], spread_ms[ky]) >= abs(diff))})
    compare("pool", "concat", "copy", "the concat against a device copy of the same bytes")
    compare("uniform", "concat", "copy", "the concat against a device copy of the same bytes")
    compare("pool", "concat_digest", "planned", "the long-list route against the parts path (negative: the route is faster)")
    compare("c5_ec", "split", "planned", "the split storm against one planned call (negative: split is faster)")
    lines.append({"case": "pool", "timed_call_stats": stats})
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
