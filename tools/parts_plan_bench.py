#!/usr/bin/env python3
"""What msha_hash_actions_device_planned costs and gains, kernel-resident.

    python3 tools/parts_plan_bench.py [--reps 7] [--out profiles/parts_planned/parts_plan_bench.jsonl]

Cases (each entry a callable; all alternate in one process, as tools/parts_bench.py
times its pairs: warm-up repetitions for 300 ms so the clock settles, then `reps` timed
ones, a repetition being `inner` calls back to back between one pair of HIP events):
  uniform   `--lanes` lists of one 512-byte part: `planned` (the new entry), `unplanned`
            (msha_hash_actions_device over the same arrays) and `plan_only` (the new
            entry under MSHA_PARTS_PLAN_ONLY=1: init, measure, scan and scatter alone) --
            the planner's overhead where it has nothing to gain
  c5_noec   a c5-shaped batch without EpochChanges: 70/95 Requests of one 512-byte
            part, the rest Batches of k x 32-byte parts, k = 1..20, in input order:
            `planned` against `unplanned` -- the ordering's gain
  c5_ec     the same actions plus 5 % EpochChanges, the 100 lists of
            workloads.epoch_change_parts_pool() named through action_list: `planned`
            (there is no unplanned form: every action would repeat ~2,000 descriptors),
            `longest` (one action naming the pool's longest list, over the pool's lists
            alone: that lane's time, the floor of the step) and `plan_only`
  wave_sum  the A/B of the wave-sum threshold T (MSHA_PARTS_PLAN_WAVE_SUM, read at each
            call): `plan_only` of c5_ec's lists and of `--ec-copies` copies of the pool as
            lists of their own, at T = 4, 8, 16, 32, 64, 128 and "never"
Prints one JSON line an entry (ms of every repetition, the median, (max - min) /
median) and one line a comparison with `noise`: true when the larger spread, in ms, is
at least the difference of the medians. A sample of the digests of what was timed is
checked against hashlib. A measurement, not a threshold. Needs the GPU; no fallback.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NEVER = 1 << 30


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lanes", type=int, default=1 << 20, help="lists of the uniform case, actions of the c5 cases")
    ap.add_argument("--ec-copies", type=int, default=64, help="copies of the 100-list pool in the wave_sum A/B")
    ap.add_argument("--inner", type=int, default=4, help="calls between one pair of events")
    ap.add_argument("--min-warmup-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "parts_planned", "parts_plan_bench.jsonl"),
                    help="the JSON lines are written to this file too (replacing it; '' for none)")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 repetitions")
    import torch
    from mirbft_amd import Engine, _lib
    from mirbft_amd.workloads import SEED, epoch_change_parts_pool, scatter_parts, splitmix64
    build = _lib.require_tree_build("parts_plan_bench")
    dev = torch.device("cuda:0")

    def up(x):
        x = np.ascontiguousarray(x)
        if x.dtype == np.uint64:
            x = x.view(np.int64)
        if x.dtype == np.uint32:
            x = x.view(np.int32)
        return torch.from_numpy(x.copy()).to(dev)

    g = torch.Generator(device=dev)
    g.manual_seed(5)
    n = a.lanes

    # -- uniform: one 512-byte part a list
    stride = 528
    u_arena = torch.randint(0, 256, (n * stride + 64,), dtype=torch.uint8, device=dev, generator=g)
    u_off = torch.arange(n, dtype=torch.int64, device=dev) * stride
    u_len = torch.full((n,), 512, dtype=torch.int64, device=dev)
    u_begin = torch.arange(n + 1, dtype=torch.int64, device=dev)
    u_out = {k: torch.zeros((n, 32), dtype=torch.uint8, device=dev) for k in ("planned", "unplanned")}

    # -- c5 without EpochChanges: kinds and k drawn as workloads.c5_storm draws them
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
    c_off[1:] = np.cumsum(c_len)[:-1]              # parts back to back: 32-byte parts at 32-byte multiples
    own_bytes = int(c_off[-1] + c_len[-1])
    # -- the EpochChange pool, scattered, behind the own payloads (16-byte aligned base)
    pool = epoch_change_parts_pool()
    p_arena, p_off, p_len, p_begin = scatter_parts(pool)
    base = (own_bytes + 15) & ~15
    c_arena = torch.cat([torch.randint(0, 256, (base,), dtype=torch.uint8, device=dev, generator=g), up(p_arena)])
    d_coff, d_clen, d_cbegin = up(c_off), up(c_len), up(c_begin)
    c_out = {w: torch.zeros((n, 32), dtype=torch.uint8, device=dev) for w in ("planned", "unplanned")}
    # lists of c5_ec: the n own lists, then the 100 pool lists; 5 % of the actions name a pool list
    e_off = torch.cat([d_coff, up(p_off + np.uint64(base))])
    e_len = torch.cat([d_clen, up(p_len)])
    e_begin = torch.cat([d_cbegin, up(p_begin[1:] + np.uint64(total_parts))])
    pick = ((u >> np.uint64(16)) & np.uint64(0xFFFF)) % np.uint64(len(pool))
    is_ec = ((u >> np.uint64(48)) % np.uint64(20)) == 0
    e_al_host = np.where(is_ec, np.uint64(n) + pick, np.arange(n, dtype=np.uint64)).astype(np.uint32)
    e_al = up(e_al_host)
    e_out = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    pool_bytes = [sum(len(p) for p in m) for m in pool]
    longest = int(np.argmax(pool_bytes))
    l_al = up(np.array([longest], dtype=np.uint32))          # over the pool's 100 lists alone
    l_off, l_len, l_begin = up(p_off), up(p_len), up(p_begin)
    l_out = torch.zeros((1, 32), dtype=torch.uint8, device=dev)
    # the pool `copies` times as lists of their own (the part descriptors repeated, the bytes shared)
    c = a.ec_copies
    n_pp = int(p_off.size)
    x_off, x_len = up(p_off).repeat(c), up(p_len).repeat(c)
    step = torch.arange(c, dtype=torch.int64, device=dev).repeat_interleave(len(pool)) * n_pp
    x_begin = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), up(p_begin[1:]).repeat(c) + step])
    x_arena = up(p_arena)
    x_out = torch.zeros((len(pool) * c, 32), dtype=torch.uint8, device=dev)

    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    entries = {}      # (case, name) -> (callable, env)

    with Engine(1) as eng:
        def planned(arena, off, ln, begin, out, al=None):
            return lambda: eng.hash_actions_device_planned(arena, off, ln, begin, out, action_list=al, stream=stream)

        entries[("uniform", "planned")] = (planned(u_arena, u_off, u_len, u_begin, u_out["planned"]), {})
        entries[("uniform", "unplanned")] = (
            lambda: eng.hash_actions_device(u_arena, u_off, u_len, u_begin, u_out["unplanned"], stream=stream), {})
        entries[("uniform", "plan_only")] = (planned(u_arena, u_off, u_len, u_begin, u_out["planned"]),
                                             {"MSHA_PARTS_PLAN_ONLY": "1"})
        entries[("c5_noec", "planned")] = (planned(c_arena, d_coff, d_clen, d_cbegin, c_out["planned"]), {})
        entries[("c5_noec", "unplanned")] = (
            lambda: eng.hash_actions_device(c_arena, d_coff, d_clen, d_cbegin, c_out["unplanned"], stream=stream), {})
        entries[("c5_ec", "planned")] = (planned(c_arena, e_off, e_len, e_begin, e_out, e_al), {})
        entries[("c5_ec", "longest")] = (planned(x_arena, l_off, l_len, l_begin, l_out, l_al), {})
        entries[("c5_ec", "plan_only")] = (planned(c_arena, e_off, e_len, e_begin, e_out, e_al),
                                           {"MSHA_PARTS_PLAN_ONLY": "1"})
        for t in (4, 8, 16, 32, 64, 128, NEVER):
            env = {"MSHA_PARTS_PLAN_ONLY": "1", "MSHA_PARTS_PLAN_WAVE_SUM": str(t)}
            tag = "never" if t == NEVER else str(t)
            entries[("wave_sum", "c5_ec T=" + tag)] = (planned(c_arena, e_off, e_len, e_begin, e_out, e_al), env)
            entries[("wave_sum", "pool_x%d T=%s" % (c, tag))] = (planned(x_arena, x_off, x_len, x_begin, x_out), env)

        def run(fn, env):
            for k_, v in env.items():
                os.environ[k_] = v
            try:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.inner):
                    fn()
                e1.record(stream)
                e1.synchronize()
                return e0.elapsed_time(e1) / a.inner
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
            for key, (fn, env) in entries.items():
                ms = run(fn, env)
                if rep:
                    times[key].append(ms)
        # the digests checked below come from full calls made last
        for key in (("uniform", "planned"), ("uniform", "unplanned"), ("c5_noec", "planned"),
                    ("c5_noec", "unplanned"), ("c5_ec", "planned"), ("c5_ec", "longest")):
            entries[key][0]()
        planned(x_arena, x_off, x_len, x_begin, x_out)()
        os.environ["MSHA_PARTS_TIMING"] = "1"          # one more c5_ec call, for its lanes and blocks
        entries[("c5_ec", "planned")][0]()
        del os.environ["MSHA_PARTS_TIMING"]
        eng.device_status()
        stats = eng.parts_plan_stats()

    # what was timed computed the right thing (a sample, against hashlib)
    for i in [0, 1, 63, 64, n // 2, n - 1]:
        host = u_arena[i * stride:i * stride + 512].cpu().numpy().tobytes()
        for w in ("planned", "unplanned"):
            assert bytes(u_out[w][i].cpu().numpy()) == hashlib.sha256(host).digest(), ("uniform", w, i)
        lo, hi = int(c_off[int(c_begin[i])]), int(c_off[int(c_begin[i + 1]) - 1] + c_len[int(c_begin[i + 1]) - 1])
        want = hashlib.sha256(c_arena[lo:hi].cpu().numpy().tobytes()).digest()        # own parts are back to back
        for w in ("planned", "unplanned"):
            assert bytes(c_out[w][i].cpu().numpy()) == want, ("c5_noec", w, i)
        if not is_ec[i]:
            assert bytes(e_out[i].cpu().numpy()) == want, ("c5_ec own", i)
    pool_digest = [hashlib.sha256(b"".join(m)).digest() for m in pool]
    for i in np.nonzero(is_ec)[0][:6].tolist():
        assert bytes(e_out[i].cpu().numpy()) == pool_digest[int(e_al_host[i]) - n], ("c5_ec pool", i)
    assert bytes(l_out[0].cpu().numpy()) == pool_digest[longest], "longest"
    for i in [0, 99, 100, len(pool) * c - 1]:
        assert bytes(x_out[i].cpu().numpy()) == pool_digest[i % len(pool)], ("pool copies", i)

    shapes = {"uniform": {"lists": n, "part_bytes": 512},
              "c5_noec": {"lists": n, "parts": total_parts, "requests": int(is_req.sum())},
              "c5_ec": {"actions": n, "lists": n + len(pool), "pool_actions": int(is_ec.sum()),
                        "longest_list": {"parts": int(p_begin[longest + 1] - p_begin[longest]),
                                         "bytes": pool_bytes[longest]}},
              "wave_sum": {"pool_lists": len(pool) * c, "pool_parts_a_list_mean": n_pp // len(pool)}}
    lines, med, spread_ms = [], {}, {}
    for key, ts in times.items():
        med[key] = statistics.median(ts)
        spread_ms[key] = max(ts) - min(ts)
        lines.append({"case": key[0], "entry": key[1], "shape": shapes[key[0]], "reps": a.reps, "inner": a.inner,
                      "warmup_reps": warm, "ms": [round(t, 4) for t in ts], "median_ms": round(med[key], 4),
                      "spread": round(spread_ms[key] / med[key], 4), "build": build["id"]})

    def compare(case, x, y, what):
        kx, ky = (case, x), (case, y)
        diff = med[kx] - med[ky]
        lines.append({"case": case, "compare": what, "%s_minus_%s_ms" % (x, y): round(diff, 4),
                      "ratio": round(med[kx] / med[ky], 4),
                      "noise": bool(max(spread_ms[kx], spread_ms[ky]) >= abs(diff))})
    compare("uniform", "planned", "unplanned", "the planner's overhead on a uniform batch")
    compare("c5_noec", "planned", "unplanned", "the ordering's gain (negative: planned is faster)")
    compare("c5_ec", "planned", "longest", "the folded step against its longest lane alone")
    lines.append({"case": "c5_ec", "timed_call_stats": stats})
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
