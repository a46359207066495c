"""The probes, the numbering and the decisions of the device digest maps
(mirbft_amd/csrc/dmap.hpp) under AddressSanitizer + UBSan, as a stand-alone program with
its own main (tests/cpp/dmap_check.cpp) over the sequences the GPU test runs
(tests/dmap_matrix.py; all but the one that is too long for a sanitizer run), the inserts
in three slot orders, its results compared with the dict oracle; the sequences proven to
cover what they claim; and the oracle's comparison shown to reject wrong results. Host
code only: nothing is loaded into Python."""
import os
import subprocess

import numpy as np

import dmap_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _by_name():
    seqs = M.all_sequences()
    names = [s.name for s in seqs]
    assert len(set(names)) == len(names)
    return {s.name: s for s in seqs}


def test_sequences_cover_what_they_claim():
    S = _by_name()
    T = M.TILE
    assert M.launches() == 7 and M.sizes() == [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1]
    # one call on an empty map: every size with every pattern; all distinct fits exactly
    for n in M.sizes():
        p = M.patterns(n)
        assert set(p) == {"distinct", "equal", "random"} and all(v.size == n for v in p.values())
        assert np.unique(p["distinct"]).size == n and np.unique(p["equal"]).size == 1
        assert p["random"].max() < max(1, n // 4)
        for name in p:
            s = S["one_%d_%s" % (n, name)]
            first = M.run_oracle(s)[0]
            assert first["result"][:4] == (n, s.max_keys, s.max_keys, 0) and s.steps[0].threshold == 2
    big = S["big_exact_fit"]
    assert big.big and big.max_keys == big.steps[0].n == 65537 and -(-65537 // T) > 256      # a second scan chunk
    # the same keys twice: ids kept, before and after chain
    a, b, c = M.run_oracle(S["twice"])
    assert np.array_equal(a["ids"], b["ids"]) and (a["after"] == 1).all() and np.array_equal(b["before"], a["after"])
    assert (b["after"] == 2).all() and b["result"][2] == 0 and b["result"][4] == 300 and (c["after"] == 3).all()
    assert np.array_equal(c["ids"], a["ids"][::-1])
    # disjoint keys number on
    a, b, _ = M.run_oracle(S["disjoint"])
    assert b["ids"].tolist() == list(range(300, 600)) and b["result"][1:3] == (600, 300)
    # new and held keys interleaved, inside a tile and across two tile edges: new ids skip the held leaders
    a, b, _ = M.run_oracle(S["interleaved"])
    ids = b["ids"]
    assert (ids[0:600:2] == np.arange(300)).all()                         # held: even rows below 600
    assert (ids[1:600:2] == 300 + np.arange(300)).all() and (ids[600:] == 600 + np.arange(100)).all()
    assert ids[T - 1] == 300 + (T - 1) // 2 and ids[T] == T // 2 and ids[T + 1] == 300 + T // 2
    assert b["result"][:5] == (700, 700, 400, 0, 300) and b["result"][5] == 300
    # a leader in tile 0 whose other members lie in tile 1
    a, b = M.run_oracle(S["leader_elsewhere"])
    assert a["ids"][280] == a["ids"][290] == a["ids"][5] == 5 and a["after"][290] == 3 and a["crossed"][0] == 5
    assert a["result"][4:] == (1, 1, 3, 5) and b["result"][4:6] == (1, 1) and b["crossed"][0] == 5 and b["after"][5] == 6
    # the stored compare: all 32 bytes, and the scope
    assert sorted(S["stored_byte_%d" % k].steps[1].flips[0][1] for k in range(32)) == list(range(32))
    for name in ["stored_byte_%d" % k for k in range(32)] + ["stored_scope"]:
        s = S[name]
        st = s.steps[1]
        d0, d1 = s.steps[0].digests().reshape(-1, 32), st.digests().reshape(-1, 32)
        if name == "stored_scope":
            assert (d1[0] == d0[3]).all() and st.scope[0] ^ s.steps[0].scope[3] == 1 << 31
        else:
            assert (d1[0] != d0[3]).sum() == 1 and st.scope[0] == s.steps[0].scope[3]
        r = M.run_oracle(s)[1]
        assert r["ids"].tolist() == [65, 3, 10] and r["result"][:3] == (3, 66, 1) and r["crossed"][0] == 1
    # the chain: capacity 64, homes 0 and 63, the map filled exactly in three adds
    for h in (0, 63):
        s = S["chain_home_%d" % h]
        assert s.home == h and s.max_keys == 8 and M.capacity(8) == 64
        res = [r for r in M.run_oracle(s) if r["kind"] == M.ADD]
        assert [r["result"][1] for r in res] == [3, 5, 8] and all(r["result"][3] == 0 for r in res)
        assert [st.kind for st in s.steps] == [M.ADD, M.FIND] * 3
    # full: all or nothing
    r = M.run_oracle(S["full"])
    assert r[0]["result"][:4] == (4, 3, 3, 0)
    assert r[1]["result"] == (4, 3, 2, 1, 0, 0, 0, 0) and (r[1]["ids"] == M.NO_ID).all()
    assert r[1]["before"].tolist() == [0, 1, 0, 1] and r[1]["after"].tolist() == [1, 3, 1, 3]
    assert all(np.array_equal(x, y) for x, y in zip(r[0]["state"], r[1]["state"]))
    assert r[2]["ids"].tolist() == [0, 1, 2, M.NO_ID, M.NO_ID]
    assert r[3]["ids"].tolist() == [3, 1] and r[3]["result"][:4] == (2, 4, 1, 0)
    assert r[4]["result"][:4] == (1, 4, 1, 1) and r[5]["result"][:4] == (3, 4, 0, 0)
    # crossing
    r = M.run_oracle(S["crossing"])
    assert r[0]["result"][4:6] == (2, 2) and r[0]["crossed"][:2].tolist() == [0, 3]          # A and C: 0 -> 3
    assert r[1]["result"][4:6] == (1, 1) and r[1]["crossed"][0] == 2                         # B: 2 -> 3
    assert r[1]["before"].tolist() == [1, 3, 2, 3] and r[1]["after"].tolist() == [2, 5, 3, 5]
    assert r[2]["result"][4] == 0 and S["crossing"].steps[2].threshold == 0
    assert S["crossing"].steps[3].crossed_cap == 0 and r[3]["result"][4:6] == (1, 0) and r[4]["result"][4:6] == (1, 0)
    r = M.run_oracle(S["crossing_cap"])
    assert r[0]["result"][4:6] == (5, 2) and r[0]["crossed"].tolist() == [0, 3]
    assert r[1]["result"][4:6] == (5, 5) and r[1]["crossed"].tolist() == [0, 3, 6, 9, 12]
    r = M.run_oracle(S["crossing_two_tiles"])
    assert r[0]["crossed"].tolist() == [10, 300, M.SENTINEL, M.SENTINEL] and 10 // T != 300 // T
    # optional arrays, clear and reuse, find
    assert all(not st.counts for st in S["no_counts"].steps)
    r = M.run_oracle(S["clear_reuse"])
    assert (r[2]["ids"] == M.NO_ID).all() and r[3]["ids"].tolist() == [0, 1, 2, 0] and r[6]["ids"].tolist() == [0]
    assert r[1]["state"][0].size == 0 and r[5]["state"][0].size == 0
    r = M.run_oracle(S["find"])
    assert (r[0]["ids"] == M.NO_ID).all() and r[2]["ids"].tolist() == [1, M.NO_ID, 0, 0, M.NO_ID]
    assert r[2]["count"].tolist() == [1, 0, 2, 2, 0] and r[3]["count"] is None
    r = M.run_oracle(S["scoped"])
    assert r[0]["result"][:3] == (96, 3, 3) and r[1]["ids"].tolist() == [2, 3, 4, 0] and r[3]["ids"].tolist() == [0, M.NO_ID, 4]


def test_problems_reject_wrong_results():
    S = _by_name()
    assert M.launches() == 7                                               # the sequences are those of dmap.hpp's seven kernels
    want = M.run_oracle(S["interleaved"])[1]
    assert M.problems(want, want) == []
    shifted = dict(want, ids=want["ids"].copy())
    shifted["ids"][want["ids"] >= 300] += 1                                # new ids that did not skip a held leader
    assert any("ids differs" in p for p in M.problems(want, shifted))
    for name in ("before", "after"):
        off = dict(want, **{name: want[name].copy()})
        off[name][17] += 1                                                 # a count off by one
        assert any("%s differs at 17" % name in p for p in M.problems(want, off))
    c = want["crossed"].copy()
    c[[3, 4]] = c[[4, 3]]                                                  # an unsorted crossed list
    assert any("crossed differs at 3" in p for p in M.problems(want, dict(want, crossed=c)))
    capped = M.run_oracle(S["crossing_cap"])[0]
    past = capped["crossed"].copy()
    assert capped["result"][5] == 2 and past.size == 2
    wide = dict(capped, crossed=np.append(past, 6).astype(np.uint32))      # the oracle's list is crossed_cap long ...
    assert any("crossed is missing or of another length" in p for p in M.problems(capped, wide))
    two = M.run_oracle(S["crossing_two_tiles"])[0]
    over = two["crossed"].copy()
    assert over[2] == M.SENTINEL
    over[2] = 301                                                          # ... and a write past listed shows
    assert any("crossed differs at 2" in p for p in M.problems(two, dict(two, crossed=over)))
    assert any("result" in p for p in M.problems(want, dict(want, result=want["result"][:7] + (1,))))
    # a map that changed after full: one count, one key byte, one more entry
    refused = M.run_oracle(S["full"])[1]
    scope, digests, count = refused["state"]
    c2 = count.copy()
    c2[1] += 1
    assert any("state count differs" in p for p in M.problems(refused, dict(refused, state=(scope, digests, c2))))
    d2 = digests.copy()
    d2[2, 31] ^= 1
    assert any("state digests differs" in p for p in M.problems(refused, dict(refused, state=(scope, d2, count))))
    grown = (np.append(scope, 0).astype(np.uint32), np.vstack([digests, digests[:1]]), np.append(count, 1).astype(np.uint32))
    assert any("3 entries expected, got 4" in p for p in M.problems(refused, dict(refused, state=grown)))
    # arrays the step was not given are not looked at
    quiet = M.run_oracle(S["no_counts"])[0]
    assert quiet["before"] is None and M.problems(quiet, dict(quiet, before=np.zeros(1, np.uint32))) == []


def test_probes_and_numbering_under_asan_ubsan(tmp_path):
    seqs = [s for s in M.all_sequences() if not s.big]
    assert len(seqs) == len(M.all_sequences()) - 1
    path, results = str(tmp_path / "sequences.bin"), str(tmp_path / "results.bin")
    M.write_sequences(path, seqs)
    exe = tmp_path / "dmap_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
                    "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "dmap_check.cpp")], check=True)
    r = subprocess.run([str(exe), path, results], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    steps = sum(len(s.steps) for s in seqs)
    assert "units and layout checked" in r.stdout and "dmap ok: %d sequences, %d steps" % (len(seqs), steps) in r.stdout
    got = M.read_results(results, seqs)
    for s, g in zip(seqs, got):
        for k, (want, have) in enumerate(zip(M.run_oracle(s), g)):
            assert M.problems(want, have) == [], (s.name, k)
