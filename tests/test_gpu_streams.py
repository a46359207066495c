"""Stream sets on the GPU (include/mirsha.h "Stream sets"): resumable batched SHA-256
with hash.Hash semantics. Every expected digest comes from hashlib; the exported
chaining states are checked against a FIPS 180-4 compression function carried in
tests/stream_matrix.py (hashlib exposes no midstate)."""
import hashlib
import random
import struct

import numpy as np
import pytest

from mirbft_amd import GPUHasher, MshaError, StreamSet
from mirbft_amd import _lib as L
from stream_matrix import IV as _IV, midstate as _midstate

gpu = pytest.mark.gpu


def _sha(b) -> bytes:
    return hashlib.sha256(bytes(b)).digest()


def _rows(digests) -> list:
    return [bytes(r) for r in digests]


# -- FIPS 180-4 section 6.2.2, for the midstate checks: carried in tests/stream_matrix.py --
def test_the_carried_compression_function_is_sha256():
    """The test's own reference: padding by hand + _compress equals hashlib."""
    for n in (0, 3, 55, 56, 64, 200):
        m = bytes(range(256))[:n] if n <= 256 else b""
        padded = m + b"\x80" + b"\x00" * ((55 - n) % 64) + struct.pack(">Q", 8 * n)
        assert struct.pack(">8I", *_midstate(padded)) == _sha(m)


# -- 3. boundary matrix ----------------------------------------------------------------
_N = 229          # 3 waves + 37 lanes
_CUT_KINDS = ("zero", "in_first", "mult64", "r55", "r56", "r63", "r64", "r65")


def _bounds(total: int, s: int, rnd: random.Random, used: set) -> list:
    """Write boundaries [0, c1, c2, c3, total] of a message cut into 1-4 writes
    (fewer writes: trailing empty ones)."""
    q = rnd.randrange(0, 6)
    cand = {"zero": 0, "in_first": rnd.randrange(1, 64), "mult64": 64 * rnd.randrange(1, 7), "r55": 64 * q + 55,
            "r56": 64 * q + 56, "r63": 64 * q + 63, "r64": 64 * q + 64, "r65": 64 * q + 65}
    writes = 1 + s % 4
    picks = [_CUT_KINDS[(s // 4 + 3 * j) % len(_CUT_KINDS)] for j in range(writes - 1)]
    cuts = []
    for k in picks:
        if cand[k] <= total:
            used.add(k)
        cuts.append(min(cand[k], total))
    b = [0] + sorted(cuts) + [total]
    return b + [total] * (5 - len(b))


@gpu
def test_boundary_matrix_229_streams(engine):
    rnd = random.Random(3)
    totals = list(range(384)) + [1000, 4151]
    totals += [64, 128, 55, 56, 119, 120, 191, 192] * 9        # fill the second pass
    totals = totals[:2 * _N]
    assert set(range(384)) | {1000, 4151} <= set(totals)
    used = set()
    ids = np.arange(_N, dtype=np.uint64)
    with StreamSet(engine, _N) as ss:
        for p in range(2):
            msgs = [rnd.randbytes(t) for t in totals[p * _N:(p + 1) * _N]]
            bounds = [_bounds(len(m), s, rnd, used) for s, m in enumerate(msgs)]
            for r in range(4):
                ss.write(ids, [m[b[r]:b[r + 1]] for m, b in zip(msgs, bounds)])
                exp = [_sha(m[:b[r + 1]]) for m, b in zip(msgs, bounds)]
                got = ss.sum()
                assert got.shape == (_N, 32) and _rows(got) == exp, (p, r)
                assert _rows(ss.sum()) == exp, (p, r, "a second sum")       # Sum changes nothing
                assert ss.lengths().tolist() == [b[r + 1] for b in bounds]
            assert _rows(ss.sum()) == [_sha(m) for m in msgs]
            ss.reset()
            assert _rows(ss.sum()) == [_sha(b"")] * _N and not ss.lengths().any()
    assert used == set(_CUT_KINDS), set(_CUT_KINDS) - used


# -- 4. repeated ids ---------------------------------------------------------------------
@gpu
def test_repeated_ids_in_one_call(engine):
    rnd = random.Random(4)
    n = 50
    ids, chunks = [], []
    whole = [b""] * n
    for j in range(41):
        for s, c in ((5, rnd.randbytes(32)), (6 + j, rnd.randbytes(rnd.randrange(0, 200)))):
            ids.append(s)
            chunks.append(c)
            whole[s] += c
    with StreamSet(engine, n) as ss:
        ss.write(ids, chunks)
        assert len(whole[5]) == 41 * 32
        assert _rows(ss.sum()) == [_sha(w) for w in whole]
        assert ss.lengths().tolist() == [len(w) for w in whole]
        assert ss.lengths([5, 0, 46]).tolist() == [41 * 32, 0, len(whole[46])]
        # the hash.Hash view of one stream
        h = ss.stream(5)
        assert h.size == 32 and h.block_size == 64
        assert h.sum(b"ab") == b"ab" + _sha(whole[5])
        assert h.write(b"xyz") == 3 and h.sum() == _sha(whole[5] + b"xyz")
        h.reset()
        assert h.sum() == _sha(b"")


# -- 5. NodeState chain ------------------------------------------------------------------
@gpu
def test_nodestate_chain_through_a_4_stream_set(engine):
    """tests/test_gpu_checkpoint.py's scenario, streamed: every committed digest is
    written as it arrives (Apply), Snap is sum, then reset + write(prev)."""
    rnd = random.Random(11)
    nodes = 4
    ref = [hashlib.sha256() for _ in range(nodes)]
    with GPUHasher(engine).new_streams(nodes) as ss:
        for interval in range(20):
            committed = [[_sha(b"%d-%d-%d" % (n, interval, j)) for j in range(rnd.randrange(0, 41))]
                         for n in range(nodes)]
            for j in range(max(len(c) for c in committed)):
                live = [n for n in range(nodes) if j < len(committed[n])]
                ss.write(live, [committed[n][j] for n in live])          # Apply
            for n in range(nodes):
                for d in committed[n]:
                    ref[n].update(d)
            exp = [r.digest() for r in ref]
            assert _rows(ss.sum()) == exp, interval                          # Snap: Sum(nil)
            ss.reset()
            ss.write(list(range(nodes)), exp)                                # New + Write(CheckpointHash)
            ref = [hashlib.sha256(e) for e in exp]


# -- 6. buffered-only writes -----------------------------------------------------------
@gpu
def test_buffered_only_writes_launch_nothing(engine):
    rnd = random.Random(6)
    with StreamSet(engine, 10) as ss:
        whole = [b""] * 10
        ss.write([0], [rnd.randbytes(70)])          # one real launch first
        whole[0] = None
        before = ss.stats()
        assert before["launches_absorb"] == 1 and before["buffered_only_writes"] == 0
        for _ in range(3):
            ids = [1, 2, 3, 2]
            chunks = [rnd.randbytes(rnd.randrange(0, 16)) for _ in ids]
            ss.write(ids, chunks)
            for s, c in zip(ids, chunks):
                whole[s] += c
        ss.write([], [])
        after = ss.stats()
        assert after["launches_absorb"] == before["launches_absorb"]
        assert after["buffered_only_writes"] == before["buffered_only_writes"] + 4
        assert after["writes"] == before["writes"] + 4 and after["pieces"] == before["pieces"]
        assert max(len(w) for w in whole[1:]) < 64
        assert _rows(ss.sum(list(range(1, 10)))) == [_sha(w) for w in whole[1:]]


# -- 7. load modes -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool():
    return np.random.default_rng(7).integers(0, 256, 1 << 16, dtype=np.uint8)


def _mode_case(engine, pool, n, want_mode):
    rng = np.random.default_rng(n)
    nb = 1 + (np.arange(n, dtype=np.uint64) + rng.integers(0, 5, n).astype(np.uint64)) % 5   # 1..5 blocks
    off = rng.integers(0, pool.size - 320, n).astype(np.uint64)
    ids = np.arange(n, dtype=np.uint64)
    with StreamSet(engine, n, staging_bytes=int(n) * 320) as ss:
        ss.write_packed(pool, ids, off, nb * 64)
        st = ss.stats()
        assert st["launches_absorb"] == 1 and st["pieces"] == 1 and st["last_lanes"] == n
        assert st["last_load_mode"] == want_mode, st
        assert st["blocks_absorbed"] == int(nb.sum())
        got = ss.sum()
        assert ss.stats()["last_load_mode"] == want_mode
    raw = pool.tobytes()
    exp = [_sha(raw[o:o + 64 * b]) for o, b in zip(off.tolist(), nb.tolist())]
    assert set(nb.tolist()) == {1, 2, 3, 4, 5}
    bad = [i for i in range(n) if bytes(got[i]) != exp[i]]
    assert not bad, (len(bad), bad[:5])


@gpu
def test_load_mode_prefetch_below_three_waves_a_simd(engine, pool):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _mode_case(engine, pool, cus * 256 - 27, 1)


@gpu
def test_load_mode_paired_from_three_waves_a_simd(engine, pool):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _mode_case(engine, pool, cus * 768 + 37, 2)


@gpu
def test_load_mode_small_end_130_lanes(engine, pool):
    _mode_case(engine, pool, 130, 1)


# -- 8. pieces -----------------------------------------------------------------------------
@gpu
def test_a_write_larger_than_the_staging_runs_in_pieces(engine):
    rnd = random.Random(8)
    with StreamSet(engine, 5, staging_bytes=4096) as ss:
        first = [rnd.randbytes(k) for k in (17, 0, 63, 100, 64)]
        ss.write(range(5), first)
        p0 = ss.stats()["pieces"]
        second = [rnd.randbytes(k) for k in (130, 10_000, 1, 700, 31)]
        ss.write([0, 1, 2, 3, 4], second)
        st = ss.stats()
        assert st["pieces"] - p0 >= 3, st
        assert _rows(ss.sum()) == [_sha(a + b) for a, b in zip(first, second)]
        assert ss.lengths().tolist() == [len(a) + len(b) for a, b in zip(first, second)]


# -- 9. atomic validation -----------------------------------------------------------------
@gpu
def test_a_bad_write_changes_no_stream(engine):
    rnd = random.Random(9)
    n = 6
    with StreamSet(engine, n) as ss:
        base = [rnd.randbytes(k) for k in (0, 5, 64, 100, 63, 129)]
        ss.write(range(n), base)
        sums, lens = _rows(ss.sum()), ss.lengths().tolist()
        with pytest.raises(MshaError) as ei:        # the third job names id n
            ss.write([0, 1, n, 2, 3], [rnd.randbytes(80) for _ in range(5)])
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG
        assert _rows(ss.sum()) == sums and ss.lengths().tolist() == lens
        arena = np.frombuffer(rnd.randbytes(256), dtype=np.uint8)
        with pytest.raises(MshaError) as ei:        # the second range leaves the arena
            ss.write_packed(arena, np.array([0, 1, 2]), np.array([0, 200, 0]), np.array([100, 57, 100]))
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG
        assert _rows(ss.sum()) == sums and ss.lengths().tolist() == lens
        assert sums == [_sha(b) for b in base]
        ss.write([5], [b"!"])                        # and the set goes on working
        assert bytes(ss.sum([5])[0]) == _sha(base[5] + b"!")


# -- 10. export / import -------------------------------------------------------------------
@gpu
def test_export_layout_and_import_into_another_set(engine):
    rnd = random.Random(10)
    lens = [128 + 0, 64 + 1, 192 + 55, 63, 0, 640 + 63]        # residues 0, 1, 55, 63 (and a fresh stream)
    msgs = [rnd.randbytes(k) for k in lens]
    with StreamSet(engine, len(msgs)) as a, StreamSet(engine, 16) as b:
        a.write(range(len(msgs)), msgs)
        blob = a.export_state()
        assert blob.shape == (len(msgs), 108)
        for m, row in zip(msgs, blob):
            raw = bytes(row)
            r = len(m) % 64
            assert raw[:4] == b"sha\x03"
            assert struct.unpack(">Q", raw[100:108])[0] == len(m)
            assert raw[36:36 + r] == m[len(m) - r:] and raw[36 + r:100] == bytes(64 - r)
            assert list(struct.unpack(">8I", raw[4:36])) == _midstate(m), len(m)
        assert bytes(a.export_state([3])[0]) == bytes(blob[3])
        # into other ids of a second set, then on from there
        to = [9, 2, 15, 0, 7, 4]
        b.write([9, 1], [b"overwritten by the import", b"untouched"])
        noisy = blob.copy()
        for row, m in zip(noisy, msgs):
            row[36 + len(m) % 64:100] = 0xAB        # buffer bytes past length % 64 are ignored
        b.import_state(to, noisy)
        assert b.lengths(to).tolist() == lens
        assert _rows(b.sum(to)) == [_sha(m) for m in msgs]
        more = [rnd.randbytes(k) for k in (1, 63, 9, 200, 64, 0)]
        b.write(to, more)
        assert _rows(b.sum(to)) == [_sha(m + x) for m, x in zip(msgs, more)]
        assert bytes(b.sum([1])[0]) == _sha(b"untouched")
        with pytest.raises(MshaError) as ei:        # a wrong magic changes nothing
            b.import_state([1], b"shb\x03" + bytes(104))
        assert ei.value.code == L.MSHA_ERR_INVALID_ARG and bytes(b.sum([1])[0]) == _sha(b"untouched")


# -- 11. device forms ------------------------------------------------------------------------
@gpu
def test_device_forms_absorb_then_finish(engine):
    import torch
    dev = torch.device("cuda:0")
    n = 64 * 5 - 27
    rng = np.random.default_rng(11)
    lens = np.arange(n, dtype=np.int64)                                   # 0 .. 292
    off = np.concatenate([[0], np.cumsum((lens + 15) // 16 * 16)[:-1]]).astype(np.int64)
    arena = rng.integers(0, 256, int(off[-1] + lens[-1]) + 64, dtype=np.uint8)   # + the slack
    raw = arena.tobytes()
    exp = [_sha(raw[o:o + k]) for o, k in zip(off.tolist(), lens.tolist())]
    d_arena = torch.from_numpy(arena).to(dev)
    d_off, d_len = torch.from_numpy(off).to(dev), torch.from_numpy(lens).to(dev)

    def fresh_out():
        # (torch works on the null stream, the engine on its own: order them here)
        t = torch.full((n, 32), 0x5A, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        return t

    # finish from the initial value with no prefix is a whole-message hash
    out, out2 = fresh_out(), fresh_out()
    engine.finish_device(None, None, d_arena, d_off, d_len, out)
    engine.digest_batch_device(d_arena, d_off, d_len, out2)
    engine.device_status()
    assert _rows(out.cpu().numpy()) == exp
    assert torch.equal(out, out2)

    # absorb the whole blocks, then finish the rest with the prefix
    iv = np.tile(np.array(_IV, dtype=np.uint32), (n, 1)).view(np.int32)
    state = torch.from_numpy(iv.copy()).to(dev)
    nblocks = lens // 64
    prefix = nblocks * 64
    d_nblocks, d_prefix = torch.from_numpy(nblocks).to(dev), torch.from_numpy(prefix).to(dev)
    d_off2, d_len2 = torch.from_numpy(off + prefix).to(dev), torch.from_numpy(lens - prefix).to(dev)
    out = fresh_out()
    engine.absorb_device(state, d_arena, d_off, d_nblocks)
    engine.finish_device(state, d_prefix, d_arena, d_off2, d_len2, out)
    engine.device_status()
    assert _rows(out.cpu().numpy()) == exp
    got_state = state.cpu().numpy().view(np.uint32)
    for i in (0, 63, 64, 127, 128, 292):
        assert got_state[i].tolist() == _midstate(raw[off[i]:off[i] + lens[i]]), i

    # a misaligned start: reported, that state unchanged (absorb) / that digest zero (finish)
    bad = 200                                                              # 3 whole blocks
    off_bad = off.copy()
    off_bad[bad] += 8
    state = torch.from_numpy(iv.copy()).to(dev)
    d_off_bad = torch.from_numpy(off_bad).to(dev)
    torch.cuda.synchronize()
    engine.absorb_device(state, d_arena, d_off_bad, d_nblocks)
    with pytest.raises(MshaError) as ei:
        engine.device_status()
    assert ei.value.code == L.MSHA_ERR_ALIGNMENT
    after = state.cpu().numpy().view(np.uint32)
    assert after[bad].tolist() == _IV
    assert after[bad + 1].tolist() == got_state[bad + 1].tolist() and after[bad - 1].tolist() == got_state[bad - 1].tolist()
    out = fresh_out()
    engine.finish_device(None, None, d_arena, d_off_bad, d_len, out)
    with pytest.raises(MshaError) as ei:
        engine.device_status()
    assert ei.value.code == L.MSHA_ERR_ALIGNMENT
    res = _rows(out.cpu().numpy())
    assert res[bad] == bytes(32)
    assert res[:bad] == exp[:bad] and res[bad + 1:] == exp[bad + 1:]
    engine.device_status()                                                 # the flag was cleared
