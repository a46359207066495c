"""msha_absorb_chain_device on the GPU (mirbft_amd/csrc/kernels.hip k_absorb_chain8): the
eight-lane chain resumed from a state and stopped without padding. Every state is
compared with tests/stream_matrix.py's absorb() -- FIPS 180-4 written out in Python --
and with absorb_device, existing and separately tested code, on a copy of the same
states. Lane counts sit on the consumer-wave (8) and workgroup (16) edges; block counts
cover lanes of nothing, unequal lanes in one workgroup, and the pair path (a workgroup
whose longest lane has 64 blocks or more) with even and odd counts."""
import numpy as np
import pytest

import stream_matrix as S
from mirbft_amd import MshaError
from mirbft_amd import _lib as L

pytestmark = pytest.mark.gpu

NS = (1, 8, 9, 16, 17, 33)


def _patterns(n):
    """name -> blocks per lane."""
    out = {"all1": [1] * n, "all2": [2] * n, "all3": [3] * n, "mixed": [(5 * i + 3) % 6 for i in range(n)]}
    for big in (63, 64, 65, 67):
        b = [1] * n
        b[min(n - 1, 5)] = big
        out["one%d" % big] = b
    return out


def _case(blocks, rng, random_state):
    n = len(blocks)
    off, data, at = [], [], 0
    for b in blocks:
        off.append(at)
        d = rng.bytes(64 * b)
        data.append(d)
        at += 64 * b + 16 * int(rng.integers(0, 3))           # 16-aligned starts, gaps between lanes
    arena = np.frombuffer(b"".join(x + bytes(o2 - o1 - len(x)) for x, o1, o2 in zip(data, off, off[1:] + [at]))
                          + rng.bytes(L.MSHA_DEVICE_ARENA_SLACK), dtype=np.uint8)
    state = (rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32) if random_state
             else np.tile(np.array(S.IV, dtype=np.uint32), (n, 1)))
    want = np.array([S.absorb(state[i].tolist(), data[i]) for i in range(n)], dtype=np.uint32).reshape(n, 8)
    return arena, np.array(off, dtype=np.int64), np.array(blocks, dtype=np.int64), state, want


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda:0")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def matrix():
    """Every (n, pattern, start) cell, built once: inputs and the Python reference."""
    rng = np.random.default_rng(0xAB50)
    cells = {}
    for n in NS:
        for name, blocks in _patterns(n).items():
            for random_state in (False, True):
                cells[(n, name, random_state)] = _case(blocks, rng, random_state)
    return cells


@pytest.mark.parametrize("n", NS)
def test_matrix(engine, matrix, n):
    import torch
    for (cn, name, random_state), (arena, off, nb, state, want) in matrix.items():
        if cn != n:
            continue
        d_arena, d_off, d_nb = _dev(arena), _dev(off), _dev(nb)
        chain, lane = _dev(state), _dev(state)
        torch.cuda.synchronize()
        engine.absorb_chain_device(chain, d_arena, d_off, d_nb)
        engine.absorb_device(lane, d_arena, d_off, d_nb)
        torch.cuda.synchronize()
        engine.device_status()
        got = _words(chain)
        bad = [int(i) for i in np.nonzero((got != want).any(axis=1))[0]]
        assert bad == [], (n, name, random_state, bad[:8], nb[bad[:8]].tolist())
        assert np.array_equal(got, _words(lane)), (n, name, random_state)
        zero = np.nonzero(nb == 0)[0]
        assert np.array_equal(got[zero], state[zero])                  # a lane of no blocks keeps its state


def test_resume(engine):
    """Absorbing k1 then k2 blocks equals absorbing k1 + k2, across the pair path's threshold."""
    import torch
    rng = np.random.default_rng(0xAB51)
    splits = [(1, 1), (2, 3), (63, 1), (1, 63), (64, 3), (40, 41), (0, 5), (5, 0), (65, 66)]
    blocks = [a + b for a, b in splits]
    arena, off, nb, state, want = _case(blocks, rng, True)
    d_arena = _dev(arena)
    k1 = np.array([a for a, _ in splits], dtype=np.int64)
    k2 = np.array([b for _, b in splits], dtype=np.int64)
    # every argument is uploaded first and kept until the device has finished: the calls only
    # enqueue, on the context's stream, and a tensor let go before that is torch's to reuse
    st, whole = _dev(state), _dev(state)
    d_off, d_off2, d_k1, d_k2, d_nb = _dev(off), _dev(off + 64 * k1), _dev(k1), _dev(k2), _dev(nb)
    torch.cuda.synchronize()
    engine.absorb_chain_device(st, d_arena, d_off, d_k1)
    engine.absorb_chain_device(st, d_arena, d_off2, d_k2)
    engine.absorb_chain_device(whole, d_arena, d_off, d_nb)
    torch.cuda.synchronize()
    engine.device_status()
    assert np.array_equal(_words(st), want) and np.array_equal(_words(whole), want)


def test_misaligned_lane(engine):
    import torch
    rng = np.random.default_rng(0xAB52)
    arena, off, nb, state, want = _case([2, 3, 1, 4, 2, 66, 1, 2, 3, 1, 2], rng, True)
    bad = 3
    off = off.copy()
    off[bad] += 8
    st, d = _dev(state), (_dev(arena), _dev(off), _dev(nb))
    torch.cuda.synchronize()
    engine.absorb_chain_device(st, *d)
    torch.cuda.synchronize()
    with pytest.raises(MshaError) as ei:
        engine.device_status()
    assert ei.value.code == L.MSHA_ERR_ALIGNMENT
    engine.device_status()                                              # reported once
    got = _words(st)
    assert np.array_equal(got[bad], state[bad])                         # unchanged
    keep = [i for i in range(len(nb)) if i != bad]
    assert np.array_equal(got[keep], want[keep])                        # the others exact


def test_counters_and_empty_call(engine):
    import torch
    rng = np.random.default_rng(0xAB53)
    arena, off, nb, state, want = _case([2, 1, 3], rng, False)
    st = _dev(state)
    d = (_dev(arena), _dev(off), _dev(nb))
    torch.cuda.synchronize()
    before = engine.stats()
    engine.absorb_chain_device(st, *d)
    torch.cuda.synchronize()
    after = engine.stats()
    moved = {k: after[k] - before[k] for k in after if k.startswith("launches_") and after[k] != before[k]}
    assert moved == {"launches_coop": 1, "launches_chain8": 1}
    assert np.array_equal(_words(st), want)
    # n == 0 launches nothing (and reads no pointer)
    empty = torch.empty(0, dtype=torch.int64, device="cuda:0")
    engine.absorb_chain_device(torch.empty((0, 8), dtype=torch.int32, device="cuda:0"), d[0], empty, empty)
    assert L.lib().msha_absorb_chain_device(engine._ctx, None, None, None, None, 0, None) == L.MSHA_OK
    again = engine.stats()
    assert all(again[k] == after[k] for k in after if k.startswith("launches_"))
    engine.device_status()


def test_capture_and_two_replays(engine):
    import torch
    rng = np.random.default_rng(0xAB54)
    blocks = [3, 1, 70, 2, 5, 1, 1, 2, 9]
    arena, off, nb, state, want1 = _case(blocks, rng, True)
    data = [arena[int(o): int(o) + 64 * b].tobytes() for o, b in zip(off, blocks)]

    def want(times):
        h = [state[i].tolist() for i in range(len(blocks))]
        for _ in range(times):
            h = [S.absorb(h[i], data[i]) for i in range(len(blocks))]
        return np.array(h, dtype=np.uint32)

    st = _dev(state)
    d = (_dev(arena), _dev(off), _dev(nb))
    torch.cuda.synchronize()
    engine.absorb_chain_device(st, *d)                                  # the context's first device call is not captured
    torch.cuda.synchronize()
    assert np.array_equal(_words(st), want(1))
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            engine.absorb_chain_device(st, *d, stream=s)
        finally:
            g.capture_end()
    torch.cuda.synchronize()
    assert np.array_equal(_words(st), want(1))                          # the capture itself ran nothing
    for times in (2, 3):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_words(st), want(times)), times
    engine.device_status()
    del g
