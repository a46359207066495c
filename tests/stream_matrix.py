"""Stream kernel matrix: reference, case builders and runner (not collected by pytest).

The resume kernels of mirbft_amd/csrc/stream_kernels.hip restate hash_message's
block loop: three load modes and, under kPair, their own decision on which load
holds the tail block (prefetched with the pair before it for an odd count of whole
blocks, loaded alone for an even one). This module aims at them what
tests/kernel_matrix.py aims at kernels.hip:

  finish cells  (r class, nfull class, prefix and state, wave kind)
  absorb cells  (block-count class, state, wave kind)

from LENGTH PATTERNS over tail lengths 0..383 (every r = len % 64 with nfull =
len // 64 from 0 to 5) plus 1000 and 4151. tests/test_stream_matrix_cpu.py checks
from the lengths alone that the patterns hit every cell, and that the reference
below agrees with hashlib; tests/test_gpu_stream_matrix.py runs the cases.

The reference is FIPS 180-4's compression function carried here (hashlib exposes
no chaining state): midstate() for absorbed states, resume_digest() for a digest
continued from a state -- with a 64-bit bit length taken mod 2^64, as Go
crypto/sha256's `len <<= 3` on a uint64 and the kernels' `len * 8` do. Where a
lane's message is one hashlib can express (from the initial value, prefix 0) the
expected digest is hashlib's; the CPU test proves the two agree. The natural kPair
case (some 200,000 lanes) takes hashlib for every lane: a resumed lane's digest is
its whole message's.

`python tests/stream_matrix.py --child` runs, in a process of its own, the
device-form matrix and a stream-set pass under the MSHA_LOAD_MODE of its
environment (read once per process by the library), one JSON line per case.

No GPU code here; torch is imported only when a case runs.
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import random
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WAVE = 64
PARTIAL_LANES = 37                  # every lane count is 64 k + 37
N_SMALL = 64 * 6 + PARTIAL_LANES    # 421: the device-form matrix


# ---------------------------------------------------------------------------
# FIPS 180-4 section 6.2.2
# ---------------------------------------------------------------------------
K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
    0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
    0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
    0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
    0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
    0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
    0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
M32 = 0xFFFFFFFF


def rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def compress(h, block):
    w = list(struct.unpack(">16I", block))
    for i in range(16, 64):
        s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M32)
    a, b, c, d, e, f, g, hh = h
    for i in range(64):
        t1 = (hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g & M32)) + K[i] + w[i]) & M32
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        hh, g, f, e, d, c, b, a = g, f, e, (d + t1) & M32, c, b, a, (t1 + t2) & M32
    return [(x + y) & M32 for x, y in zip(h, (a, b, c, d, e, f, g, hh))]


def absorb(state_words, data: bytes) -> list:
    """state_words after the whole 64-byte blocks of data (a rest under 64 bytes is ignored)."""
    h = list(state_words)
    for b in range(len(data) // 64):
        h = compress(h, data[64 * b:64 * b + 64])
    return h


def midstate(msg: bytes) -> list:
    """The chaining state after msg's whole blocks, from the initial value."""
    return absorb(IV, msg)


def resume_digest(state_words, tail_bytes, total_len: int) -> bytes:
    """The digest of a message of total_len bytes whose first total_len -
    len(tail_bytes) bytes (a multiple of 64) are already folded into state_words:
    tail_bytes padded by hand, the bit length (8 total_len) mod 2^64."""
    tail = bytes(tail_bytes)
    padded = tail + b"\x80" + b"\x00" * ((55 - len(tail)) % 64) + struct.pack(">Q", (8 * total_len) & (2 ** 64 - 1))
    assert len(padded) % 64 == 0
    return struct.pack(">8I", *absorb(state_words, padded))


def sha(b) -> bytes:
    return hashlib.sha256(bytes(b)).digest()


# ---------------------------------------------------------------------------
# The launchers' choice of load mode, restated (kernels.hpp pick_mode,
# stream_kernels.hip stream_mode)
# ---------------------------------------------------------------------------
MODE_NAMES = ("kSingle", "kPrefetch", "kPair", "kPipe")


def pick_mode(n, cus, forced=-1):
    """kernels.hpp pick_mode(): 0 kSingle, 1 kPrefetch, 2 kPair, 3 kPipe."""
    if 0 <= forced <= 3:
        return forced
    if n <= cus * 4 * 64:
        return 3
    return 1 if n < cus * 4 * 64 * 3 else 2


def stream_mode(n, cus, forced=-1):
    """stream_kernels.hip stream_mode(): pick_mode, its kPipe run as kPrefetch."""
    m = pick_mode(n, cus, forced)
    return 1 if m == 3 else m


def pair_n(cus):
    """The lane count of the natural kPair case (tests/test_gpu_streams.py's)."""
    return 768 * cus + PARTIAL_LANES


# ---------------------------------------------------------------------------
# Cells
# ---------------------------------------------------------------------------
R_CLASSES = ("r0", "r1_55", "r56_63")
NFULL_CLASSES = ("nfull0", "nfull_odd", "nfull_even")
STATE_KINDS = ("iv", "null", "resumed")     # (prefix 0, IV rows), (prefix 0, state NULL), (prefix 64 q, absorbed)
WAVE_KINDS = ("uniform", "ragged", "partial")
NB_CLASSES = ("nb0", "nb1", "nb2", "nb_odd", "nb_even")
ABSORB_STATES = ("iv", "carried")

FINISH_CELLS = set(itertools.product(R_CLASSES, NFULL_CLASSES, STATE_KINDS, WAVE_KINDS))
ABSORB_CELLS = set(itertools.product(NB_CLASSES, ABSORB_STATES, WAVE_KINDS))


def r_class(t):
    r = int(t) % 64
    return R_CLASSES[0 if r == 0 else (1 if r < 56 else 2)]


def nfull_class(t):
    nfull = int(t) // 64
    return NFULL_CLASSES[0 if nfull == 0 else (1 if nfull % 2 else 2)]


def nb_class(nb):
    nb = int(nb)
    return NB_CLASSES[nb] if nb <= 2 else NB_CLASSES[3 if nb % 2 else 4]


def wave_kind_of(values, start):
    """Kind of the wave values[start : start + 64]: the partial last wave, a whole
    wave of one value, a whole wave of several."""
    w = values[start:start + WAVE]
    if len(w) < WAVE:
        return "partial"
    return "uniform" if (w == w[0]).all() else "ragged"


def finish_cells(tails, kinds):
    """{(r class, nfull class, state kind, wave kind)} over the lanes; the wave kind
    is decided by the tail lengths (they alone steer the kernel's loop)."""
    tails = np.asarray(tails)
    cells = set()
    for s in range(0, len(tails), WAVE):
        wk = wave_kind_of(tails, s)
        for i in range(s, min(s + WAVE, len(tails))):
            cells.add((r_class(tails[i]), nfull_class(tails[i]), kinds[i], wk))
    return cells


def absorb_cells(nb, carried):
    """{(block-count class, state, wave kind)} over the lanes of one absorb launch;
    carried[i]: lane i's state came from an earlier absorb of at least one block."""
    nb = np.asarray(nb)
    cells = set()
    for s in range(0, len(nb), WAVE):
        wk = wave_kind_of(nb, s)
        for i in range(s, min(s + WAVE, len(nb))):
            cells.add((nb_class(nb[i]), "carried" if carried[i] else "iv", wk))
    return cells


# ---------------------------------------------------------------------------
# Length patterns
# ---------------------------------------------------------------------------
TAILS = np.array(list(range(384)) + [1000, 4151], dtype=np.int64)
# One whole wave each: every (r class, nfull class), then 1000, 4151 and 63. A launch
# of six whole waves sees the first six walking up and the last six walking down.
UNIFORM_TAILS = (0, 37, 56, 64, 119, 255, 128, 129, 312, 1000, 4151, 63)
# The partial last wave of uniform_up: every (r class, nfull class) at its edges
PARTIAL_TAILS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 183, 184, 191, 192, 247, 248, 255,
                 256, 257, 311, 312, 319, 320, 321, 375, 376, 383, 1000, 4151, 448, 512, 17, 100, 200, 300)
PAIR_PARTIAL_TAILS = (0, 37, 60, 64, 119, 255, 128, 129, 312)     # one of every (r class, nfull class)
FINISH_PATTERNS = ("uniform_up", "uniform_down", "ragged")


def finish_tails(pattern, n=N_SMALL):
    """The tail length (d_len) of every lane."""
    assert n % WAVE == PARTIAL_LANES and len(PARTIAL_TAILS) == PARTIAL_LANES
    i = np.arange(n, dtype=np.int64)
    if pattern == "ragged":
        # 199 is coprime to 386: the 64 lanes of a wave all differ, 386 lanes see all of TAILS
        return TAILS[(i * 199) % len(TAILS)].copy()
    u = np.array(UNIFORM_TAILS, dtype=np.int64)
    k = (i // WAVE) % len(u)
    if pattern == "uniform_up":
        t = u[k]
        t[n - PARTIAL_LANES:] = PARTIAL_TAILS
        return t
    if pattern == "uniform_down":
        t = u[len(u) - 1 - k]
        t[n - PARTIAL_LANES:] = 56
        return t
    if pattern == "pair":
        # the natural kPair launch: three ragged waves cycling 0..383, then a whole
        # wave of one length (UNIFORM_TAILS first, then 0..383 upward); the partial
        # last wave: PAIR_PARTIAL_TAILS, each twice (a lane from the IV, a resumed one)
        t = ((i * 7919) % 384).astype(np.int64)
        w = i // WAVE
        g = w // 4
        ut = np.where(g < len(u), u[g % len(u)], (g - len(u)) % 384)
        uni = (w % 4 == 3) & (i < n - PARTIAL_LANES)
        t[uni] = ut[uni]
        j = np.arange(PARTIAL_LANES)
        t[n - PARTIAL_LANES:] = np.array(PAIR_PARTIAL_TAILS, dtype=np.int64)[(j // 2) % len(PAIR_PARTIAL_TAILS)]
        return t
    raise KeyError(pattern)


def resume_blocks(n, kind):
    """q[i]: the whole blocks of lane i's message absorbed before the finish (its
    prefix is 64 q). Resumed lanes: 1..3, varying per lane."""
    i = np.arange(n, dtype=np.int64)
    if kind == "resumed":
        return 1 + i % 3
    if kind == "third":
        # the natural kPair launch: one third of the lanes resumed, the choice moving
        # on by one lane with every 384 (the period of that pattern's ragged tails), so
        # that every tail length meets it; in the partial last wave every other lane
        q = np.where((i + i // 384) % 3 == 2, 1 + (i // 7) % 3, 0)
        j = np.arange(PARTIAL_LANES)
        q[n - PARTIAL_LANES:] = np.where(j % 2 == 1, 1 + (j // 2) % 3, 0)
        return q
    return np.zeros(n, dtype=np.int64)


def finish_cases():
    """(pattern, state kind) of every device-form finish case at N_SMALL lanes."""
    return [(p, k) for p in FINISH_PATTERNS for k in STATE_KINDS]


def finish_case_cells(pattern, kind, n=N_SMALL):
    tails = finish_tails(pattern, n)
    if kind == "third":
        kinds = np.where(resume_blocks(n, kind) > 0, "resumed", "iv")
    else:
        kinds = np.full(n, kind)
    return finish_cells(tails, kinds.tolist())


ABSORB_PATTERNS = ("uniform", "ragged")
# uniform: wave k absorbs _NB_FIRST[k] blocks from the IV, then _NB_SECOND[k]: waves
# 0..4 carry a state into every class of the second count, wave 5 meets it fresh
_NB_FIRST = (1, 2, 3, 4, 7, 0)
_NB_SECOND = (0, 1, 2, 3, 4, 7)


def absorb_blocks(pattern, n=N_SMALL):
    """(first, second): the block counts of two absorb launches over the same states."""
    i = np.arange(n, dtype=np.int64)
    if pattern == "uniform":
        k = (i // WAVE) % len(_NB_FIRST)
        a, b = np.array(_NB_FIRST, dtype=np.int64)[k], np.array(_NB_SECOND, dtype=np.int64)[k]
        a[n - PARTIAL_LANES:] = 5
        b[n - PARTIAL_LANES:] = 6
        return a, b
    if pattern == "ragged":
        return (i * 5) % 8, (i * 3 + i // 8) % 8
    raise KeyError(pattern)


def absorb_case_cells(pattern, n=N_SMALL):
    a, b = absorb_blocks(pattern, n)
    return absorb_cells(a, np.zeros(n, dtype=bool)) | absorb_cells(b, a > 0)


# ---------------------------------------------------------------------------
# Write cuts of the stream-set passes (tests/test_gpu_streams.py's boundary kinds)
# ---------------------------------------------------------------------------
CUT_KINDS = ("zero", "in_first", "mult64", "r55", "r56", "r63", "r64", "r65")


def cut_bounds(total, s, rnd, used):
    """Write boundaries [0, c1, c2, c3, total] of a message cut into 1 to 4 writes
    (fewer writes: trailing empty ones) at CUT_KINDS boundaries; `used` collects the
    kinds that fell inside the message."""
    q = rnd.randrange(0, 6)
    cand = {"zero": 0, "in_first": rnd.randrange(1, 64), "mult64": 64 * rnd.randrange(1, 7), "r55": 64 * q + 55,
            "r56": 64 * q + 56, "r63": 64 * q + 63, "r64": 64 * q + 64, "r65": 64 * q + 65}
    writes = 1 + s % 4
    picks = [CUT_KINDS[(s // 4 + 3 * j) % len(CUT_KINDS)] for j in range(writes - 1)]
    cuts = []
    for k in picks:
        if cand[k] <= total:
            used.add(k)
        cuts.append(min(cand[k], total))
    b = [0] + sorted(cuts) + [total]
    return b + [total] * (5 - len(b))


def set_pass_inputs(n, seed):
    """n messages over TAILS (all of them when n >= 386) and their write bounds."""
    rnd = random.Random(seed)
    totals = [int(TAILS[(i * 199) % len(TAILS)]) for i in range(n)]
    msgs = [rnd.randbytes(t) for t in totals]
    used = set()
    bounds = [cut_bounds(len(m), s, rnd, used) for s, m in enumerate(msgs)]
    return msgs, bounds, used


# ---------------------------------------------------------------------------
# Inputs, expectations, failure messages
# ---------------------------------------------------------------------------
def _seed(*what):
    return zlib.crc32(repr(what).encode())


def build_arena(lens, seed):
    """Random bytes: message i at a 64-byte aligned offset, 64 bytes of slack after
    the last (the kernels read the block after a lane's last whole one)."""
    lens = np.asarray(lens, dtype=np.int64)
    stride = (lens + 63) // 64 * 64
    off = np.zeros(len(lens), dtype=np.int64)
    off[1:] = np.cumsum(stride)[:-1]
    arena = np.random.default_rng(seed).integers(0, 256, int(stride.sum()) + 64, dtype=np.uint8)
    return arena, off


def mismatch(what, mode, tails, prefix, got, exp):
    """None when equal; else the case, how many lanes differ and, for the first few,
    the lane, its tail length, nfull, r, prefix and the load mode of the launch."""
    got, exp = np.asarray(got), np.asarray(exp)
    bad = np.nonzero(np.any(got != exp, axis=1))[0]
    if bad.size == 0:
        return None
    first = [{"lane": int(i), "wave": int(i) // WAVE, "lane_in_wave": int(i) % WAVE, "tail_len": int(tails[i]),
              "nfull": int(tails[i]) // 64, "r": int(tails[i]) % 64, "prefix": int(prefix[i]),
              "load_mode": MODE_NAMES[mode], "got": bytes(got[i]).hex(), "want": bytes(exp[i]).hex()}
             for i in bad[:6]]
    return {"what": what, "bad": int(bad.size), "of": int(len(tails)), "first": first}


def state_mismatch(what, mode, nb, got, exp):
    """As mismatch(), for absorbed states (rows of eight words)."""
    got, exp = np.asarray(got), np.asarray(exp)
    bad = np.nonzero(np.any(got != exp, axis=1))[0]
    if bad.size == 0:
        return None
    first = [{"lane": int(i), "wave": int(i) // WAVE, "lane_in_wave": int(i) % WAVE, "nblocks": int(nb[i]),
              "load_mode": MODE_NAMES[mode], "got": [int(x) for x in got[i]], "want": [int(x) for x in exp[i]]}
             for i in bad[:6]]
    return {"what": what, "bad": int(bad.size), "of": int(len(nb)), "first": first}


def _digest_rows(digests):
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32)


def expected_finish(raw, off, q, tails, states=None):
    """Row i: the digest of raw[off[i] : off[i] + 64 q[i] + tails[i]]. With `states`
    (the expected absorbed state of every lane) a resumed lane's digest is
    resume_digest from that state; every other one is hashlib's."""
    out = []
    for i, (o, k, t) in enumerate(zip(off.tolist(), q.tolist(), tails.tolist())):
        if states is not None and k:
            out.append(resume_digest(states[i], raw[o + 64 * k:o + 64 * k + t], 64 * k + t))
        else:
            out.append(sha(raw[o:o + 64 * k + t]))
    return _digest_rows(out)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _iv_rows(n):
    return np.tile(np.array(IV, dtype=np.uint32), (n, 1))


SENTINEL = 0xA5


def run_finish_case(eng, pattern, kind, n, mode, check_states=True):
    """One finish case through Engine.absorb_device / finish_device -> a list of
    mismatches (empty: every digest and every absorbed state is right). The output
    is pre-filled with a sentinel; device_status() must come back clean."""
    import torch
    what = "finish %s / %s (n = %d)" % (pattern, kind, n)
    tails, q = finish_tails(pattern, n), resume_blocks(n, kind)
    arena, off = build_arena(64 * q + tails, _seed("finish", pattern, kind))
    raw = arena.tobytes()
    prefix = 64 * q
    states = None
    if check_states:
        states = [midstate(raw[o:o + 64 * k]) for o, k in zip(off.tolist(), q.tolist())]
    exp = expected_finish(raw, off, q, tails, states)
    # every tensor exists before the first launch and lives until device_status() has
    # synchronised: torch works on the null stream, the engine on its own
    d_arena, d_off, d_len = _dev(arena), _dev(off + prefix), _dev(tails)
    d_off0, d_q, d_prefix, state = _dev(off), _dev(q), _dev(prefix), _dev(_iv_rows(n).view(np.int32))
    out = torch.full((n, 32), SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    bad = []
    if kind == "null":
        eng.finish_device(None, None, d_arena, d_off, d_len, out)
    else:
        if q.any():
            eng.absorb_device(state, d_arena, d_off0, d_q)
        eng.finish_device(state, d_prefix, d_arena, d_off, d_len, out)
        eng.device_status()
        if states is not None:
            got_state = state.cpu().numpy().view(np.uint32)
            bad.append(state_mismatch(what + ": absorbed states", mode, q, got_state,
                                      np.array(states, dtype=np.uint32)))
    eng.device_status()
    bad.append(mismatch(what, mode, tails, prefix, out.cpu().numpy(), exp))
    return [b for b in bad if b]


def run_absorb_case(eng, pattern, n, mode):
    """Two absorb launches over the same states (the second continues the first),
    every state checked word for word against midstate() after each."""
    import torch
    a, b = absorb_blocks(pattern, n)
    arena, off = build_arena(64 * (a + b), _seed("absorb", pattern))
    raw = arena.tobytes()
    state = _dev(_iv_rows(n).view(np.int32))
    d_arena = _dev(arena)
    bad = []
    done = np.zeros(n, dtype=np.int64)
    for tag, nb in (("first", a), ("second", b)):
        d_off, d_nb = _dev(off + 64 * done), _dev(nb)
        torch.cuda.synchronize()
        eng.absorb_device(state, d_arena, d_off, d_nb)
        eng.device_status()
        done = done + nb
        exp = np.array([midstate(raw[o:o + 64 * k]) for o, k in zip(off.tolist(), done.tolist())], dtype=np.uint32)
        bad.append(state_mismatch("absorb %s / %s launch (n = %d)" % (pattern, tag, n), mode, nb,
                                  state.cpu().numpy().view(np.uint32), exp))
    return [x for x in bad if x]


def run_device_matrix(eng, mode, n=N_SMALL):
    """The device-form matrix at n lanes: [(case, mismatches)]."""
    out = []
    for p, k in finish_cases():
        out.append(("finish_%s_%s" % (p, k), run_finish_case(eng, p, k, n, mode)))
    for p in ABSORB_PATTERNS:
        out.append(("absorb_%s" % p, run_absorb_case(eng, p, n, mode)))
    return out


def device_matrix_cases():
    return ["finish_%s_%s" % c for c in finish_cases()] + ["absorb_%s" % p for p in ABSORB_PATTERNS]


def run_set_pass(eng, n, seed, staging_bytes=0):
    """A stream set of n streams over TAILS, each message written in 1 to 4 cuts at
    CUT_KINDS boundaries, sum() after every round. Returns (launches, bad): the load
    mode every launch reported ({"op", "mode"}; a round that only buffered launched
    nothing and is left out) and the failed comparisons."""
    from mirbft_amd import StreamSet
    msgs, bounds, used = set_pass_inputs(n, seed)
    ids = np.arange(n, dtype=np.uint64)
    launches, bad = [], []
    assert used == set(CUT_KINDS), set(CUT_KINDS) - used
    with StreamSet(eng, n, staging_bytes=staging_bytes) as ss:
        for r in range(4):
            before = ss.stats()["launches_absorb"]
            ss.write(ids, [m[b[r]:b[r + 1]] for m, b in zip(msgs, bounds)])
            st = ss.stats()
            if st["launches_absorb"] > before:
                launches.append({"op": "write %d" % r, "mode": st["last_load_mode"]})
            got = ss.sum()
            launches.append({"op": "sum %d" % r, "mode": ss.stats()["last_load_mode"]})
            exp = _digest_rows([sha(m[:b[r + 1]]) for m, b in zip(msgs, bounds)])
            wrong = np.nonzero(np.any(got != exp, axis=1))[0]
            if wrong.size:
                bad.append({"what": "stream set, round %d" % r, "bad": int(wrong.size), "of": n,
                            "first": [{"stream": int(i), "bounds": bounds[i],
                                       "tail_len": bounds[i][r + 1] % 64, "prefix": bounds[i][r + 1] // 64 * 64}
                                      for i in wrong[:6]]})
            if ss.lengths().tolist() != [b[r + 1] for b in bounds]:
                bad.append({"what": "stream set, round %d: lengths()" % r})
    return launches, bad


# ---------------------------------------------------------------------------
# Forced load modes (MSHA_LOAD_MODE), in a process of their own
# ---------------------------------------------------------------------------
def child_cases():
    return device_matrix_cases() + ["stream_set"]


def child_main():
    mode = int(os.environ["MSHA_LOAD_MODE"])
    import torch  # one HIP runtime per process: torch's, loaded before libmirsha (see mirbft_amd/_lib.py)
    torch.cuda.init()
    from mirbft_amd import Engine, _lib
    _lib.require_tree_build("tests/stream_matrix.py --child")   # conftest.py's rule
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ran = stream_mode(N_SMALL, cus, mode)

    def emit(case, bad, **more):
        print(json.dumps(dict({"case": case, "mode": mode, "cus": cus, "mismatch": bad}, **more)), flush=True)

    with Engine(1) as eng:
        for case, bad in run_device_matrix(eng, ran):
            emit(case, bad)
        launches, bad = run_set_pass(eng, N_SMALL, 12)
        emit("stream_set", bad, launches=launches)
    return 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        sys.exit(child_main())
    sys.exit("usage: MSHA_LOAD_MODE=0..3 python tests/stream_matrix.py --child")
