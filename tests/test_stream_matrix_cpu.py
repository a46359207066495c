"""The stream kernel matrix (tests/stream_matrix.py) checked without a GPU: the
case builders hit, by their lengths alone, every cell they promise -- the cell sets
are compared for equality, so a thinned pattern fails here and not silently on the
GPU -- and the reference the GPU tests rest on, resume_digest(), agrees with
hashlib wherever hashlib can express the message."""
import hashlib
import random
import struct

import numpy as np
import pytest

import stream_matrix as SM

BIG, SMALL = 256, 8        # CUs: the MI355X's count, and a small device


def test_the_cell_sets_are_the_full_products():
    assert len(SM.FINISH_CELLS) == 3 * 3 * 3 * 3 and len(SM.ABSORB_CELLS) == 5 * 2 * 3
    assert {SM.r_class(t) for t in range(384)} == set(SM.R_CLASSES)
    assert {SM.nfull_class(t) for t in range(384)} == set(SM.NFULL_CLASSES)
    assert [SM.nb_class(k) for k in range(8)] == ["nb0", "nb1", "nb2", "nb_odd", "nb_even", "nb_odd", "nb_even",
                                                  "nb_odd"]
    assert (SM.r_class(0), SM.r_class(1), SM.r_class(55), SM.r_class(56), SM.r_class(63), SM.r_class(64)) == \
        ("r0", "r1_55", "r1_55", "r56_63", "r56_63", "r0")
    assert (SM.nfull_class(63), SM.nfull_class(64), SM.nfull_class(128), SM.nfull_class(4151)) == \
        ("nfull0", "nfull_odd", "nfull_even", "nfull_even")


def test_finish_cases_hit_every_cell():
    """The device-form matrix at 421 lanes: the nine (pattern, state kind) cases
    together hit all 81 finish cells, and each state kind alone all 27 of its own."""
    assert SM.N_SMALL % 64 == SM.PARTIAL_LANES
    cells = set()
    for kind in SM.STATE_KINDS:
        own = set()
        for p in SM.FINISH_PATTERNS:
            assert (p, kind) in SM.finish_cases()
            own |= SM.finish_case_cells(p, kind)
        assert own == {c for c in SM.FINISH_CELLS if c[2] == kind}, (kind, sorted(SM.FINISH_CELLS - own))
        cells |= own
    assert cells == SM.FINISH_CELLS
    assert len(SM.finish_cases()) == 9


def test_finish_tail_lengths_cover_0_to_383_and_the_long_ones():
    want = set(range(384)) | {1000, 4151}
    assert set(SM.finish_tails("ragged").tolist()) == want
    # every whole wave of the ragged pattern holds 64 different lengths
    t = SM.finish_tails("ragged")
    for s in range(0, SM.N_SMALL - SM.PARTIAL_LANES, 64):
        assert len(set(t[s:s + 64].tolist())) == 64
    both = set(SM.finish_tails("uniform_up")[:384].tolist()) | set(SM.finish_tails("uniform_down")[:384].tolist())
    assert both == set(SM.UNIFORM_TAILS)
    assert {(SM.r_class(u), SM.nfull_class(u)) for u in SM.UNIFORM_TAILS} == \
        {(r, f) for r in SM.R_CLASSES for f in SM.NFULL_CLASSES}
    assert {(SM.r_class(u), SM.nfull_class(u)) for u in SM.PARTIAL_TAILS} == \
        {(r, f) for r in SM.R_CLASSES for f in SM.NFULL_CLASSES}


def test_resumed_lanes_absorb_one_to_three_blocks():
    """The split point of a resumed lane: q = 1..3 of its message's blocks absorbed,
    d_len still every tail length; each (tail length, q) pairing varies by lane."""
    q = SM.resume_blocks(SM.N_SMALL, "resumed")
    assert set(q.tolist()) == {1, 2, 3}
    for w in range(0, SM.N_SMALL, 64):
        assert set(q[w:w + 64].tolist()) == {1, 2, 3}          # the prefix varies inside every wave
    for kind in ("iv", "null"):
        assert not SM.resume_blocks(SM.N_SMALL, kind).any()


@pytest.mark.parametrize("cus", [BIG, SMALL])
def test_the_natural_pair_case(cus):
    """n = 768 CUs + 37 is in the kPair range and below it kPrefetch; the lanes of
    that case hit every finish cell of the two state kinds one launch can mix, a
    third of them resumed, and tail lengths 0..383."""
    n = SM.pair_n(cus)
    assert n % 64 == SM.PARTIAL_LANES
    assert SM.stream_mode(n, cus) == 2 and SM.stream_mode(768 * cus - 1, cus) == 1
    assert SM.stream_mode(SM.N_SMALL, cus) == 1                 # pick_mode's kPipe range runs as kPrefetch
    assert SM.pick_mode(SM.N_SMALL, cus) == 3
    for forced in range(4):
        assert SM.stream_mode(SM.N_SMALL, cus, forced) == (1 if forced == 3 else forced)
    q = SM.resume_blocks(n, "third")
    assert abs(int((q > 0).sum()) - n / 3) <= SM.PARTIAL_LANES and set(q[q > 0].tolist()) == {1, 2, 3}
    assert SM.finish_case_cells("pair", "third", n) == {c for c in SM.FINISH_CELLS if c[2] != "null"}
    t = SM.finish_tails("pair", n)
    assert set(range(384)) <= set(t.tolist())
    assert set(range(384)) == set(t[q > 0].tolist()) - {1000, 4151}        # the resumed lanes alone see 0..383
    assert int((64 * q + (t + 63) // 64 * 64).sum()) < (100 << 20) * cus // BIG + (1 << 20)   # the arena stays small


def test_absorb_cases_hit_every_cell():
    cells = set()
    for p in SM.ABSORB_PATTERNS:
        cells |= SM.absorb_case_cells(p)
    assert cells == SM.ABSORB_CELLS, sorted(SM.ABSORB_CELLS - cells)
    # block counts of the launches: {0, 1, 2, odd > 2, even > 2}
    for p in SM.ABSORB_PATTERNS:
        a, b = SM.absorb_blocks(p)
        assert {SM.nb_class(x) for x in a.tolist()} == set(SM.NB_CLASSES), p
        assert {SM.nb_class(x) for x in b.tolist()} == set(SM.NB_CLASSES), p


def test_the_child_runs_every_case():
    assert SM.child_cases() == SM.device_matrix_cases() + ["stream_set"]
    assert len(SM.device_matrix_cases()) == 9 + 2
    msgs, bounds, used = SM.set_pass_inputs(SM.N_SMALL, 12)
    assert used == set(SM.CUT_KINDS)
    assert {len(m) for m in msgs} == set(range(384)) | {1000, 4151}
    assert {sum(1 for j in range(4) if b[j + 1] > b[j] or j == 0) for b in bounds} >= {1, 2, 3, 4}
    for m, b in zip(msgs, bounds):
        assert b[0] == 0 and b[4] == len(m) and b == sorted(b)
    msgs, bounds, used = SM.set_pass_inputs(229, 5)      # the set of the piece tests
    assert used == set(SM.CUT_KINDS)


# -- the reference -------------------------------------------------------------------------
def test_compress_is_sha256():
    for n in (0, 3, 55, 56, 64, 200):
        m = bytes(range(256))[:n]
        padded = m + b"\x80" + b"\x00" * ((55 - n) % 64) + struct.pack(">Q", 8 * n)
        assert struct.pack(">8I", *SM.midstate(padded)) == hashlib.sha256(m).digest()


def test_resume_digest_from_the_iv_is_hashlib():
    rnd = random.Random(1)
    for t in list(range(384)) + [1000, 4151]:
        m = rnd.randbytes(t)
        assert SM.resume_digest(SM.IV, m, t) == hashlib.sha256(m).digest(), t


@pytest.mark.parametrize("prefix", [64, 128, 4096])
def test_resume_digest_from_a_midstate_is_hashlib(prefix):
    rnd = random.Random(prefix)
    head = rnd.randbytes(prefix)
    state = SM.midstate(head)
    assert state != SM.IV
    for t in range(384):
        tail = rnd.randbytes(t)
        assert SM.resume_digest(state, tail, prefix + t) == hashlib.sha256(head + tail).digest(), (prefix, t)


def test_resume_digest_takes_the_bit_length_mod_2_64():
    """What hashlib cannot express: the last eight bytes of the padded input are
    (8 total) mod 2^64, big-endian -- Go's `len <<= 3` on a uint64."""
    state, tail = list(range(1, 9)), b"abc"
    for total, bits in ((2 ** 29, 2 ** 32), (2 ** 32 + 3, 2 ** 35 + 24), (2 ** 61, 0), (2 ** 61 + 3, 24)):
        padded = tail + b"\x80" + bytes(52) + struct.pack(">Q", bits)
        assert SM.resume_digest(state, tail, total) == struct.pack(">8I", *SM.absorb(state, padded)), total
    assert SM.resume_digest(state, tail, 2 ** 61 + 3) == SM.resume_digest(state, tail, 3)
    assert SM.resume_digest(state, tail, 2 ** 29 + 3) != SM.resume_digest(state, tail, 3)


def test_expected_finish_is_the_whole_message_hash():
    """expected_finish(): a resumed lane's digest through resume_digest from the
    expected absorbed state equals hashlib over the whole message."""
    n = 64 + 37
    tails, q = SM.finish_tails("ragged", n), SM.resume_blocks(n, "resumed")
    arena, off = SM.build_arena(64 * q + tails, 1)
    raw = arena.tobytes()
    states = [SM.midstate(raw[o:o + 64 * k]) for o, k in zip(off.tolist(), q.tolist())]
    a = SM.expected_finish(raw, off, q, tails, states)
    b = SM.expected_finish(raw, off, q, tails)
    assert a.shape == (n, 32) and np.array_equal(a, b)
    assert (off % 64 == 0).all() and len(raw) >= int(off[-1] + 64 * q[-1] + tails[-1]) + 64


def test_mismatch_names_the_lane():
    tails, prefix = np.array([5, 200]), np.array([0, 128])
    exp = np.zeros((2, 32), dtype=np.uint8)
    got = exp.copy()
    assert SM.mismatch("x", 2, tails, prefix, got, exp) is None
    got[1, 0] = 1
    m = SM.mismatch("case x", 2, tails, prefix, got, exp)
    f = m["first"][0]
    assert m["what"] == "case x" and m["bad"] == 1
    assert (f["lane"], f["tail_len"], f["nfull"], f["r"], f["prefix"], f["load_mode"]) == (1, 200, 3, 8, 128, "kPair")
