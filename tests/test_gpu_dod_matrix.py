"""The digest-of-digests matrix on the GPU (tests/dod_matrix.py): k_digest_of_digests
and the DigestSrc form of k_digest_split, through the device entry, the host entry's
small path, its pipeline and three virtual shards -- given waves on either side of the
index stage and on its edge, waves uniform but for one lane, every count modulo 4 on
both sides of 4, and surplus chains with fewer, as many and more blocks than
segments. Each case asserts the exact msha_stats deltas of the kernel it claims to
test and every digest, bit-exact: there is no tolerance anywhere. The expected
digests are hashlib's, or the oracle's scalar leg for the large cases.

Not tested: a `begin` past 2^32 (the high halves of k0 and the span that
DigestSrc::full carries through readfirstlane / readlane pairs): it needs 16 GiB of
idx."""
import numpy as np
import pytest

import dod_matrix as DM
import kernel_matrix as KM

pytestmark = pytest.mark.gpu

ENV = ("MSHA_SMALL_BYTES", "MSHA_SMALL_MSGS", "MSHA_VIRTUAL_SHARDS", "MSHA_SMALL_CHAIN8", "MSHA_SMALL_CHAIN2")


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


CASES = DM.cases()


@pytest.mark.parametrize("name,pattern,index_pattern", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_dod_matrix(engine, monkeypatch, name, pattern, index_pattern):
    t = DM.target(name)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in t["env"].items():
        monkeypatch.setenv(k, v)
    DM.run_case(None if t["fresh"] else engine, name, pattern, index_pattern, _cus())


def test_split_epoch_ring_with_fresh_indices(engine, monkeypatch):
    """The same ragged split case six times on one context, the indices drawn afresh
    each time: six epochs of the split flag ring with DigestSrc, every digest exact
    each time (a chain that took a flag of an earlier launch for its own would hash
    from a stale state)."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    c = _cus()
    t = DM.target("dod_split_s5")
    begin = DM.case_begin(t, "ragged", c)
    ls = DM.launches(t, "ragged", c, begin)
    assert ls[0][2], "on %d CUs this n does not split" % c
    for rep in range(6):
        what = "dod_split_s5 / ragged, call %d" % rep
        table, idx = DM.build_index("random", int(begin[-1]), KM._salt("ring", rep))
        d, got = DM.run_call(engine, "device", table, idx, begin)
        KM.check_deltas(KM._only(launches_split=1, launches_dod=0, small_calls=0), d, what)
        bad = DM.mismatch(what, begin, got, DM.expected(table, idx, begin), ls)
        assert bad is None, bad


REJECTED = [
    ("begin_0_not_0", [1, 3, 5], 5, "begin must start at 0 and end at n_idx"),
    ("begin_n_not_n_idx", [0, 3, 4], 5, "begin must start at 0 and end at n_idx"),
    ("begin_n_past_n_idx", [0, 3, 6], 5, "begin must start at 0 and end at n_idx"),
    ("begin_decreasing", [0, 4, 3, 5], 5, "begin must be non-decreasing"),
]


@pytest.mark.parametrize("what,begin,n_idx,text", REJECTED, ids=[r[0] for r in REJECTED])
def test_host_entry_rejects_a_bad_begin(engine, monkeypatch, what, begin, n_idx, text):
    """msha_digest_of_digests refuses a begin that does not start at 0, does not end
    at n_idx, or decreases: MSHA_ERR_INVALID_ARG with its text, nothing launched, and
    the context hashes the next batch."""
    from mirbft_amd import _lib
    from mirbft_amd.engine import MshaError
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    table, idx = DM.build_index("random", n_idx, 9)
    st0 = engine.stats()
    with pytest.raises(MshaError) as ei:
        engine.digest_of_digests(table, idx, np.array(begin, dtype=np.uint64))
    assert ei.value.code == _lib.MSHA_ERR_INVALID_ARG and text in str(ei.value)
    st1 = engine.stats()
    assert all(st1[k] == st0[k] for k in DM.COUNTERS + ("calls", "messages")), (st0, st1)
    good = DM.to_begin(np.array([2, 0, 3]))
    assert np.array_equal(engine.digest_of_digests(table, idx, good), DM.expected_hashlib(table, idx, good))
    engine.device_status()
