"""The per-kernel length matrix on the GPU (tests/kernel_matrix.py): every hash
kernel of kernels.hip -- the static lane kernel in both automatic load modes, the
split kernel's main workgroups and segments, the pipelined kernel, the planned
call's static and work-stealing lane kernels, the uniform-layout kernels, the
eight-lane, two-lane (both forms) and cooperative chain kernels -- given whole
waves of one length at every padding edge, waves uniform but for one lane, ragged
waves and block counts around the chain kernels' pairing threshold. Each case
asserts the launch counter of the kernel it claims to test and every digest,
bit-exact against the oracle's scalar FIPS 180-4 leg. The load modes that only
MSHA_LOAD_MODE reaches (read once per process) run in a fresh child process each.
"""
import json
import os
import subprocess
import sys

import pytest

import kernel_matrix as KM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Set when a child process ended by a signal or its time limit: nothing of this
# module goes to the GPU after that.
_child_fault = []


@pytest.fixture(autouse=True)
def _no_gpu_work_after_a_fault():
    if _child_fault:
        pytest.fail("not run: an earlier child process %s" % _child_fault[0])


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


CASES = KM.cases()


@pytest.mark.parametrize("name,pattern", CASES, ids=["%s-%s" % c for c in CASES])
def test_kernel_matrix(engine, monkeypatch, name, pattern):
    t = KM.target(name)
    for k in ("MSHA_LANE_WS", "MSHA_SMALL_CHAIN8", "MSHA_SMALL_CHAIN2"):
        monkeypatch.delenv(k, raising=False)
    for k, v in t["env"].items():
        monkeypatch.setenv(k, v)
    engine.set_kernel_policy(t["policy"])
    try:
        KM.run_case(engine, name, pattern, _cus())
    finally:
        engine.set_kernel_policy("auto")


def _run_child(mode):
    env = dict(os.environ)
    env["MSHA_LOAD_MODE"] = str(mode)
    cmd = [sys.executable, os.path.join(ROOT, "tests", "kernel_matrix.py"), "--child"]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    except subprocess.TimeoutExpired:
        _child_fault.append("(MSHA_LOAD_MODE=%d) ran into its time limit" % mode)
        pytest.fail("the child with MSHA_LOAD_MODE=%d ran into its time limit" % mode)
    if r.returncode < 0:
        _child_fault.append("(MSHA_LOAD_MODE=%d) ended by signal %d" % (mode, -r.returncode))
        pytest.fail("the child with MSHA_LOAD_MODE=%d ended by signal %d\n%s" % (mode, -r.returncode, r.stderr[-2000:]))
    return r


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_forced_load_mode(mode):
    """MSHA_LOAD_MODE = kSingle / kPrefetch / kPair / kPipe in a process of its own:
    the lane kernel (the pipelined one for mode 3) on whole-wave, near-uniform and
    ragged batches and on the uniform layout at a size where nothing but the forced
    mode decides, and the split kernel's main workgroups in modes 0 to 2."""
    r = _run_child(mode)
    assert r.returncode == 0, "child exit status %d\n%s" % (r.returncode, r.stderr[-2000:])
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            c = json.loads(line)
            got[c["case"]] = c
    assert list(got) == KM.child_cases(), (list(got), r.stderr[-2000:])
    for case, c in got.items():
        assert c["mode"] == mode
        what = "MSHA_LOAD_MODE=%d / %s" % (mode, case)
        kernel = KM.child_expected(case, mode, c["cus"])[0]
        if case == "split":
            assert kernel == "split", "%s: on %d CUs this n does not split" % (what, c["cus"])
            want = KM._only(launches_split=1)
        else:
            assert kernel == ("pipe" if mode == 3 else "lane"), "%s: on %d CUs outside the range (%s)" % (
                what, c["cus"], kernel)
            want = KM._only(launches_pipe=1) if mode == 3 else KM._only(launches_lane=1)
        KM.check_deltas(want, c["deltas"], what)
        assert c["mismatch"] is None, c["mismatch"]
