"""Every rate tool's `run` on the GPU at the smallest arguments that walk all of it (tests/rate_tools_cases.py): a fresh child
process each, exit status 0, and the skeleton of what it emits -- the key tree in order with every int, str, bool and None leaf --
against tests/golden/rate_tools_skeleton.json, which was taken from two runs of the tools as they were before tools/ratelib.py
(a leaf on which those two runs differed is pinned by its type only, tests/golden/make_golden_rate_tools.py).  The process header
is held to the running build's own device, version and csrc_hash."""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from rate_tools_cases import CASES, HEADER, bad_floats, mismatch, skeleton
from sparsebench_amd import srchash

pytestmark = pytest.mark.gpu

LIMIT = 120  # s: a case takes a second or two
ended = []   # the case whose child ended on a time limit or a signal: no further GPU work is started behind it


@pytest.fixture(scope="module")
def skeletons():
    with open(os.path.join(GOLDEN, "rate_tools_skeleton.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", list(CASES))
def test_run_emits_the_skeleton(case, skeletons, gpu, tmp_path):
    if ended:
        pytest.skip("the child of %s ended on a time limit or a signal" % ended[0])
    tool, args = CASES[case]
    path = str(tmp_path / "one_process.json")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), "run"] + args.split() + ["--out", path],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        ended.append(case)
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        ended.append(case)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    with open(path) as f:
        out = json.load(f)
    assert json.loads(r.stdout.decode().strip().split("\n")[-1]) == out  # what it prints is what it writes
    assert mismatch(skeletons[case], skeleton(out)) is None
    assert [out[k] for k in HEADER] == [gpu.sb_device_name().decode(), gpu.sb_version().decode(), srchash.csrc_hash()]
    assert bad_floats(out) == []
