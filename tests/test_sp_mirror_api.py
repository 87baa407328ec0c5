"""The single-precision mirror switch without a GPU: libsbhip.so exports sb_set_sp_mirror / sb_sp_mirror /
sb_matrix_all_row_programs (include/sbhip.h), the process default follows SB_SP_MIRROR before sb_init -- unset: 0, "0": 0,
"1": 1, anything else: the process ends with a message naming the file and line -- and hostapi.Problem refuses mirror=True on
a double-precision problem."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sb_set_sp_mirror", "sb_sp_mirror", "sb_matrix_all_row_programs")


def test_library_exports_the_sp_mirror_symbols():
    from sparsebench_amd import capi
    L = capi.load()
    for s in NEW:
        assert hasattr(L, s), "libsbhip.so does not export %s" % s
        assert s in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "sbhip.h")).read()
    for s in NEW:
        assert s + "(" in header


CHILD = ("import sys; sys.path.insert(0, %r)\n"
         "from sparsebench_amd import capi\n"
         "L = capi.load()\n"
         "print('MIRROR', L.sb_sp_mirror())\n"
         "L.sb_set_sp_mirror(1 - L.sb_sp_mirror())\n"
         "print('SET', L.sb_sp_mirror())\n"
         "print('INIT', L.sb_is_initialized())\n") % ROOT


def _child(value):
    env = dict(os.environ)
    env.pop("SB_SP_MIRROR", None)
    if value is not None:
        env["SB_SP_MIRROR"] = value
    return subprocess.run([sys.executable, "-c", CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("value,want", [(None, 0), ("0", 0), ("1", 1)])
def test_environment_sets_the_process_default(value, want):
    out = _child(value)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    txt = out.stdout.decode()
    assert "MIRROR %d" % want in txt and "SET %d" % (1 - want) in txt
    assert "INIT 0" in txt  # read without touching a device


@pytest.mark.parametrize("value", ["on", "2", "yes", "01", "1 "])
def test_a_bad_value_fails_loudly(value):
    out = _child(value)
    assert out.returncode != 0
    err = out.stderr.decode()
    assert "SB_SP_MIRROR=%s" % value in err and "expected 0 or 1" in err, err[-2000:]
    assert "sbhip_sp.inc.h:" in err  # file:line, as the library's other errors
    assert "MIRROR" not in out.stdout.decode()


@pytest.mark.parametrize("arg", [2, -1])
def test_a_bad_argument_fails_loudly(arg):
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from sparsebench_amd import capi\n"
            "capi.load().sb_set_sp_mirror(%d)\n") % (ROOT, arg)
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    err = out.stderr.decode()
    assert out.returncode != 0 and "sb_set_sp_mirror(%d)" % arg in err and "sbhip_sp.inc.h:" in err, err[-2000:]


def test_mirror_on_a_double_precision_problem_is_refused():
    from sparsebench_amd import hostapi
    with pytest.raises(ValueError):
        hostapi.Problem("generate", 8, 8, 8, fmt="scs", precision="double", mirror=True)
