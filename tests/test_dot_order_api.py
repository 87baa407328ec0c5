"""The dot-order switch without a GPU: libsbhip.so exports sb_set_dot_order / sb_dot_order / sb_cg_set_dot_order /
sb_cg_dot_order (include/sbhip.h), and the process default follows SB_DOT_ORDER before sb_init -- unset: tree (0),
"seq": 1, anything else: the process ends with a message naming the file and line."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sb_set_dot_order", "sb_dot_order", "sb_cg_set_dot_order", "sb_cg_dot_order")


def test_library_exports_the_dot_order_symbols():
    from sparsebench_amd import capi
    L = capi.load()
    for s in NEW:
        assert hasattr(L, s), "libsbhip.so does not export %s" % s
        assert s in capi.SYMBOLS


CHILD = ("import sys; sys.path.insert(0, %r)\n"
         "from sparsebench_amd import capi\n"
         "L = capi.load()\n"
         "print('ORDER', L.sb_dot_order())\n"
         "L.sb_set_dot_order(1 - L.sb_dot_order())\n"
         "print('SET', L.sb_dot_order())\n"
         "print('INIT', L.sb_is_initialized())\n") % ROOT


def _child(value):
    env = dict(os.environ)
    env.pop("SB_DOT_ORDER", None)
    if value is not None:
        env["SB_DOT_ORDER"] = value
    return subprocess.run([sys.executable, "-c", CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("value,want", [(None, 0), ("tree", 0), ("seq", 1)])
def test_environment_sets_the_process_default(value, want):
    out = _child(value)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    txt = out.stdout.decode()
    assert "ORDER %d" % want in txt and "SET %d" % (1 - want) in txt
    assert "INIT 0" in txt  # read without touching a device


@pytest.mark.parametrize("value", ["sequential", "SEQ", "1", "tree,seq"])
def test_a_bad_value_fails_loudly(value):
    out = _child(value)
    assert out.returncode != 0
    err = out.stderr.decode()
    assert "SB_DOT_ORDER=%s" % value in err and "expected tree or seq" in err, err[-2000:]
    assert "sbhip_launch.inc.h:" in err  # file:line, as the library's other errors
    assert "ORDER" not in out.stdout.decode()


def test_a_bad_argument_fails_loudly():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from sparsebench_amd import capi\n"
            "capi.load().sb_set_dot_order(2)\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode != 0 and "sb_set_dot_order(2)" in out.stderr.decode()
