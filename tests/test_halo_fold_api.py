"""The halo-fold switch without a GPU: include/sbhip.h declares sb_comm_halo_fold / sb_comm_halo_fold_selected /
sb_cg_halo_fold and capi.load() binds them; the process default follows SB_HALO_FOLD before sb_init -- unset: 0, "0": 0,
"1": 1, anything else: the process ends with a message naming the variable, the file and the line."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sb_comm_halo_fold", "sb_comm_halo_fold_selected", "sb_cg_halo_fold")


def test_library_exports_the_halo_fold_symbols():
    from sparsebench_amd import capi, hostapi
    L = capi.load()
    for s in NEW:
        assert hasattr(L, s), "libsbhip.so does not export %s" % s
        assert s in capi.SYMBOLS
    header = open(os.path.join(ROOT, "include", "sbhip.h")).read()
    for s in NEW:
        assert s + "(" in header
    assert callable(hostapi.CG.halo_fold)


CHILD = ("import sys; sys.path.insert(0, %r)\n"
         "from sparsebench_amd import capi\n"
         "L = capi.load()\n"
         "print('FOLD', L.sb_comm_halo_fold_selected())\n"
         "print('INIT', L.sb_is_initialized())\n") % ROOT


def _child(value):
    env = dict(os.environ)
    env.pop("SB_HALO_FOLD", None)
    if value is not None:
        env["SB_HALO_FOLD"] = value
    return subprocess.run([sys.executable, "-c", CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("value,want", [(None, 0), ("", 0), ("0", 0), ("1", 1)])
def test_environment_sets_the_process_default(value, want):
    out = _child(value)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    txt = out.stdout.decode()
    assert "FOLD %d" % want in txt
    assert "INIT 0" in txt  # answered without touching a device


@pytest.mark.parametrize("value", ["2", "on", "yes", "01", "1 "])
def test_a_bad_value_fails_loudly(value):
    out = _child(value)
    assert out.returncode != 0
    err = out.stderr.decode()
    assert "SB_HALO_FOLD=%s" % value in err and "expected 0 or 1" in err, err[-2000:]
    assert "sbhip_comm.inc.h:" in err  # file:line, as the library's other errors
    assert "FOLD" not in out.stdout.decode()


def test_the_setter_needs_an_initialised_layer():
    """sb_comm_halo_fold synchronises the layer's stream: before sb_init it ends the process with the usual message"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from sparsebench_amd import capi\n"
            "capi.load().sb_comm_halo_fold(1)\n") % ROOT
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode != 0 and "sb_init() has not been called" in out.stderr.decode(), out.stderr.decode()[-2000:]
