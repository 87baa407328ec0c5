"""The rate tools' shared module on the CPU (tools/ratelib.py): every `merge` against committed bytes, the solve helpers against
a fake handle, and every tool's command line against the table taken from the parsers before they were shared."""
import argparse
import ast
import importlib
import json
import math
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from rate_tools_cases import TOOLS

sys.path.insert(0, os.path.join(ROOT, "tools"))  # as `python tools/<tool>.py` has it
import ratelib  # noqa: E402

PROFILES = os.path.join(ROOT, "profiles")
RUNS = os.path.join(GOLDEN, "rate_runs")
WITH_RUNS = ("sgs_rate", "mg_rate", "mg_fw_rate", "poly_rate", "mg_poly_rate", "galerkin_rate", "aggregation_rate",
             "bicgstab_precond_rate")
GOLDEN_RUNS = {"pcg_rate": ("pcg_rate.0", "pcg_rate.1"), "bicgstab_rate": ("bicgstab_rate.0", "bicgstab_rate.1"),
               "gmres_rate": ("gmres_rate.0", "gmres_rate.1"), "cg_batch_rate": ("cg_batch_rate.0", "cg_batch_rate.1"),
               "gmres_precond_rate": ("gmres_precond_rate-cd.0", "gmres_precond_rate-cd.1", "gmres_precond_rate-hpcg.0")}
assert sorted(WITH_RUNS + tuple(GOLDEN_RUNS)) == sorted(TOOLS)


def merged_by(tool, files, out):
    importlib.import_module(tool).merge(argparse.Namespace(files=files, out=out))
    with open(out, "rb") as f:
        return f.read()


def inputs_and_merged(tool, tmp_path):
    """(per-process files, the merged bytes they must give): a profile's `runs` split back into its processes' files, or the
    golden runs with what the tool's merge made of them before it was shared"""
    if tool in GOLDEN_RUNS:
        return [os.path.join(RUNS, n + ".json") for n in GOLDEN_RUNS[tool]], os.path.join(RUNS, tool + ".merged.json")
    committed = os.path.join(PROFILES, tool + ".json")
    with open(committed) as f:
        prof = json.load(f)
    assert len(prof["devices"]) == 1  # the reconstruction needs it
    files = []
    for i, run in enumerate(prof["runs"]):
        if isinstance(run, list):  # a bare `cases` list
            run = {"device": prof["devices"][0], "library": prof["library"], "csrc_hash": prof["csrc_hash"], "cases": run}
        files.append(str(tmp_path / ("p%d.json" % i)))
        with open(files[-1], "w") as f:
            f.write(json.dumps(run) + "\n")
    return files, committed


@pytest.mark.parametrize("tool", TOOLS)
def test_merge_gives_the_committed_bytes(tool, tmp_path):
    files, want = inputs_and_merged(tool, tmp_path)
    with open(want, "rb") as f:
        assert merged_by(tool, files, str(tmp_path / "merged.json")) == f.read()


@pytest.mark.parametrize("tool", TOOLS)
def test_merge_refuses_runs_of_different_builds(tool, tmp_path):
    files, _ = inputs_and_merged(tool, tmp_path)
    with open(files[-1]) as f:
        other = dict(json.load(f), csrc_hash="0" * 16)
    with open(tmp_path / "other.json", "w") as f:
        json.dump(other, f)
    with pytest.raises(SystemExit) as e:
        merged_by(tool, [files[0], str(tmp_path / "other.json")], str(tmp_path / "merged.json"))
    assert str(e.value).startswith("the runs do not describe the same build")
    assert not os.path.exists(tmp_path / "merged.json")


# ---- find_k / to_eps / window_us against a fake handle -------------------------------------------------------------------

class Fake:
    """a handle whose loop stops after body `stop_after`; `k_off` and `ran_off` falsify what it reports"""
    COUNTER = "n_pAp"

    def __init__(self, stop_after=10 ** 9, k_off=0, ran_off=0):
        self.stop_after, self.k_off, self.ran_off = stop_after, k_off, ran_off
        self.pieces, self.solves, self.done, self.stop_seen = [], [], 0, False

    def start(self, itermax, eps):
        self.started, self.done, self.pieces, self.stop_seen = (itermax, eps), 0, [], False

    def _run(self, cnt):
        assert not self.stop_seen, "a piece was requested after the stop flag was read as set"
        self.pieces.append(cnt)
        self.done = min(self.done + cnt, self.stop_after)

    def counters(self):
        stop = int(self.done >= self.stop_after)
        self.stop_seen = self.stop_seen or bool(stop)
        return {"stop": stop, self.COUNTER: self.done + self.ran_off}

    def finish(self):
        return self.done + 1 + self.k_off

    def solve(self, itermax, eps):
        self.solves.append((itermax, eps))
        self.done = min(itermax - 1, self.stop_after)
        return self.finish()

    def loop_ms(self):
        return 0.5 * self.done


class CG(Fake):
    run_iters = Fake._run


class PCG(CG):
    pass


class BiCGStab(Fake):
    COUNTER = "n_rv"
    run_iters = Fake._run


class GMRES(Fake):
    COUNTER = "steps"
    run_steps = Fake._run

    def run_iters(self, cnt):
        raise AssertionError("a handle that steps was asked to iterate")


KINDS = (CG, PCG, BiCGStab, GMRES)


@pytest.mark.parametrize("cls", KINDS)
def test_find_k_pieces(cls):
    s = cls()
    assert ratelib.find_k(s, 24, 1e-3, 10) == 24 and s.pieces == [10, 10, 3] and s.started == (24, 1e-3)  # 23 bodies, no stop
    s = cls()
    assert ratelib.find_k(s, 24, 1e-3, 50) == 24 and s.pieces == [23]  # a piece larger than itermax - 1
    s = cls(stop_after=12)
    assert ratelib.find_k(s, 24, 1e-3, 5) == 13 and s.pieces == [5, 5, 5]  # nothing requested once stop is seen (Fake._run asserts)
    s = cls(stop_after=10, k_off=3)
    assert ratelib.find_k(s, 24, 1e-3, 5) == 14 and s.pieces == [5, 5]  # k is what finish() returns
    assert ratelib.find_ks({"a": cls(stop_after=3), "b": cls(stop_after=7)}, argparse.Namespace(itermax=24, piece=2), 0.1) == {"a": 4, "b": 8}


@pytest.mark.parametrize("cls", KINDS)
def test_to_eps(cls):
    s = cls(stop_after=12)
    assert ratelib.to_eps(s, 13, 1e-3) == 6.0 and s.solves == [(13, 1e-3)]
    kind = cls.__name__.lower()
    for named, who in ((False, ""), (True, kind + " ")):
        with pytest.raises(RuntimeError) as e:
            ratelib.to_eps(cls(stop_after=12, k_off=-1), 13, 1e-3, named)
        assert str(e.value) == "the timed solve did not run the 12 bodies that reach eps: %sk=12 bodies run 12" % who
        with pytest.raises(RuntimeError) as e:
            ratelib.to_eps(cls(stop_after=12, ran_off=1), 13, 1e-3, named)
        assert str(e.value) == "the timed solve did not run the 12 bodies that reach eps: %sk=13 bodies run 13" % who


@pytest.mark.parametrize("cls", KINDS)
def test_window_us(cls):
    s = cls()
    assert ratelib.window_us(s, 8, "x") == 1e3 * 4.0 / 8 and s.solves == [(9, 0.0)]  # itermax = bodies + 1 at eps = 0
    with pytest.raises(RuntimeError) as e:
        ratelib.window_us(cls(stop_after=6), 8, "x")  # r.r reached 0.0 early: k and the counter both fall short
    assert str(e.value) == "the timed loop did not run every body: x k=7 bodies run 6"
    with pytest.raises(RuntimeError) as e:
        ratelib.window_us(cls(k_off=1), 8, "x")
    assert str(e.value) == "the timed loop did not run every body: x k=10 bodies run 8"
    with pytest.raises(RuntimeError) as e:
        ratelib.window_us(cls(ran_off=-1), 8, "x")
    assert str(e.value) == "the timed loop did not run every body: x k=9 bodies run 7"


def test_the_loops_warm_every_name_once_then_alternate():
    order = []
    got = ratelib.alternate(("a", "b", "c"), 2, lambda n: order.append(n) or len(order))
    assert order == ["a", "b", "c"] + ["a", "b", "c"] * 2 and got == {"a": [4, 7], "b": [5, 8], "c": [6, 9]}
    order = []
    ratelib.alternate(("a", "b"), 1, order.append, lambda n: order.append("warm " + n))
    assert order == ["warm a", "warm b", "a", "b"]
    solvers = {"cg": CG(), "gmres": GMRES()}
    assert ratelib.body_windows(solvers, ["gmres", "cg"], 4, 3) == {"gmres": [500.0] * 3, "cg": [500.0] * 3}
    assert [len(s.solves) for s in solvers.values()] == [4, 4]
    solvers = {"a": CG(stop_after=5), "b": BiCGStab(stop_after=30), "c": GMRES(stop_after=7)}
    ks = {"a": 6, "b": 24, "c": 8}
    assert ratelib.reached(ks, 24) == {"a": True, "b": False, "c": True}
    assert ratelib.to_eps_rounds(solvers, ks, 0.1, 2, ratelib.reached(ks, 24)) == {"a": [2.5, 2.5], "b": [], "c": [3.5, 3.5]}
    assert solvers["b"].solves == [] and solvers["c"].solves == [(8, 0.1)] * 2
    assert ratelib.to_eps_rounds(solvers, ks, 0.1, 0) == {"a": [], "b": [], "c": []}
    assert ratelib.medians({"a": [3.0, 1.0, 2.0], "b": []}) == {"a": 2.0, "b": None}
    assert ratelib.rounded({"a": [1.234, 5.678], "b": None, "c": 0.126}, 2) == {"a": [1.23, 5.68], "b": None, "c": 0.13}


def test_rel_eps_is_each_former_spelling():
    """1e-10 * np.linalg.norm(b), 1e-10 * math.sqrt(np.dot(b, b)) and, for b = 1, 1e-10 * math.sqrt(nr): the same double"""
    class P:
        def __init__(self, b):
            self.b = b

        def rhs(self):
            return self.b, None

    for b in (np.random.default_rng(7).standard_normal(4097) * 1e3, np.ones(1536), np.ones(80 ** 3)):
        assert ratelib.rel_eps(P(b)) == 1e-10 * math.sqrt(float(np.dot(b, b))) == 1e-10 * float(np.linalg.norm(b))
    assert ratelib.rel_eps(P(np.ones(1536))) == 1e-10 * math.sqrt(float(1536))


def test_ranges():
    rows = {}
    for e in ({"k": 5, "x": 2.0, "y": 1.0}, {"k": 5, "x": 1.5}):
        ratelib.collect(rows, "s", e, ("x", "y", "z"))
    assert rows == {"s": {"k": 5, "x": [2.0, 1.5], "y": [1.0], "z": []}} and list(rows["s"]) == ["k", "x", "y", "z"]
    with pytest.raises(SystemExit) as e:
        ratelib.collect(rows, "s", {"k": 6}, ("x", "y", "z"))
    assert str(e.value) == "k of s differs between processes"
    ratelib.ranges(rows.values(), ("x", "y", "z"))
    assert rows == {"s": {"k": 5, "x": [1.5, 2.0], "y": [1.0, 1.0], "z": None}}


# ---- the command line ----------------------------------------------------------------------------------------------------

def cli_table(ap):
    """subcommand -> option -> [dest, type name, default, choices, nargs, required]"""
    sub = next(a for a in ap._actions if isinstance(a, argparse._SubParsersAction))
    return {cmd: {(a.option_strings[0] if a.option_strings else a.dest):
                  [a.dest, a.type.__name__ if a.type else None, a.default, list(a.choices) if a.choices else None, a.nargs, a.required]
                  for a in p._actions if not isinstance(a, argparse._HelpAction)} for cmd, p in sub.choices.items()}


@pytest.mark.parametrize("tool", TOOLS)
def test_command_line_is_the_one_before(tool):
    with open(os.path.join(GOLDEN, "rate_tools_cli.json")) as f:
        want = json.load(f)[tool]
    ap = importlib.import_module(tool).main(parse=False)
    assert cli_table(ap) == want
    sub = next(a for a in ap._actions if isinstance(a, argparse._SubParsersAction))
    assert sub.dest == "cmd" and sub.required


def test_no_rate_tool_imports_another():
    for tool in TOOLS:
        with open(os.path.join(ROOT, "tools", tool + ".py")) as f:
            src = f.read()
        names = [n.name for node in ast.walk(ast.parse(src)) if isinstance(node, ast.Import) for n in node.names]
        names += [node.module or "" for node in ast.walk(ast.parse(src)) if isinstance(node, ast.ImportFrom)]
        assert not [n for n in names if n.split(".")[-1].endswith("_rate")], tool
        assert "sys.path" not in src, tool
