#!/usr/bin/env python3
"""tests/golden/rate_tools_skeleton.json from two `run`s per case of tests/rate_tools_cases.py, made on an MI355X:

    for i in 0 1: tools/<tool>.py run <the case's arguments> --out DIR/<case>.$i.json
    tests/golden/make_golden_rate_tools.py DIR

A leaf keeps its value only where the two runs agree on it.  A leaf on which they differ is a measurement (poly_rate's
best_poly_to_eps names the handle with the smallest measured time): it is pinned by its type only, and so is every leaf of the same
key in the same tool's output, where the two runs agreed by chance.  The process header (device, library, csrc_hash) names the
build, not what the tool does: by type here, and tests/test_gpu_rate_tools.py holds it to the running build's own."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from rate_tools_cases import CASES, HEADER, leaf_type, pinned, skeleton  # noqa: E402


def moved(v, key=None):
    """the keys of the leaves pinned by type that are no floats"""
    if isinstance(v, dict):
        return {k for name, x in v.items() for k in moved(x, name)}
    if isinstance(v, list):
        return {k for x in v for k in moved(x, key)}
    return {key} if v[0] == ":" and v != ":float" else set()


def by_type(v, keys, key=None):
    if isinstance(v, dict):
        return {name: by_type(x, keys, name) for name, x in v.items()}
    if isinstance(v, list):
        return [by_type(x, keys, key) for x in v]
    return ":" + leaf_type(v) if key in keys else v


def main(runs):
    out = {}
    for case in CASES:
        a, b = (json.load(open(os.path.join(runs, "%s.%d.json" % (case, i)))) for i in (0, 1))
        out[case] = pinned(skeleton(a), skeleton(b))
        out[case].update({k: ":str" for k in HEADER})
        keys = moved(out[case]) - set(HEADER)
        if keys:
            print("%s: pinned by type only: %s" % (case, sorted(keys)))
            out[case] = by_type(out[case], keys)
    with open(os.path.join(HERE, "rate_tools_skeleton.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
