"""The thirteen rate tools (tools/*_rate.py with the run / merge shape): the smallest `run` arguments that still walk every branch
of each, and the skeleton of a `run`'s JSON that tests/golden/rate_tools_skeleton.json pins.

The generated grid is 16^3 (the smallest with the four-level hierarchy 16 -> 8 -> 4 -> 2), the irregular stand-in 8^3 nodes, the
convection-diffusion grid 8^3; windows of 5 bodies, 2 repeats, 2 applies."""
import json
import math

TOOLS = ("sgs_rate", "pcg_rate", "bicgstab_rate", "gmres_rate", "cg_batch_rate", "mg_rate", "mg_fw_rate", "poly_rate",
         "mg_poly_rate", "galerkin_rate", "aggregation_rate", "bicgstab_precond_rate", "gmres_precond_rate")

HEADER = ("device", "library", "csrc_hash")  # what every `run` says of its process

# case -> (tool, arguments behind `run`)
CASES = {
    "sgs_rate": ("sgs_rate", "--n 16 --scaled 16 --nodes 8 --bodies 5 --repeats 2 --apply-reps 2"),
    "pcg_rate": ("pcg_rate", "--n 16 --nodes 8 --bodies 5 --repeats 2 --sol-repeats 2"),
    "bicgstab_rate": ("bicgstab_rate", "--n 16 --cd 8 --bodies 5 --repeats 2 --sol-repeats 2"),
    "gmres_rate": ("gmres_rate", "--n 16 --restart 5 --cycles 2 --repeats 2"),
    "cg_batch_rate": ("cg_batch_rate", "--n 16 --bodies 5 --repeats 2"),
    "mg_rate": ("mg_rate", "--n 16 --small 16 --bodies 5 --repeats 2 --apply-reps 2"),
    "mg_fw_rate": ("mg_fw_rate", "--sizes 16 --bodies 5 --repeats 2 --apply-reps 2"),
    "poly_rate": ("poly_rate", "--sizes 16 --nodes 8 --bodies 5 --repeats 2 --apply-reps 2"),
    "mg_poly_rate": ("mg_poly_rate", "--sizes 16 --bodies 5 --repeats 2 --apply-reps 2"),
    "galerkin_rate": ("galerkin_rate", "--cases 16:scs,16:crs --repeats 2"),
    "aggregation_rate": ("aggregation_rate", "--cases hpcg:16:scs,irregular:8:crs --sizes 8 --repeats 2"),
    "bicgstab_precond_rate-cd": ("bicgstab_precond_rate", "--problem cd --cd 8 --repeats 2"),
    "bicgstab_precond_rate-hpcg": ("bicgstab_precond_rate", "--problem hpcg --n 16 --repeats 2"),
    "gmres_precond_rate-cd": ("gmres_precond_rate", "--problem cd --cd 8 --repeats 2"),
    "gmres_precond_rate-hpcg": ("gmres_precond_rate", "--problem hpcg --n 16 --repeats 2"),
}


def skeleton(v):
    """the key tree in order; an int, str, bool or None leaf as "=<its JSON>", a float leaf as ":float" """
    if isinstance(v, dict):
        return {k: skeleton(x) for k, x in v.items()}
    if isinstance(v, list):
        return [skeleton(x) for x in v]
    return ":float" if isinstance(v, float) else "=" + json.dumps(v)


def leaf_type(leaf):
    return leaf[1:] if leaf[0] == ":" else type(json.loads(leaf[1:])).__name__


def pinned(a, b):
    """the skeleton two runs agree on: a leaf on whose value they differ is pinned by its type only, as ":int" """
    if isinstance(a, dict) and isinstance(b, dict) and list(a) == list(b):
        return {k: pinned(a[k], b[k]) for k in a}
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [pinned(x, y) for x, y in zip(a, b)]
    if isinstance(a, str) and isinstance(b, str) and leaf_type(a) == leaf_type(b):
        return a if a == b else ":" + leaf_type(a)
    raise ValueError("the two runs differ in shape: %r / %r" % (a, b))


def mismatch(want, got, path="$"):
    """the first place where the skeleton `got` leaves the pinned skeleton `want`, or None"""
    if isinstance(want, dict) and isinstance(got, dict):
        if list(want) != list(got):
            return "%s: keys %r, want %r" % (path, list(got), list(want))
        pairs = [("%s.%s" % (path, k), want[k], got[k]) for k in want]
    elif isinstance(want, list) and isinstance(got, list):
        if len(want) != len(got):
            return "%s: %d entries, want %d" % (path, len(got), len(want))
        pairs = [("%s[%d]" % (path, i), x, y) for i, (x, y) in enumerate(zip(want, got))]
    elif isinstance(want, str) and isinstance(got, str):
        ok = leaf_type(got) == want[1:] if want[0] == ":" else got == want
        return None if ok else "%s: got %s, want %s" % (path, got, want)
    else:
        return "%s: got %r, want %r" % (path, got, want)
    return next((bad for bad in (mismatch(x, y, where) for where, x, y in pairs) if bad), None)


def bad_floats(v, path=()):
    """the float leaves that are not finite, and those under a key that names a time (`ms` or `us` among its words, as in loop_ms,
    us_per_body, apply_us) that are not positive"""
    if isinstance(v, dict):
        return [b for k, x in v.items() for b in bad_floats(x, path + (k,))]
    if isinstance(v, list):
        return [b for x in v for b in bad_floats(x, path)]
    if isinstance(v, float):
        timed = any(w in ("ms", "us") for k in path for w in k.split("_"))
        if not math.isfinite(v) or (timed and v <= 0.0):
            return ["%s = %r" % (".".join(path), v)]
    return []
