"""The Chebyshev polynomial handle of PCG is the Chebyshev-smoothed V-cycle of one level: the same
histories, launches, byte model and apply, bit for bit, for every number of steps at which the two take different kernels (1:
the r update carries the r.z values; 2 and 3: the last poly_step_k does), on a grid of whole 64-row chunks and on one of 210
rows, which is no multiple of 64 or 256.  The same statement for the sweeps (precond "sgs" == "mg" and "mgfw" of one level) is
tests/test_gpu_mg_kernels.py's and tests/test_gpu_mg_fw_kernels.py's (launches, bytes, apply) and tests/test_gpu_mg.py's and
tests/test_gpu_mg_fw.py's (histories).  Also pinned here: how many levels each kind of handle answers for."""
import numpy as np
import pytest

import precond_ref
from sparsebench_amd import hostapi

pytestmark = pytest.mark.gpu

GRIDS = ((8, 8, 8), (5, 6, 7))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


@pytest.fixture(scope="module", params=GRIDS, ids=["%dx%dx%d" % g for g in GRIDS])
def problem(request, gpu):
    p = hostapi.Problem("generate", *request.param, fmt="scs", Cc=64, sigma=256)
    yield p
    p.free()


@pytest.mark.parametrize("steps", (1, 2, 3))
def test_the_polynomial_is_the_one_level_chebyshev_cycle(problem, steps):
    poly = hostapi.PCG(problem, precond="poly", steps=steps, ratio=4.0)
    one = hostapi.PCG(problem, precond="mgpoly", levels=1, steps=steps, ratio=4.0)
    assert poly.precond() == "poly" and one.precond() == "mgpoly" and poly.steps() == one.steps() == one.level_steps(0) == steps
    assert one.launches_per_body() == poly.launches_per_body()
    assert one.precond_bytes() == poly.precond_bytes()
    r = precond_ref.probe_vector(problem.nr, 7)
    assert same_bits(one.apply(r), poly.apply(r))
    assert one.solve(12, 0.0) == poly.solve(12, 0.0) == 12
    for a, b, what in zip(one.history(), poly.history(), ("rr", "rz", "pAp")):
        assert len(a) > 0 and same_bits(a, b), (what, a, b)
    one.free(), poly.free()


def test_levels_of_every_kind(problem):
    want = dict(jacobi=0, poly=0, sgs=1, mg=1, mgfw=1, mgpoly=1)
    for precond, levels in want.items():
        s = hostapi.PCG(problem, precond=precond, levels=1 if precond.startswith("mg") else None)
        assert s.precond() == precond and s.levels() == levels, (precond, s.levels())
        s.free()
