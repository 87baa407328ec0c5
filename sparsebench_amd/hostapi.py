"""Python mirror of the C host side (libsparsebench_host.so) for tests and bench.py.

`Problem` sequences what the C driver does -- matrixGenerate | MMMatrixRead ->
commPartition -> convertMatrix -- through the flat surface in host/sbh_flat.c, and
`CG` wraps the HIP layer's solveCG (sb_cg_*).  Plumbing only: no arithmetic happens in
Python, and nothing here falls back to the CPU.
"""
import ctypes as C
import math
import os
import shutil
import tempfile

import numpy as np

from . import capi

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB = os.path.join(HERE, "lib", "libsparsebench_host.so")
HOST_LIB_SP = os.path.join(HERE, "lib", "libsparsebench_host_sp.so")  # -DPRECISION=1: CG_FLOAT = float
vp = C.c_void_p
_host = None
_host_sp = None

# setup-exchange callbacks (include/sparsebench/sparsebench.h: sbh_exchange)
ALLGATHER_FN = C.CFUNCTYPE(None, vp, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int))
ALLTOALLV_FN = C.CFUNCTYPE(None, vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                           C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int))


class ExchangeS(C.Structure):
    _fields_ = [("ctx", vp), ("allgather_ints", ALLGATHER_FN), ("alltoallv_ints", ALLTOALLV_FN)]


def host(precision="double"):
    """the C host library: libsparsebench_host.so, or (precision="single") libsparsebench_host_sp.so -- both can be loaded in
    one process (the SP core binds its own calls to itself)"""
    global _host, _host_sp
    if precision not in ("double", "single"):
        raise ValueError("precision %r: expected 'double' or 'single'" % (precision,))
    if precision == "single" and _host_sp is not None:
        return _host_sp
    if precision == "double" and _host is not None:
        return _host
    capi.load()  # same libsbhip.so instance the host library links against
    path = HOST_LIB_SP if precision == "single" else HOST_LIB
    if not os.path.exists(path):
        raise RuntimeError("sparsebench_amd: %s is missing -- run `make host`" % path)
    H = C.CDLL(path)
    H.sbh_problem_create.restype = vp
    H.sbh_problem_create.argtypes = [C.c_char_p] + [C.c_int] * 9
    H.sbh_problem_matrix.restype = vp
    H.sbh_problem_matrix.argtypes = [vp]
    H.sbh_problem_halo.restype = vp
    H.sbh_problem_halo.argtypes = [vp]
    H.sbh_problem_setup_seconds.restype = C.c_double
    H.sbh_problem_setup_seconds.argtypes = [vp]
    H.sbh_problem_scalar.restype = C.c_uint
    H.sbh_problem_scalar.argtypes = [vp, C.c_int]
    H.sbh_problem_array.restype = vp
    H.sbh_problem_array.argtypes = [vp, C.c_int]
    H.sbh_problem_values.restype = vp
    H.sbh_problem_values.argtypes = [vp]
    H.sbh_problem_gm_entries.argtypes = [vp, vp, vp]
    H.sbh_convert_mtx_to_bmx.restype = None
    H.sbh_convert_mtx_to_bmx.argtypes = [C.c_char_p]
    H.sbh_problem_rhs.restype = C.c_int
    H.sbh_problem_rhs.argtypes = [vp, vp, vp]
    H.sbh_problem_free.argtypes = [vp]
    H.sbh_problem_create_csr.restype = vp
    H.sbh_problem_create_csr.argtypes = [C.c_uint, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]
    H.commSetExchange.argtypes = [vp]
    H.MMMatrixRead.argtypes = [vp, C.c_char_p]
    H.commDistributeMatrix.argtypes = [vp, vp, vp]
    H.sbh_exchange_rccl.restype = vp
    H.sbh_mg_levels.restype = C.c_int
    H.sbh_mg_levels.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    H.sbh_mg_f2c.restype = None
    H.sbh_mg_f2c.argtypes = [C.c_int, C.c_int, C.c_int, vp]
    H.sbh_mg_trilinear.restype = None
    H.sbh_mg_trilinear.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp]
    if precision == "single":
        _host_sp = H
    else:
        _host = H
    return H


_SCALARS = ["nr", "nc", "nnz", "nnzTrue", "totalNr", "totalNnz", "startRow", "stopRow", "C",
            "sigma", "nChunks", "nrPadded", "nElems", "externalCount", "totalSendCount",
            "indegree", "outdegree"]
_ARRAYS = {"rowPtr": 0, "rowNnz": 1, "crs_colInd": 2, "chunkPtr": 3, "chunkLens": 4,
           "scs_colInd": 5, "oldToNewPerm": 6, "newToOldPerm": 7, "elementsToSend": 8,
           "sources": 9, "recvCounts": 10, "rdispls": 11, "destinations": 12, "sendCounts": 13,
           "sdispls": 14, "externalGlobal": 15}


def mg_levels(nx, ny, nz, levels=None):
    """L of the geometric hierarchy of an nx x ny x nz grid (sbh_mg_levels): `levels`, or None for the deepest of up to 4 the
    grid allows.  L levels need every dimension divisible by 2^(L-1) and every coarse dimension >= 2: ValueError otherwise."""
    why = C.create_string_buffer(256)
    L = host().sbh_mg_levels(int(nx), int(ny), int(nz), 0 if levels is None else int(levels), why, 256)
    if levels is not None and int(levels) < 1:
        raise ValueError("MG: levels must be 1 or more, got %r" % (levels,))
    if not L:
        raise ValueError(why.value.decode())
    return L


def mg_f2c(nx, ny, nz):
    """the injection map of an nx x ny x nz grid (all even) onto the grid of half the size in every direction (sbh_mg_f2c):
    coarse point (x, y, z) is fine point (2x, 2y, 2z), both in the generator's numbering"""
    if nx % 2 or ny % 2 or nz % 2:
        raise ValueError("MG: the grid %d x %d x %d has an odd dimension" % (nx, ny, nz))
    out = np.empty((nx // 2) * (ny // 2) * (nz // 2), dtype=np.uint32)
    host().sbh_mg_f2c(int(nx), int(ny), int(nz), out.ctypes.data_as(vp))
    return out


def mg_trilinear(nx, ny, nz):
    """the trilinear prolongation of an nx x ny x nz grid (all even) from the grid of half the size in every direction
    (sbh_mg_trilinear) as a CSR triple (ptr uint64, col uint32, val float64) over the fine points, generator's numbering on both
    sides: weights 1, 1/2, 1/4, 1/8, the upper faces' missing neighbours dropped.  omega = 0.5 goes with it"""
    if nx % 2 or ny % 2 or nz % 2 or min(nx, ny, nz) < 2:
        raise ValueError("MG: the grid %d x %d x %d has an odd or empty dimension" % (nx, ny, nz))
    n = nx * ny * nz
    ptr, col, val = np.empty(n + 1, dtype=np.uint64), np.empty(8 * n, dtype=np.uint32), np.empty(8 * n, dtype=np.float64)
    host().sbh_mg_trilinear(int(nx), int(ny), int(nz), ptr.ctypes.data_as(vp), col.ctypes.data_as(vp), val.ctypes.data_as(vp))
    nnz = int(ptr[n])
    return ptr, col[:nnz].copy(), val[:nnz].copy()


def _write_mtx(path, A):
    """a scipy CSR matrix as a general real Matrix Market file, entries in storage order, 17 significant digits: every double
    comes back bit for bit through Problem(path)"""
    with open(path, "w") as f:
        f.write("%%%%MatrixMarket matrix coordinate real general\n%d %d %d\n" % (A.shape[0], A.shape[1], A.nnz))
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        step = 1 << 20
        for a in range(0, A.nnz, step):
            f.write("".join("%d %d %.17g\n" % t for t in zip((rows[a:a + step] + 1).tolist(), (A.indices[a:a + step] + 1).tolist(),
                                                              A.data[a:a + step].tolist())))


def galerkin_product(problem, P, n_coarse=None):
    """A_c = P^T A P of an uploaded double-precision one-rank problem, formed on the device (sb_matrix_galerkin): P a
    scipy.sparse matrix or a (ptr, col, val) CSR triple of nr x n_c, original numbering on both sides (n_coarse: n_c of a triple
    whose last coarse columns no row touches; None: its largest column + 1).  Returns ((ptr uint64, col
    uint32, val float64) in the coarse level's original numbering, columns ascending, exact zeros dropped, and the stats dict)"""
    if getattr(problem, "precision", "double") != "double":
        raise ValueError("galerkin_product: double precision only (the problem was built with precision=%r)" % (problem.precision,))
    if problem.nr != problem.totalNr:
        raise ValueError("galerkin_product runs on one rank")
    if not problem.upload:
        raise ValueError("galerkin_product reads the uploaded matrix: the problem was built with upload=False")
    if n_coarse is not None:
        nc = int(n_coarse)
    elif hasattr(P, "tocsr"):
        nc = P.shape[1]
    else:
        try:
            nc = int(np.max(P[1])) + 1 if len(P[1]) else 1
        except (TypeError, ValueError, IndexError):
            raise ValueError("P of level 0 must be a scipy.sparse matrix or a (ptr, col, val) triple")
    return _galerkin_product(problem, P, nc)


def _galerkin_product(problem, P, nc):
    ptr, col, val = _p_triple(P, problem.nr, int(nc), 0)
    L = capi.load()
    h = L.sb_matrix_galerkin(problem.matrix, int(nc), ptr.ctypes.data_as(vp), col.ctypes.data_as(vp), val.ctypes.data_as(vp))
    try:
        n, nnz = L.sb_csr_rows(h), L.sb_csr_nnz(h)
        out = (np.empty(n + 1, dtype=np.uint64), np.empty(nnz, dtype=np.uint32), np.empty(nnz, dtype=np.float64))
        st = np.zeros(6)
        L.sb_csr_copy(h, *[a.ctypes.data_as(vp) for a in out])
        L.sb_csr_stats(h, st.ctypes.data_as(vp))
    finally:
        L.sb_csr_free(h)
    return out, {"stage1_ms": float(st[0]), "stage2_ms": float(st[1]), "t_entries": int(st[2]), "dropped": int(st[3]),
                 "max_row_t": int(st[4]), "max_row_ac": int(st[5])}


def mg_galerkin(problem, levels=None, directory=None, _owned=None, product="scipy"):
    """the Galerkin hierarchy of a generated problem for PCG(precond="mgpoly", coarse=...): [(Problem, P, 1.0), ...] with the
    trilinear P per level and A_{l+1} = P_l^T A_l P_l, formed by scipy.sparse in CSR with sorted columns and exact zeros dropped,
    written with 17 significant digits as level<l>.mtx into `directory` (None: a new temporary one) and opened as Problems of the
    fine problem's format, C and sigma.  omega is 1.0: scaling A_c and the restriction together cancels in the cycle.  The caller
    frees the problems and removes the files (PCG(galerkin=True) does both with the handle).  ImportError without scipy.
    product="device": the same list with every A_{l+1} formed on the device from level l's uploaded matrix (galerkin_product,
    DESIGN 4.17) and opened with Problem.from_csr -- no scipy, no files, no directory; each Problem carries the product's stats as
    `galerkin_stats` (PCG(galerkin="device") frees the problems with the handle)."""
    if product not in ("scipy", "device"):
        raise ValueError("product must be 'scipy' or 'device', got %r" % (product,))
    if product == "device":
        if directory is not None:
            raise ValueError("product='device' writes no files: it takes no directory")
        return _mg_galerkin_device(problem, levels, _owned)
    try:
        import scipy.sparse as sp
    except ImportError:
        raise ImportError("mg_galerkin forms P^T A P with scipy.sparse, and scipy is not installed")
    name = getattr(problem, "filename", None)
    if name not in ("generate", "generate7P"):
        raise ValueError("mg_galerkin needs the grid: %r is not a generated problem" % (name,))
    if problem.nr != problem.totalNr:
        raise ValueError("mg_galerkin runs on one rank")
    if getattr(problem, "precision", "double") != "double":
        raise ValueError("mg_galerkin: double precision only (the problem was built with precision=%r)" % (problem.precision,))
    dims = problem.dims
    nlev = mg_levels(*dims, levels=levels)
    if directory is None:
        directory = tempfile.mkdtemp(prefix="sb_galerkin_")
    col, val = problem.gm_entries()
    A = sp.csr_matrix((val.astype(np.float64), col.astype(np.int64), problem.array("rowPtr").astype(np.int64)),
                      shape=(problem.nr, problem.nr))
    out = []
    for l in range(nlev - 1):
        triple = mg_trilinear(*dims)
        nf = dims[0] * dims[1] * dims[2]
        dims = tuple(d // 2 for d in dims)
        P = sp.csr_matrix((triple[2], triple[1].astype(np.int64), triple[0].astype(np.int64)), shape=(nf, nf // 8))
        A = (P.T.tocsr() @ A @ P).tocsr()
        A.sum_duplicates()
        A.eliminate_zeros()
        A.sort_indices()
        path = os.path.join(os.fspath(directory), "level%d.mtx" % (l + 1))
        _write_mtx(path, A)
        q = Problem(path, fmt=problem.fmt, Cc=problem.Cc, sigma=problem.sigma_arg, upload=problem.upload)
        if _owned is not None:
            _owned.append(q)
        out.append((q, triple, 1.0))
    return out


def _mg_galerkin_device(problem, levels, _owned):
    name = getattr(problem, "filename", None)
    if name not in ("generate", "generate7P"):
        raise ValueError("mg_galerkin needs the grid: %r is not a generated problem" % (name,))
    if problem.nr != problem.totalNr:
        raise ValueError("mg_galerkin runs on one rank")
    if getattr(problem, "precision", "double") != "double":
        raise ValueError("mg_galerkin: double precision only (the problem was built with precision=%r)" % (problem.precision,))
    if not problem.upload:
        raise ValueError("mg_galerkin(product='device') reads the uploaded matrices: the problem was built with upload=False")
    dims = problem.dims
    nlev = mg_levels(*dims, levels=levels)
    out, fine = [], problem
    for _ in range(nlev - 1):
        triple = mg_trilinear(*dims)
        dims = tuple(d // 2 for d in dims)
        (ptr, col, val), stats = _galerkin_product(fine, triple, dims[0] * dims[1] * dims[2])
        q = Problem.from_csr(ptr, col, val, fmt=problem.fmt, Cc=problem.Cc, sigma=problem.sigma_arg)
        q.galerkin_stats = stats
        if _owned is not None:
            _owned.append(q)
        out.append((q, triple, 1.0))
        fine = q
    return out


def _need_device_matrix(problem, who):
    if getattr(problem, "precision", "double") != "double":
        raise ValueError("%s: double precision only (the problem was built with precision=%r)" % (who, problem.precision))
    if problem.nr != problem.totalNr:
        raise ValueError("%s runs on one rank" % who)
    if not problem.upload:
        raise ValueError("%s reads the uploaded matrix: the problem was built with upload=False" % who)


def _theta(theta, who):
    if isinstance(theta, bool) or not isinstance(theta, (int, float, np.integer, np.floating)) or not 0.0 <= float(theta) < math.inf:
        raise ValueError("%s: theta must be finite and not negative, got %r" % (who, theta))
    return float(theta)


def _omega_s(omega_s, who):
    if isinstance(omega_s, bool) or not isinstance(omega_s, (int, float, np.integer, np.floating)) or not 0.0 <= float(omega_s) < math.inf:
        raise ValueError("%s: omega_s must be finite and not negative, got %r" % (who, omega_s))
    return float(omega_s)


def aggregate(problem, theta=0.0):
    """the aggregates of an uploaded double-precision one-rank problem, made on the device from the matrix alone
    (sb_matrix_aggregate): (agg int32 per row in original numbering, -1 for a row without a strong entry; the number
    of aggregates; the rounds the independent set took)"""
    _need_device_matrix(problem, "aggregate")
    theta = _theta(theta, "aggregate")
    agg, n_agg, rounds = np.empty(problem.nr, dtype=np.int32), C.c_uint32(0), C.c_uint32(0)
    capi.load().sb_matrix_aggregate(problem.matrix, theta, agg.ctypes.data_as(vp), C.byref(n_agg), C.byref(rounds))
    return agg, int(n_agg.value), int(rounds.value)


def sa_prolongation(problem, theta=0.0, omega_s=4.0 / 3.0, lmax=None, stats=False):
    """the smoothed-aggregation prolongation P = T - (omega_s / lmax) D^-1 A T of such a problem (sb_matrix_sa_prolongation, DESIGN
    4.19): ((ptr uint64, col uint32, val float64) of nr x n_agg in original numbering, columns ascending; n_agg).  lmax None: the
    row-sum bound of D^-1/2 A D^-1/2; omega_s = 0: the tentative 0/1 prolongator.  stats=True adds the dict of device times and
    counts"""
    _need_device_matrix(problem, "sa_prolongation")
    theta, omega_s = _theta(theta, "sa_prolongation"), _omega_s(omega_s, "sa_prolongation")
    if lmax is not None and not (0.0 < float(lmax) < math.inf):
        raise ValueError("lmax must be finite and positive (None: the row-sum bound), got %r" % (lmax,))
    L = capi.load()
    n_agg = C.c_uint32(0)
    h = L.sb_matrix_sa_prolongation(problem.matrix, theta, omega_s, 0.0 if lmax is None else float(lmax), C.byref(n_agg))
    try:
        n, nnz = L.sb_csr_rows(h), L.sb_csr_nnz(h)
        out = (np.empty(n + 1, dtype=np.uint64), np.empty(nnz, dtype=np.uint32), np.empty(nnz, dtype=np.float64))
        st = np.zeros(6)
        L.sb_csr_copy(h, *[a.ctypes.data_as(vp) for a in out])
        L.sb_csr_stats(h, st.ctypes.data_as(vp))
    finally:
        L.sb_csr_free(h)
    if stats:
        return out, int(n_agg.value), {"aggregate_ms": float(st[0]), "product_ms": float(st[1]), "smooth_ms": float(st[2]),
                                       "rounds": int(st[3]), "strong_entries": int(st[4]), "max_row_p": int(st[5])}
    return out, int(n_agg.value)


MG_AGGREGATION_DEPTH = 4    # levels at most, the fine one included
MG_AGGREGATION_COARSEST = 64  # a level of at most this many rows is the last


def mg_aggregation(problem, levels=None, theta=0.0, omega_s=4.0 / 3.0, _owned=None):
    """the smoothed-aggregation hierarchy of ANY uploaded double-precision one-rank problem for PCG(precond="mgpoly", coarse=...):
    [(Problem, P, 1.0), ...] with P_l = sa_prolongation(level l) and A_{l+1} = P_l^T A_l P_l formed on the device
    (galerkin_product), opened with Problem.from_csr in the fine problem's format, C and sigma.  Stops at `levels`
    levels (None: 4) or at the first level of at most 64 rows.  A level that coarsens by less than 2 is refused by name (a level
    without a root by the library).  Each Problem carries `aggregation_stats` (the level above's rounds and times) and
    `galerkin_stats`; the caller frees the problems (PCG(coarsening="aggregation") does with the handle)."""
    _need_device_matrix(problem, "mg_aggregation")
    if levels is not None and (isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1):
        raise ValueError("MG: levels must be 1 or more, got %r" % (levels,))
    theta, omega_s = _theta(theta, "mg_aggregation"), _omega_s(omega_s, "mg_aggregation")
    depth = MG_AGGREGATION_DEPTH if levels is None else int(levels)
    out, fine = [], problem
    while len(out) + 1 < depth and fine.nr > MG_AGGREGATION_COARSEST:
        l = len(out)
        P, n_agg, st = sa_prolongation(fine, theta, omega_s, stats=True)
        if 2 * n_agg > fine.nr:
            raise ValueError("mg_aggregation: level %d: %d aggregates of %d rows: the level coarsens by less than 2 (theta = %r)"
                             % (l, n_agg, fine.nr, theta))
        (ptr, col, val), gst = _galerkin_product(fine, P, n_agg)
        q = Problem.from_csr(ptr, col, val, fmt=problem.fmt, Cc=problem.Cc, sigma=problem.sigma_arg)
        q.aggregation_stats, q.galerkin_stats = st, gst
        if _owned is not None:
            _owned.append(q)
        out.append((q, P, 1.0))
        fine = q
    return out


def _omega(omega, l):
    if not (isinstance(omega, (int, float)) and np.isfinite(omega) and omega > 0.0):
        raise ValueError("omega of level %d must be finite and positive, got %r" % (l, omega))
    return float(omega)


def _p_triple(P, n_fine, n_coarse, l):
    """a prolongation as contiguous (ptr uint64, col uint32, val float64): a scipy.sparse matrix (its CSR form, entries as
    stored) or a (ptr, col, val) triple; the shape is checked here, the contents by the library"""
    if hasattr(P, "tocsr"):
        if P.shape != (n_fine, n_coarse):
            raise ValueError("P of level %d must be %d x %d, got %r" % (l, n_fine, n_coarse, P.shape))
        P = P.tocsr()
        P = (P.indptr, P.indices, P.data)
    try:
        ptr, col, val = P
    except (TypeError, ValueError):
        raise ValueError("P of level %d must be a scipy.sparse matrix or a (ptr, col, val) triple" % l)
    if np.any(np.asarray(ptr) < 0) or np.any(np.asarray(col) < 0):
        raise ValueError("P of level %d has a negative pointer or column" % l)
    ptr, col = np.ascontiguousarray(ptr, dtype=np.uint64), np.ascontiguousarray(col, dtype=np.uint32)
    val = np.ascontiguousarray(val, dtype=np.float64)
    if ptr.shape != (n_fine + 1,):
        raise ValueError("P of level %d must have %d row pointers (level %d has %d rows), got %r" % (l, n_fine + 1, l, n_fine, ptr.shape))
    if col.ndim != 1 or col.shape != val.shape or int(ptr.max()) > len(col):
        raise ValueError("P of level %d: %d columns, %d weights, row pointers up to %d" % (l, col.size, val.size, int(ptr.max())))
    return ptr, col, val


def convert_mtx_to_bmx(path):
    """file.mtx -> file.bmx next to it (the driver's -c option); SB_BMX_FP64=1 keeps fp64 values"""
    host().sbh_convert_mtx_to_bmx(os.fspath(path).encode())
    return os.path.splitext(os.fspath(path))[0] + ".bmx"


def read_bmx_slice(path, rank=0, size=1):
    """rank's row slice of a .bmx file as (startRow, rowPtr, col, val), global column ids"""
    H = host()
    H.sbh_bmx_read.restype = vp
    H.sbh_bmx_read.argtypes = [C.c_char_p, C.c_int, C.c_int]
    H.sbh_gm_scalar.restype = C.c_uint
    H.sbh_gm_scalar.argtypes = [vp, C.c_int]
    H.sbh_gm_copy.argtypes = [vp, vp, vp, vp]
    H.sbh_gm_free.argtypes = [vp]
    g = H.sbh_bmx_read(os.fspath(path).encode(), rank, size)
    nr, nnz, start = (H.sbh_gm_scalar(g, i) for i in range(3))
    rp, col, val = np.empty(nr + 1, np.uint32), np.empty(nnz, np.uint32), np.empty(nnz, np.float64)
    H.sbh_gm_copy(g, rp.ctypes.data_as(vp), col.ctypes.data_as(vp), val.ctypes.data_as(vp))
    H.sbh_gm_free(g)
    return start, rp, col, val


def _view(ptr, n, dtype):
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    ct = {np.uint32: C.c_uint32, np.int32: C.c_int32, np.float64: C.c_double, np.float32: C.c_float}[dtype]
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(int(n),))


class Problem:
    """One rank's matrix: generated HPCG stencil or a .mtx file, partitioned, converted
    and (upload=True) resident in HBM."""

    def __init__(self, filename="generate", nx=16, ny=16, nz=16, fmt="scs", Cc=64, sigma=1,
                 rank=0, size=1, upload=True, precision="double", mirror=None):
        # precision="single": the SP host library (CG_FLOAT = float, the _f32 entry points of the HIP layer)
        # mirror (single precision only): None = the process default (sb_sp_mirror, SB_SP_MIRROR); True / False = the SP
        # mirror switch set around the upload and put back afterwards
        if mirror is not None and precision != "single":
            if mirror:
                raise ValueError("mirror=True is the single-precision mirror switch; a double-precision matrix builds its mirror anyway")
            mirror = None
        self.H = host(precision)
        self.precision = precision
        self.fdtype = np.float32 if precision == "single" else np.float64
        self.fmt = fmt
        self.upload = upload
        self.rank, self.size = int(rank), int(size)
        # what a geometric hierarchy is regenerated from (PCG(precond="mg", levels=...))
        self.filename, self.dims, self.Cc, self.sigma_arg = os.fsdecode(filename), (int(nx), int(ny), int(nz)), Cc, sigma
        L = capi.load()
        old = L.sb_sp_mirror() if mirror is not None else None
        if mirror is not None:
            L.sb_set_sp_mirror(1 if mirror else 0)
        try:
            self.ptr = self.H.sbh_problem_create(os.fsencode(filename), nx, ny, nz,
                                                 0 if fmt == "crs" else 1, Cc, sigma, rank, size,
                                                 1 if upload else 0)
        finally:
            if mirror is not None:
                L.sb_set_sp_mirror(old)
        for i, name in enumerate(_SCALARS):
            setattr(self, name, int(self.H.sbh_problem_scalar(self.ptr, i)))

    @classmethod
    def from_csr(cls, ptr, col, val, fmt="scs", Cc=64, sigma=1, upload=True):
        """a one-rank double-precision Problem from CSR in memory (sbh_problem_create_csr): the layout, array for array, that
        Problem(file.mtx) gives for the same entries; filename "memory".  upload=False: the host layout only, no GPU"""
        ptr = np.ascontiguousarray(ptr, dtype=np.uint64)
        col = np.ascontiguousarray(col, dtype=np.uint32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        if ptr.ndim != 1 or len(ptr) < 1 or col.shape != val.shape or col.ndim != 1 or int(ptr[-1]) != len(col) or int(ptr[0]) != 0:
            raise ValueError("from_csr: %d row pointers from %r to %r, %d columns, %d values"
                             % (len(ptr), ptr[:1].tolist(), ptr[-1:].tolist(), col.size, val.size))
        if len(col) and int(col.max()) >= len(ptr) - 1:
            raise ValueError("from_csr: column %d is outside the %d rows" % (int(col.max()), len(ptr) - 1))
        self = cls.__new__(cls)
        self.H = host("double")
        self.precision, self.fdtype, self.fmt, self.upload = "double", np.float64, fmt, upload
        self.filename, self.dims, self.Cc, self.sigma_arg = "memory", (1, 1, 1), Cc, sigma
        self.rank, self.size = 0, 1
        self.ptr = self.H.sbh_problem_create_csr(len(ptr) - 1, ptr.ctypes.data_as(vp), col.ctypes.data_as(vp), val.ctypes.data_as(vp),
                                                 0 if fmt == "crs" else 1, Cc, sigma, 1 if upload else 0)
        for i, name in enumerate(_SCALARS):
            setattr(self, name, int(self.H.sbh_problem_scalar(self.ptr, i)))
        return self

    def array(self, name):
        n = {"rowPtr": self.nr + 1, "rowNnz": self.nr, "crs_colInd": self.nnzTrue,
             "chunkPtr": self.nChunks + 1, "chunkLens": self.nChunks, "scs_colInd": self.nElems,
             "oldToNewPerm": self.nr, "newToOldPerm": self.nr,
             "elementsToSend": self.totalSendCount, "sources": self.indegree,
             "recvCounts": self.indegree, "rdispls": self.indegree,
             "destinations": self.outdegree, "sendCounts": self.outdegree,
             "sdispls": self.outdegree, "externalGlobal": self.externalCount}[name]
        dt = np.int32 if name in ("elementsToSend", "sources", "recvCounts", "rdispls",
                                  "destinations", "sendCounts", "sdispls") else np.uint32
        return _view(self.H.sbh_problem_array(self.ptr, _ARRAYS[name]), n, dt)

    def values(self):
        n = self.nnzTrue if self.fmt == "crs" else self.nElems
        return _view(self.H.sbh_problem_values(self.ptr), n, self.fdtype)

    def gm_entries(self):
        col = np.empty(self.nnzTrue, dtype=np.uint32)
        val = np.empty(self.nnzTrue, dtype=self.fdtype)
        self.H.sbh_problem_gm_entries(self.ptr, col.ctypes.data_as(vp), val.ctypes.data_as(vp))
        return col, val

    def rhs(self):
        b = np.empty(self.nr, dtype=self.fdtype)
        xe = np.empty(self.nr, dtype=self.fdtype)
        gen = self.H.sbh_problem_rhs(self.ptr, b.ctypes.data_as(vp), xe.ctypes.data_as(vp))
        return b, (xe if gen else None)

    @property
    def matrix(self):
        return self.H.sbh_problem_matrix(self.ptr)

    @property
    def halo(self):
        return self.H.sbh_problem_halo(self.ptr)

    @property
    def setup_seconds(self):
        return self.H.sbh_problem_setup_seconds(self.ptr)

    def spmv_bytes(self):
        """algorithmic bytes of one SpMV in the reference's layout"""
        return capi.load().sb_matrix_spmv_bytes(self.matrix)

    def stream_bytes(self):
        """bytes the selected kernel really moves (compressed mirror, if in use)"""
        return capi.load().sb_matrix_stream_bytes(self.matrix)

    def use_packed(self, mode):
        capi.load().sb_matrix_use_packed(self.matrix, int(mode))
        return capi.load().sb_matrix_packed_mode(self.matrix)

    def resident_share(self, k=-1):
        """sixteenths of the Sell-64 stream that the reference-layout kernel keeps in the Infinity Cache across SpMVs
        (sb_matrix_resident_share): -1 = the upload's rule, 0 ... 16 = forced.  Returns the share in force."""
        return capi.load().sb_matrix_resident_share(self.matrix, int(k))

    def placement_report(self):
        """what the upload's placement tuner saw (us of a proxy loop body: p update | SpMV on the reference-layout stream | r update):
        with the first vectors' arena tried and the stream where hipMalloc put it, at the pair kept, at the slowest pair; None if
        it did not run (SB_PLACE=0, or a stream below 64 MB)"""
        us = (C.c_float * 3)()
        n = capi.load().sb_matrix_placement_report(self.matrix, us)
        return {"probes_timed": n, "us_first_pair": round(us[0], 2), "us_kept": round(us[1], 2), "us_slowest": round(us[2], 2)} if n else None

    def all_row_programs(self):
        """1: every chunk is a row program with a mapped or simple window (sb_matrix_all_row_programs)"""
        return capi.load().sb_matrix_all_row_programs(self.matrix)

    def pack_info(self):
        L = capi.load()
        uni = C.c_uint32(0)
        pats = L.sb_matrix_row_patterns(self.matrix, C.byref(uni))
        return {"level": L.sb_matrix_pack_level(self.matrix), "mode": L.sb_matrix_packed_mode(self.matrix),
                "row_patterns": pats, "uniform_chunks": uni.value,
                "lds_window_doubles": L.sb_matrix_lds_window(self.matrix),
                "pattern_classes": L.sb_matrix_pattern_classes(self.matrix)}

    def free(self):
        if self.ptr:
            self.H.sbh_problem_free(self.ptr)
            self.ptr = None


class CG:
    """solveCG on the GPU (sb_cg_*): state in HBM, loop without host round trips."""

    def __init__(self, problem, fused=True, graph=False, fuse_p=-1, fuse_alpha=-1, fuse_beta=-1, dot_order=None):
        self.L = capi.load()
        self.problem = problem
        b, xe = problem.rhs()
        # the solver follows the matrix's precision (sb_matrix_precision: 1 single, 2 double)
        self.single = self.L.sb_matrix_precision(problem.matrix) == 1
        create = self.L.sb_cg_create_f32 if self.single else self.L.sb_cg_create
        self.ptr = create(problem.matrix, problem.halo, b.ctypes.data_as(vp),
                          xe.ctypes.data_as(vp) if xe is not None else None)
        # fused: True = the default (1: dots fused into their producers), False = the reference's op list, or the
        # level itself (0 or 1; any other non-zero level is 1)
        self.L.sb_cg_set_fused(self.ptr, int(fused))
        self.L.sb_cg_set_graph(self.ptr, int(graph))
        self.L.sb_cg_set_fuse_p(self.ptr, int(fuse_p))  # -1: default; 1 / 0: the p update inside the SpMV where possible / not
        self.L.sb_cg_set_fuse_alpha(self.ptr, int(fuse_alpha))  # -1: default; 1 / 0: the alpha step inside the r update (one rank) / not
        self.L.sb_cg_set_fuse_beta(self.ptr, int(fuse_beta))  # the beta step at the head of the p update where that is a launch of its own
        if dot_order is not None:  # None: the process default (sb_dot_order, SB_DOT_ORDER)
            self.set_dot_order(dot_order)
        self.itermax = 0

    DOT_ORDERS = {"tree": 0, "seq": 1, None: -1}

    def set_dot_order(self, order):
        """"tree" / 0: the fixed tree order; "seq" / 1: the reference's sequential sum (validation, the reference's op
        list); None / -1: the process default.  Takes effect with the next solve / start."""
        code = self.DOT_ORDERS[order] if order in self.DOT_ORDERS else int(order)
        if code not in (-1, 0, 1):
            raise ValueError("dot_order %r: expected 'tree', 'seq' or None" % (order,))
        self.L.sb_cg_set_dot_order(self.ptr, code)

    def dot_order(self):
        """"tree" or "seq": the order the solve uses"""
        return "seq" if self.L.sb_cg_dot_order(self.ptr) else "tree"

    def vector_phase(self):
        """always 0: the solver uses the separate launches (the one-launch vector phase was removed)"""
        return self.L.sb_cg_vector_phase(self.ptr)

    def launches_per_body(self):
        return self.L.sb_cg_launches_per_body(self.ptr)

    def fuse_p(self):
        """1: the loop takes the p update inside the SpMV launch"""
        return self.L.sb_cg_fuse_p(self.ptr)

    def halo_fold(self):
        """1: the next solve sends its halo from the p update and receives it in the SpMV (sb_comm_halo_fold), 0: today's body"""
        return self.L.sb_cg_halo_fold(self.ptr)

    def collectives_per_body(self):
        return self.L.sb_cg_collectives_per_body(self.ptr)

    def solve(self, itermax=150, eps=0.0):
        self.itermax = itermax
        return self.L.sb_cg_solve(self.ptr, itermax, eps)

    def start(self, itermax, eps=0.0):
        """prologue only; follow with run_iters() and finish()"""
        self.itermax = itermax
        self.L.sb_cg_start(self.ptr, itermax, eps)

    def run_iters(self, iters):
        self.L.sb_cg_run_iters(self.ptr, iters)

    def finish(self):
        return self.L.sb_cg_finish(self.ptr)

    def history(self):
        cap = self.itermax + 2
        rr = np.zeros(cap)
        pap = np.zeros(cap)
        npap = C.c_int(0)
        nrr = self.L.sb_cg_history(self.ptr, rr.ctypes.data_as(vp), cap, pap.ctypes.data_as(vp),
                                   cap, C.byref(npap))
        return rr[:nrr].copy(), pap[:npap.value].copy()

    def solution(self):
        """x in original row order: float64, or float32 for a single-precision solver"""
        if self.single:
            x = np.empty(self.problem.nr, dtype=np.float32)
            self.L.sb_cg_solution_f32(self.ptr, x.ctypes.data_as(vp))
            return x
        x = np.empty(self.problem.nr)
        self.L.sb_cg_solution(self.ptr, x.ctypes.data_as(vp))
        return x

    def check_residual(self):
        return self.L.sb_cg_check_residual(self.ptr)

    def counters(self):
        out = (C.c_int * 5)()
        self.L.sb_cg_counters(self.ptr, out)
        return dict(zip(["stop", "stop_next", "iters", "n_rr", "n_pAp"], list(out)))

    def spmv_timing(self, on):
        self.L.sb_cg_spmv_timing(self.ptr, int(on))

    def spmv_ms(self):
        n = C.c_int(0)
        ms = self.L.sb_cg_spmv_ms(self.ptr, C.byref(n))
        return ms, n.value

    PHASES = ("p_update", "halo", "spmv", "alpha_step", "r_update", "beta_step", "dot_pass")

    def phase_timing(self, on):
        self.L.sb_cg_phase_timing(self.ptr, int(on))

    def phase_us(self):
        """{phase: (mean microseconds per occurrence, occurrences)} since phase_timing(True)"""
        ms, cnt = (C.c_double * 8)(), (C.c_int * 8)()
        n = self.L.sb_cg_phase_ms(self.ptr, ms, cnt)
        return {self.PHASES[i]: (1e3 * ms[i] / cnt[i], cnt[i]) for i in range(n) if cnt[i]}

    def loop_ms(self):
        return self.L.sb_cg_loop_ms(self.ptr)

    def region_ms(self):
        out = np.zeros(4)
        self.L.sb_cg_region_ms(self.ptr, out.ctypes.data_as(vp))
        return dict(zip(["waxpby", "spMVM", "ddot", "comm"], out))

    def free(self):
        if self.ptr:
            self.L.sb_cg_free(self.ptr)
            self.ptr = None


def _ptr(a):
    return a.ctypes.data_as(vp) if a is not None else None


class _Solver:
    """What GMRES, BatchCG, PCG and BiCGStab share: a handle of the C family PREFIX (sb_pcg_*, ...), refused for a
    single-precision problem before the library or the problem is touched.  A subclass's __init__ creates `ptr`."""

    PREFIX = NAME = None
    COUNTERS = ()

    def _need_double(self, problem):
        if getattr(problem, "precision", "double") != "double":
            raise ValueError("%s: double precision only (the problem was built with precision=%r)" % (self.NAME, problem.precision))

    def _open(self, problem):
        """the refusal, the library, and the problem's (b, xexact)"""
        self._need_double(problem)
        self.L = capi.load()
        self.problem = problem
        self.itermax = 0
        return problem.rhs()

    def _c(self, name):
        return getattr(self.L, "%s_%s" % (self.PREFIX, name))

    def _dinv_arg(self, dinv):
        if dinv is not None:
            dinv = np.ascontiguousarray(dinv, dtype=np.float64)
            if dinv.shape != (self.problem.nr,):
                raise ValueError("dinv must hold nr = %d doubles, got shape %r" % (self.problem.nr, dinv.shape))
        return dinv

    def _vector(self, name, *args):
        x = np.empty(self.problem.nr)
        self._c(name)(self.ptr, *args, x.ctypes.data_as(vp))
        return x

    def solve(self, itermax=150, eps=0.0):
        self.itermax = itermax
        return self._c("solve")(self.ptr, itermax, eps)

    def start(self, itermax, eps=0.0):
        """prologue only; follow with run_iters() and finish()"""
        self.itermax = itermax
        self._c("start")(self.ptr, itermax, eps)

    def finish(self):
        return self._c("finish")(self.ptr)

    def solution(self):
        """x in original row order"""
        return self._vector("solution")

    def check_residual(self):
        return self._c("check_residual")(self.ptr)

    def counters(self):
        out = (C.c_int * 5)()
        self._c("counters")(self.ptr, out)
        return dict(zip(self.COUNTERS, list(out)))

    def loop_ms(self):
        return self._c("loop_ms")(self.ptr)

    def free(self):
        if self.ptr:
            self._c("free")(self.ptr)
            self.ptr = None


class _BodySolver(_Solver):
    """the three whose loop is made of bodies (GMRES has steps: launches_per_step(j), run_steps())"""

    def launches_per_body(self):
        return self._c("launches_per_body")(self.ptr)

    def run_iters(self, iters):
        self._c("run_iters")(self.ptr, int(iters))


class _PlanBorrower:
    """What GMRES and BiCGStab share beside _Solver: a preconditioner taken from a `PCG` -- the caller's instance, BORROWED, or
    one built by name with PCG's own keyword arguments and freed with the handle."""

    PLANS = ("sgs", "mg", "mgfw", "poly", "mgpoly")

    def _check_precond(self, problem, precond, dinv, plan_args):
        """the refusals that need no library; True where precond is a PCG instance or a plan's name"""
        self._need_double(problem)
        self.pcg, self._owns_pcg, self._kind = None, False, None
        plan = isinstance(precond, PCG) or (isinstance(precond, str) and precond in self.PLANS)
        if plan and dinv is not None:
            raise ValueError("precond=%s takes no dinv: the preconditioner is the plan's"
                             % ("a PCG handle" if isinstance(precond, PCG) else repr(precond)))
        if isinstance(precond, PCG):
            if plan_args:
                raise ValueError("%s go with a precond given by name: a PCG handle brings its own" % ", ".join(sorted(plan_args)))
            if precond.ptr is None:
                raise ValueError("the PCG handle has been freed")
            if precond.problem is not problem:
                raise ValueError("the PCG handle was made over another problem: its preconditioner is that matrix's")
        elif not plan and plan_args:
            raise TypeError("%s: %s go with precond 'sgs', 'mg', 'mgfw', 'poly' or 'mgpoly' only" % (self.NAME, ", ".join(sorted(plan_args))))
        return plan

    def _take_pcg(self, problem, precond, plan_args):
        """the caller's PCG, or one of this handle's own by the name PCG knows it by"""
        if isinstance(precond, PCG):
            self.pcg = precond
        else:
            self.pcg, self._owns_pcg = PCG(problem, precond=precond, **plan_args), True

    def _drop_pcg(self):
        if self._owns_pcg and self.pcg is not None:
            self.pcg.free()
        self.pcg, self._owns_pcg = None, False

    def precond(self):
        """the kind's name: "none", "jacobi" or "caller" as the handle was made; under a plan "sgs", "mg", "mgfw", "poly" or
        "mgpoly" as the library reports it ("jacobi" for a borrowed diagonal PCG, whose dinv was copied)"""
        kind = self._c("precond")(self.ptr)
        return self.PLANS[kind - 1] if kind > 0 else (self._kind or "jacobi")

    def dinv(self):
        """the diagonal in use (a plan: level 0's), original row order"""
        return self._vector("dinv")

    def free(self):
        super().free()
        self._drop_pcg()


class GMRES(_PlanBorrower, _Solver):
    """restarted GMRES(m) on the GPU (sb_gmres_*): for matrices that are not symmetric positive definite.  Krylov basis and
    scalars in HBM, loop without host round trips; double precision, one rank.

    precond "none": no preconditioner (sb_gmres_create).  Anything else is RIGHT preconditioning, GMRES on A M^-1:
    "jacobi", or a `dinv` of nr finite non-zero doubles in original row order (precond is then "caller"), builds a diagonal PCG
    handle whose dinv is copied; a `PCG` instance is BORROWED -- over the same problem, outliving this handle, with no solve open
    when this one is made or started; "sgs", "mg", "mgfw", "poly" or "mgpoly" with PCG's own keyword arguments (levels, coarse,
    steps, lmax, ratio, coarse_steps, galerkin, coarsening, theta, omega_s) builds such a PCG of its own and frees it with
    itself.  A plan takes no dinv.  solution() is M^-1 u of the last cycle close; history() is unchanged in shape, its rr the
    explicit r.r of b - A M^-1 u."""

    PREFIX, NAME = "sb_gmres", "GMRES"
    COUNTERS = ("stop", "steps", "cycles", "n_res", "n_rr")

    def __init__(self, problem, restart=30, fused=True, precond="none", dinv=None, **plan_args):
        plan = self._check_precond(problem, precond, dinv, plan_args)
        if not plan:
            if dinv is not None:
                if precond not in ("none", "caller"):
                    raise ValueError("dinv is the caller's diagonal: it goes with no other precond, got %r" % (precond,))
                precond = "caller"
            if precond not in ("none", "jacobi", "caller") or (precond == "caller" and dinv is None):
                raise ValueError("precond must be 'none', 'jacobi', 'sgs', 'mg', 'mgfw', 'poly', 'mgpoly' or a PCG handle, or pass "
                                 "dinv; got %r" % (precond,))
            dinv = self._dinv_arg_of(problem, dinv)
            self._kind = precond
        if plan or precond == "jacobi":
            self._take_pcg(problem, precond, plan_args)
        b, xe = self._open(problem)
        args = (problem.matrix, problem.halo, _ptr(b), _ptr(xe), int(restart))
        if precond == "none":
            self.ptr = self.L.sb_gmres_create(*args)
        elif precond == "caller":  # entries of either sign: an entry point of its own
            self.ptr = self.L.sb_gmres_create_dinv(*args, _ptr(dinv))
        else:
            self.ptr = self.L.sb_gmres_create_pre(*args, self.pcg.ptr)
        if precond == "jacobi":  # a diagonal PCG handle: its dinv has been copied, so the handle goes at once
            self._drop_pcg()
        # fused: True = the multi-dot / multi-update kernels, False = the op list (one tree dot per h entry, one waxpby-shaped
        # launch per projection); same bits
        self.L.sb_gmres_set_fused(self.ptr, int(bool(fused)))

    @staticmethod
    def _dinv_arg_of(problem, dinv):
        if dinv is not None:
            dinv = np.ascontiguousarray(dinv, dtype=np.float64)
            if dinv.shape != (problem.nr,):
                raise ValueError("dinv must hold nr = %d doubles, got shape %r" % (problem.nr, dinv.shape))
            if not np.all(np.isfinite(dinv) & (dinv != 0.0)):
                raise ValueError("dinv: the preconditioner's entries must be finite and non-zero")
        return dinv

    def restart(self):
        return self.L.sb_gmres_restart(self.ptr)

    def launches_per_step(self, j):
        return self.L.sb_gmres_launches_per_step(self.ptr, int(j))

    def start(self, itermax, eps=0.0):
        """prologue only; follow with run_steps() and finish()"""
        _Solver.start(self, itermax, eps)

    def run_steps(self, steps):
        self.L.sb_gmres_run_steps(self.ptr, int(steps))

    def history(self):
        """(res_hist, rr_hist): the residual estimates (index 0: the initial norm) and every explicit r.r"""
        cap = self.itermax + 2
        res = np.zeros(cap)
        rr = np.zeros(cap)
        nrr = C.c_int(0)
        nres = self.L.sb_gmres_history(self.ptr, res.ctypes.data_as(vp), cap, rr.ctypes.data_as(vp), cap, C.byref(nrr))
        return res[:nres].copy(), rr[:nrr.value].copy()


def batch_rhs(b0, nrhs, start_row=0):
    """the right-hand sides of solveCGBatch: row 0 is b0; for c >= 1, b_c[i] = b0[i] + c * ((g(i) mod 5) - 2) with g the
    global row index (small integers: exact)"""
    b0 = np.asarray(b0, dtype=np.float64)
    g = (np.arange(len(b0), dtype=np.int64) + int(start_row)) % 5 - 2
    return np.stack([b0 + float(c) * g for c in range(int(nrhs))])


class BatchCG(_BodySolver):
    """nrhs independent CG solves on one pass over the matrix per loop body (sb_cgb_*): column c is bit for bit
    `CG` on b_c alone in the tree dot order.  B: an (nrhs, nr) array in original row order; None: `batch_rhs` of the problem's
    own right-hand side.  Double precision, one rank, nrhs in {2, 4, 8}."""

    PREFIX, NAME = "sb_cgb", "batched CG"
    COUNTERS = ("stop", "stop_next", "iters", "n_rr", "n_pAp")

    def __init__(self, problem, B=None, nrhs=4):
        b0, xe = self._open(problem)
        if B is None:
            B = batch_rhs(b0, nrhs, problem.startRow)
        else:
            B = np.ascontiguousarray(B, dtype=np.float64)
            if B.ndim != 2 or B.shape[1] != problem.nr:
                raise ValueError("B must be an (nrhs, nr) array, got shape %r" % (B.shape,))
            nrhs = B.shape[0]
            if xe is not None and not np.array_equal(B[0], b0):
                xe = None  # the exact solution belongs to the problem's own right-hand side
        self.nrhs = int(nrhs)
        B = np.ascontiguousarray(B, dtype=np.float64)
        self.ptr = self.L.sb_cgb_create(problem.matrix, problem.halo, self.nrhs, _ptr(B), _ptr(xe))

    def solve(self, itermax=150, eps=0.0):
        """returns the largest k_c"""
        return _Solver.solve(self, itermax, eps)

    def iterations(self, c):
        return self.L.sb_cgb_iterations(self.ptr, int(c))

    def history(self, c):
        cap = self.itermax + 2
        rr = np.zeros(cap)
        pap = np.zeros(cap)
        npap = C.c_int(0)
        nrr = self.L.sb_cgb_history(self.ptr, int(c), rr.ctypes.data_as(vp), cap, pap.ctypes.data_as(vp), cap, C.byref(npap))
        return rr[:nrr].copy(), pap[:npap.value].copy()

    def solution(self, c):
        """x_c in original row order"""
        return self._vector("solution", int(c))

    def check_residual(self, c=0):
        return self.L.sb_cgb_check_residual(self.ptr, int(c))

    def counters(self, c=-1):
        """column c: stop, stop_next, iters, n_rr, n_pAp; c = -1: all_stopped, columns_stopped, bodies_enqueued"""
        out = (C.c_int * 5)()
        self.L.sb_cgb_counters(self.ptr, int(c), out)
        if c < 0:
            return dict(zip(["all_stopped", "columns_stopped", "bodies_enqueued"], list(out)[:3]))
        return dict(zip(self.COUNTERS, list(out)))


class PCG(_BodySolver):
    """solveCG with a diagonal preconditioner put back (sb_pcg_*): z = r * dinv, alpha = r.z / p.Ap,
    beta = r.z / (r.z)_old, the loop test on sqrt(r.r).  dinv None: Jacobi, 1 / diag(A); else nr finite positive doubles in
    original row order (all 1.0: `CG` in the tree order bit for bit).  precond "sgs": symmetric Gauss-Seidel by multicolouring
    in place of the diagonal (takes no dinv).  precond "mg": a multigrid V-cycle with that smoother:
    `levels` for a generated problem's own geometric hierarchy (None: the deepest of up to 4 the grid allows), or
    `coarse=[(Problem, f2c), ...]` for the caller's.  precond "mgfw": that cycle with full-weighting transfers:
    `levels` for the generated hierarchy with the trilinear P and omega = 0.5, or `coarse=[(Problem, P, omega), ...]` with P a
    scipy.sparse matrix or a (ptr, col, val) CSR triple of n_l x n_{l+1}.  precond "poly": a Chebyshev polynomial in D^-1 A
    (DESIGN 4.15): `steps` terms (1 .. 16, default 3) on [lmax / ratio, lmax]; lmax None: the row-sum bound of D^-1/2 A D^-1/2,
    ratio default 16.0; takes no dinv.  precond "mgpoly": a V-cycle with that polynomial as the smoother of every level and mgfw's
    transfers: `steps` per smoothing (default 2), `coarse_steps` on the last level (default: steps), ratio default
    4.0, lmax None: every level's own bound; `levels` for the generated hierarchy with the trilinear P and omega = 0.25,
    `galerkin=True` for mg_galerkin's coarse operators in the regenerated ones' place (`galerkin="device"`: the same operators formed on
    the device, DESIGN 4.17: no scipy, no files), or `coarse` as "mgfw" takes it; `coarsening="aggregation"` (with `theta`, `omega_s`
    and `levels`) for mg_aggregation's hierarchy made from the matrix alone, on any problem.  Double
    precision, tree dot order.  One rank -- or, for "jacobi" (with or without a caller's dinv: the rank's nr local entries) and
    "poly" alone, a `Problem(..., rank=r, size=P)` of several: every call is then collective, steps, lmax and ratio
    are the same on every rank, and the other preconditioners raise ValueError before the library is touched."""

    PREFIX, NAME = "sb_pcg", "PCG"
    COUNTERS = ("stop", "stop_next", "iters", "n_rr", "n_pAp")

    def __init__(self, problem, dinv=None, precond="jacobi", levels=None, coarse=None, steps=None, lmax=None, ratio=None,
                 coarse_steps=None, galerkin=False, coarsening="geometric", theta=None, omega_s=None):
        self._need_double(problem)
        if getattr(problem, "size", 1) > 1 and precond in ("sgs", "mg", "mgfw", "mgpoly"):
            raise ValueError("PCG: precond=%r runs on one rank (the problem is rank %d of %d); 'jacobi' and 'poly' run on several"
                             % (precond, problem.rank, problem.size))
        if coarsening not in ("geometric", "aggregation"):
            raise ValueError("coarsening must be 'geometric' or 'aggregation', got %r" % (coarsening,))
        if coarsening == "aggregation":
            if precond != "mgpoly":
                raise ValueError("coarsening='aggregation' goes with precond='mgpoly' only")
            if galerkin or coarse is not None:
                raise ValueError("coarsening='aggregation' builds the hierarchy itself: it takes levels, not coarse or galerkin")
        elif theta is not None or omega_s is not None:
            raise ValueError("theta and omega_s go with coarsening='aggregation' only")
        if precond not in ("jacobi", "sgs", "mg", "mgfw", "poly", "mgpoly"):
            raise ValueError("precond must be 'jacobi' or 'sgs' or 'mg' or 'mgfw' or 'poly' or 'mgpoly', got %r" % (precond,))
        if precond not in ("poly", "mgpoly") and (steps is not None or lmax is not None or ratio is not None):
            raise ValueError("steps, lmax and ratio go with precond='poly' only, or with 'mgpoly'")
        if precond != "mgpoly" and (coarse_steps is not None or galerkin):
            raise ValueError("coarse_steps and galerkin go with precond='mgpoly' only")
        if precond == "poly":
            steps, lmax, ratio = self._poly_args(steps, lmax, ratio)
        poly = None
        if precond == "mgpoly":
            steps, lmax, ratio = self._poly_args(2 if steps is None else steps, lmax, 4.0 if ratio is None else ratio)
            cs = self._poly_args(steps if coarse_steps is None else coarse_steps, None, None, "coarse_steps")[0]
            poly = (steps, cs, lmax, ratio)
            if not isinstance(galerkin, (bool, np.bool_)) and not (isinstance(galerkin, str) and galerkin == "device"):
                raise ValueError("galerkin must be True or False, or 'device', got %r" % (galerkin,))
            if galerkin and coarse is not None:
                raise ValueError("galerkin=%r builds the coarse operators itself: it takes levels, not coarse"
                                 % (galerkin if isinstance(galerkin, str) else True,))
        if precond in ("sgs", "mg", "mgfw", "poly", "mgpoly") and dinv is not None:
            raise ValueError("precond=%r takes no dinv: its diagonal is the matrix's own" % (precond,))
        if precond not in ("mg", "mgfw", "mgpoly") and (levels is not None or coarse is not None):
            raise ValueError("levels and coarse go with precond='mg' only, or with 'mgfw' or 'mgpoly'")
        if levels is not None and coarse is not None:
            raise ValueError("precond='mg' takes levels (a generated problem's own hierarchy) or coarse (the caller's), not both")
        self._owned = []  # the coarse problems this handle generated itself
        self._owned_dir = None  # ... and the directory of the Galerkin operators' files
        self._keep = None
        if precond in ("mg", "mgfw", "mgpoly"):
            try:
                if coarsening == "aggregation":
                    found = mg_aggregation(problem, levels, 0.0 if theta is None else theta, 4.0 / 3.0 if omega_s is None else omega_s,
                                           _owned=self._owned)
                    self._create_mg_p(problem, found, "mgpoly", poly)
                elif galerkin:
                    self._create_galerkin(problem, levels, poly, device=isinstance(galerkin, str))
                else:
                    self._create_mg(problem, levels, coarse, precond != "mg", precond, poly)
            except Exception:
                self._free_owned()  # the coarse problems generated so far
                raise
            return
        b, xe = self._open(problem)
        if precond == "sgs":
            self.ptr = self.L.sb_pcg_create_sgs(problem.matrix, problem.halo, _ptr(b), _ptr(xe))
        elif precond == "poly":
            self.ptr = self.L.sb_pcg_create_poly(problem.matrix, problem.halo, _ptr(b), _ptr(xe), steps, lmax, ratio)
        else:
            self.ptr = self.L.sb_pcg_create(problem.matrix, problem.halo, _ptr(b), _ptr(xe), _ptr(self._dinv_arg(dinv)))

    def collectives_per_body(self):
        """communicator calls per loop body (sb_pcg_collectives_per_body); 0 on one rank"""
        return self.L.sb_pcg_collectives_per_body(self.ptr)

    @staticmethod
    def _poly_args(steps, lmax, ratio, what="steps"):
        """(steps, lmax, ratio) as sb_pcg_create_poly takes them (lmax 0.0: the bound), refused here where it would refuse them"""
        steps = 3 if steps is None else steps
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not 1 <= steps <= 16:
            raise ValueError("%s must be an integer from 1 to 16, got %r" % (what, steps))
        ratio = 16.0 if ratio is None else float(ratio)
        if not (1.0 < ratio < math.inf):
            raise ValueError("ratio (lmax / lmin) must be finite and greater than 1, got %r" % (ratio,))
        if lmax is not None and not (0.0 < float(lmax) < math.inf):
            raise ValueError("lmax must be finite and positive (None: the row-sum bound), got %r" % (lmax,))
        return int(steps), 0.0 if lmax is None else float(lmax), ratio

    def _create_mg(self, problem, levels, coarse, fw=False, precond="mg", poly=None):
        """coarse: [(Problem, f2c), ...], level l + 1's problem and the rows of level l that are its points (original numbering);
        else the geometric hierarchy of a generated problem at `levels` (None: the deepest of up to 4).  fw: (Problem, P, omega)
        triples and the trilinear P with omega = 0.5 in their place; poly (steps, coarse_steps, lmax, ratio): the
        Chebyshev-smoothed cycle on them, omega = 0.25"""
        if coarse is None:
            name = getattr(problem, "filename", None)
            if name not in ("generate", "generate7P"):
                raise ValueError("precond=%r needs the grid: %r is not a generated problem (pass coarse=[(Problem, %s), ...])"
                                 % (precond if fw else "mg", name, "P, omega" if fw else "f2c"))
            if problem.nr != problem.totalNr:
                raise ValueError("precond='mg' runs on one rank")
            dims = problem.dims
            nlev = mg_levels(*dims, levels=levels)
            coarse = []
            for _ in range(nlev - 1):
                transfer = (mg_trilinear(*dims), 0.25 if poly else 0.5) if fw else (mg_f2c(*dims),)
                dims = tuple(d // 2 for d in dims)
                q = Problem(name, *dims, fmt=problem.fmt, Cc=problem.Cc, sigma=problem.sigma_arg)
                self._owned.append(q)
                coarse.append((q,) + transfer)
        if fw:
            return self._create_mg_p(problem, coarse, precond, poly)
        maps = []
        for q, f2c in coarse:
            self._need_double(q)
            f2c = np.ascontiguousarray(f2c, dtype=np.uint32)
            if f2c.shape != (q.nr,):
                raise ValueError("f2c must hold the coarse problem's nr = %d rows, got shape %r" % (q.nr, f2c.shape))
            maps.append(f2c)
        b, xe = self._open(problem)
        n = len(coarse)
        mats = (vp * max(n, 1))(*[q.matrix for q, _ in coarse])
        ptrs = (vp * max(n, 1))(*[m.ctypes.data for m in maps])
        self._keep = (coarse, maps)  # the caller's coarse problems must outlive the handle, as the fine one must
        self.ptr = self.L.sb_pcg_create_mg(problem.matrix, problem.halo, _ptr(b), _ptr(xe), n, mats, ptrs)

    def _create_galerkin(self, problem, levels, poly, device=False):
        """mg_galerkin's hierarchy in a temporary directory that goes with the handle; device: formed on the device, no directory"""
        if device:
            coarse = mg_galerkin(problem, levels, _owned=self._owned, product="device")
        else:
            self._owned_dir = tempfile.mkdtemp(prefix="sb_galerkin_")
            coarse = mg_galerkin(problem, levels, self._owned_dir, _owned=self._owned)
        self._create_mg_p(problem, coarse, "mgpoly", poly)

    def _create_mg_p(self, problem, coarse, precond="mgfw", poly=None):
        ps, omegas, n_fine = [], [], problem.nr
        for l, item in enumerate(coarse):
            if not isinstance(item, (tuple, list)) or len(item) != 3:
                raise ValueError("precond=%r takes coarse=[(Problem, P, omega), ...]: entry %d is not such a triple" % (precond, l))
            q, P, omega = item
            self._need_double(q)
            omegas.append(_omega(omega, l))
            ps.append(_p_triple(P, n_fine, q.nr, l))
            n_fine = q.nr
        b, xe = self._open(problem)
        n = len(coarse)
        mats = (vp * max(n, 1))(*[item[0].matrix for item in coarse])
        arrs = [(vp * max(n, 1))(*[t[i].ctypes.data for t in ps]) for i in range(3)]
        om = np.array(omegas + [0.0], dtype=np.float64)
        self._keep = (coarse, ps)  # the caller's coarse problems must outlive the handle, as the fine one must
        if poly:
            self.ptr = self.L.sb_pcg_create_mg_poly(problem.matrix, problem.halo, _ptr(b), _ptr(xe), n, mats, arrs[0], arrs[1], arrs[2],
                                                    _ptr(om), *poly)
            return
        self.ptr = self.L.sb_pcg_create_mg_p(problem.matrix, problem.halo, _ptr(b), _ptr(xe), n, mats, arrs[0], arrs[1], arrs[2], _ptr(om))

    def mg_poly_probe(self, l, r, w, z, zc):
        """(rc, z_out) of the transfers of level l alone (sb_pcg_mg_poly_probe): rc = omega_l P_l^T (r - w), z_out = z + P_l zc;
        r, w, z in level l's original row order, zc in level l + 1's"""
        if self.precond() != "mgpoly" or not 0 <= int(l) < self.levels() - 1:
            raise ValueError("mg_poly_probe: level %r of a %r handle with %d levels has no transfers" % (l, self.precond(), self.levels()))
        nf, nc = self.level_rows(l), self.level_rows(l + 1)
        r, w, z, zc = (np.ascontiguousarray(v, dtype=np.float64) for v in (r, w, z, zc))
        if r.shape != (nf,) or w.shape != (nf,) or z.shape != (nf,) or zc.shape != (nc,):
            raise ValueError("r, w and z must hold %d doubles, zc %d" % (nf, nc))
        rc, zo = np.empty(nc), np.empty(nf)
        self.L.sb_pcg_mg_poly_probe(self.ptr, int(l), _ptr(r), _ptr(w), _ptr(z), _ptr(zc), _ptr(rc), _ptr(zo))
        return rc, zo

    def mg_fw_probe(self, l, r, z, zc):
        """(d, rc, z_out) of the transfers of level l alone (sb_pcg_mg_fw_probe): d = r - A_l z, rc = omega_l P_l^T d,
        z_out = z + P_l zc; r, z in level l's original row order, zc in level l + 1's"""
        nf, nc = self.level_rows(l), self.level_rows(l + 1)
        r, z, zc = (np.ascontiguousarray(v, dtype=np.float64) for v in (r, z, zc))
        if r.shape != (nf,) or z.shape != (nf,) or zc.shape != (nc,):
            raise ValueError("r and z must hold %d doubles, zc %d" % (nf, nc))
        d, rc, zo = np.empty(nf), np.empty(nc), np.empty(nf)
        self.L.sb_pcg_mg_fw_probe(self.ptr, int(l), _ptr(r), _ptr(z), _ptr(zc), _ptr(d), _ptr(rc), _ptr(zo))
        return d, rc, zo

    def _free_owned(self):
        for q in self._owned:
            q.free()
        self._owned = []
        if getattr(self, "_owned_dir", None):
            shutil.rmtree(self._owned_dir, ignore_errors=True)
            self._owned_dir = None

    def free(self):
        _BodySolver.free(self)
        self._free_owned()

    def precond(self):
        """"jacobi" (any diagonal), "sgs", "mg", "mgfw", "poly" or "mgpoly" """
        return ("jacobi", "sgs", "mg", "mgfw", "poly", "mgpoly")[self.L.sb_pcg_precond(self.ptr)]

    def steps(self):
        """steps of a polynomial handle or of a Chebyshev-smoothed cycle; 0 for the other kinds"""
        return self.L.sb_pcg_poly_steps(self.ptr)

    def _need_poly(self, what, l=None):
        """True on an "mgpoly" handle, whose queries take a level (default 0); a "poly" handle takes none"""
        mgp = self.precond() == "mgpoly"
        if self.steps() == 0 or (what == "rowbound" and mgp):
            raise ValueError("%s: the handle's preconditioner is %r, not 'poly'" % (what, self.precond()))
        if l is not None and not mgp:
            raise ValueError("%s: a level goes with precond='mgpoly' only" % what)
        if mgp and not 0 <= (0 if l is None else int(l)) < self.levels():
            raise ValueError("%s: level %r of a handle with %d levels" % (what, l, self.levels()))
        return mgp

    def level_steps(self, l):
        """steps of level l of an "mgpoly" handle: steps, on the last level coarse_steps"""
        self._need_poly("level_steps", l)
        return self.L.sb_pcg_mg_poly_level_steps(self.ptr, int(l))

    def interval(self, l=None):
        """(lmin, lmax) of a polynomial handle, or of level l of an "mgpoly" handle"""
        out = np.zeros(2)
        if self._need_poly("interval", l):
            self.L.sb_pcg_mg_poly_interval(self.ptr, int(l or 0), out.ctypes.data_as(vp))
        else:
            self.L.sb_pcg_poly_interval(self.ptr, out.ctypes.data_as(vp))
        return float(out[0]), float(out[1])

    def coeffs(self, l=None):
        """c1, then a_j, b_j for j = 2 .. steps: 2 steps - 1 doubles; of level l on an "mgpoly" handle"""
        if self._need_poly("coeffs", l):
            out = np.zeros(2 * self.level_steps(int(l or 0)) - 1)
            self.L.sb_pcg_mg_poly_coeffs(self.ptr, int(l or 0), out.ctypes.data_as(vp))
            return out
        out = np.zeros(2 * self.steps() - 1)
        self.L.sb_pcg_poly_coeffs(self.ptr, out.ctypes.data_as(vp))
        return out

    def rowbound(self):
        """g of the bound on lmax, original row order: the absolute row sums of D^-1/2 A D^-1/2"""
        self._need_poly("rowbound")
        return self._vector("poly_rowbound")

    def levels(self):
        """L of an MG handle; 1 for SGS, 0 for a diagonal one"""
        return self.L.sb_pcg_levels(self.ptr)

    def level_rows(self, l):
        return self.L.sb_pcg_level_rows(self.ptr, int(l))

    def level_colours(self, l):
        return self.L.sb_pcg_level_colours(self.ptr, int(l))

    def colours(self):
        """nC of an SGS handle; 0 for a diagonal one"""
        return self.L.sb_pcg_colours(self.ptr)

    def colouring(self):
        """the colour of every row, original row order (SGS handles)"""
        out = np.zeros(self.problem.nr, dtype=np.uint32)
        self.L.sb_pcg_colouring(self.ptr, out.ctypes.data_as(vp))
        return out

    def apply(self, r):
        """z = M^-1 r with the handle's preconditioner, once; r and z in original row order.  Not between start and finish."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.shape != (self.problem.nr,):
            raise ValueError("r must hold nr = %d doubles, got shape %r" % (self.problem.nr, r.shape))
        return self._vector("apply_precond", r.ctypes.data_as(vp))

    def apply_ms(self, reps=10):
        """GPU milliseconds per apply, the mean of `reps` back-to-back applies on scratch vectors"""
        return self.L.sb_pcg_apply_precond_ms(self.ptr, int(reps))

    def precond_bytes(self):
        """bytes one apply reads and writes (the byte model's input)"""
        return self.L.sb_pcg_precond_bytes(self.ptr)

    def history(self):
        """rr, rz, pAp"""
        cap = self.itermax + 2
        rr, rz, pap = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        npap = C.c_int(0)
        nrr = self.L.sb_pcg_history(self.ptr, rr.ctypes.data_as(vp), cap, rz.ctypes.data_as(vp), cap, pap.ctypes.data_as(vp), cap,
                                    C.byref(npap))
        return rr[:nrr].copy(), rz[:nrr].copy(), pap[:npap.value].copy()

    def dinv(self):
        """the preconditioner in use, original row order"""
        return self._vector("dinv")


class BiCGStab(_PlanBorrower, _BodySolver):
    """Right-preconditioned BiCGStab (sb_bicgstab_*) for matrices that need not be symmetric.  precond "none":
    dinv = 1.0 everywhere; "jacobi": 1 / diag(A); a `dinv` of nr finite non-zero doubles in original row order selects the
    caller's (precond is then "caller").  precond a `PCG` instance: that handle's preconditioner plan makes ph and sh (DESIGN
    4.18) -- the sweeps, the polynomial or a V-cycle of either; the PCG is BORROWED: it must be over the same problem, outlive this
    handle and have no solve open when this one is made or started (a diagonal PCG without a plan: its dinv is copied).  precond
    "sgs", "mg", "mgfw", "poly" or "mgpoly" with PCG's own keyword arguments (levels, coarse, steps, lmax, ratio, coarse_steps,
    galerkin, coarsening, theta, omega_s): the handle builds such a PCG of its own and frees it with itself.  Neither takes a dinv.  Double precision, one
    rank, tree dot order."""

    PREFIX, NAME = "sb_bicgstab", "BiCGStab"
    COUNTERS = ("stop", "iters", "n_rr", "n_rv", "n_ts")
    HISTORIES = ("rr", "rho", "rv", "ts", "tt")

    def __init__(self, problem, precond="none", dinv=None, **plan_args):
        if self._check_precond(problem, precond, dinv, plan_args):
            self._take_pcg(problem, precond, plan_args)
            b, xe = self._open(problem)
            self.ptr = self.L.sb_bicgstab_create_pre(problem.matrix, problem.halo, _ptr(b), _ptr(xe), self.pcg.ptr)
            return
        if dinv is not None:
            precond = "caller"
        kinds = {"none": 0, "jacobi": 1, "caller": 2}
        if precond not in kinds or (precond == "caller" and dinv is None):
            raise ValueError("precond must be 'none' or 'jacobi', or pass dinv; got %r" % (precond,))
        b, xe = self._open(problem)
        self._kind = precond
        self.ptr = self.L.sb_bicgstab_create(problem.matrix, problem.halo, _ptr(b), _ptr(xe), kinds[precond],
                                             _ptr(self._dinv_arg(dinv)))

    def history(self):
        """dict of rr, rho (entry 0: the prologue's, then one per body) and rv, ts, tt (one per body)"""
        cap = max(self.itermax, 0) + 2
        out = {}
        for which, name in enumerate(self.HISTORIES):
            a = np.zeros(cap)
            cnt = self.L.sb_bicgstab_history(self.ptr, which, a.ctypes.data_as(vp), cap)
            out[name] = a[:cnt].copy()
        return out
