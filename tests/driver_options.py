"""The benchmark driver's option parser (host/sbh_options.c) called from Python: the argv a test would give the driver goes
through sbh_parse_options of libsparsebench_host.so (or of the single-precision library) and comes back as the parsed options or
as the refusal's message and stream.  No driver is started and no device is touched: capi's sb_is_initialized() stays 0.
Below it, for the GPU tests: the caller that executes a drop-in solve* symbol, which the driver itself no longer calls."""
import ctypes as C
import os
import re
import subprocess

# the numbers of include/sparsebench/sparsebench.h
KIND = {None: -1, "jacobi": 0, "sgs": 1, "mg": 2, "mgfw": 3, "poly": 4, "mgpoly": 5}
COARSE = {"regenerated": 0, "galerkin": 1, "aggregation": 2}
TYPE = {"cg": 0, "spmv": 1, "gmres": 2, "pcg": 3, "bicgstab": 4}
RUN, HELP, CONVERT = 0, 1, 2
SIZE = ["-x", "16", "-y", "16", "-z", "16"]


class Parameter(C.Structure):
    _fields_ = [("filename", C.c_char_p), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int), ("itermax", C.c_int), ("eps", C.c_double)]


class Spec(C.Structure):
    _fields_ = [("kind", C.c_int), ("levels", C.c_int), ("steps", C.c_int), ("coarse", C.c_int)]


class Options(C.Structure):
    _fields_ = [("type", C.c_int), ("restart", C.c_int), ("nrhs", C.c_int), ("scsC", C.c_uint), ("scsSigma", C.c_uint), ("byP", C.c_int),
                ("precond", Spec), ("optind", C.c_int), ("action", C.c_int), ("convert", C.c_char_p), ("toStdout", C.c_int)]


class Parsed:
    """what one call gave: status 0 or 1; for a refusal message and stream ("stdout" or "stderr"); the options and the Parameter"""

    def __init__(self, status, message, o, param):
        self.status, self.message, self.stream = status, message, "stdout" if o.toStdout else "stderr"
        self.type, self.restart, self.nrhs, self.scsC, self.scsSigma, self.byP = o.type, o.restart, o.nrhs, o.scsC, o.scsSigma, o.byP
        self.spec = (o.precond.kind, o.precond.levels, o.precond.steps, o.precond.coarse)
        self.optind, self.action, self.convert = o.optind, o.action, o.convert.decode() if o.convert else None
        self.filename, self.dims, self.itermax, self.eps = param.filename.decode(), (param.nx, param.ny, param.nz), param.itermax, param.eps


def _lib(precision):
    from sparsebench_amd import hostapi
    H = hostapi.host(precision)
    H.sbh_parse_options.restype = C.c_int
    H.sbh_parse_options.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(Parameter), C.POINTER(Options), C.c_char_p, C.c_size_t]
    H.sbh_help_text.restype = C.c_char_p
    H.sbh_help_text.argtypes = []
    H.initParameter.restype = None
    H.initParameter.argtypes = [C.POINTER(Parameter)]
    return H


def parse(args, precision="double"):
    """the driver's command line `sparseBench <args>` through the parser of that precision's library"""
    H = _lib(precision)
    words = [b"sparseBench"] + [str(a).encode() for a in args]
    argv = (C.c_char_p * (len(words) + 1))(*words, None)
    param, o, msg = Parameter(), Options(), C.create_string_buffer(4096)
    H.initParameter(C.byref(param))
    status = H.sbh_parse_options(len(words), argv, C.byref(param), C.byref(o), msg, len(msg))
    return Parsed(status, msg.value.decode(), o, param)  # (param.filename may point into argv: read before argv goes)


def accepted(args, precision="double"):
    """the options of a command line the driver runs"""
    p = parse(args, precision)
    assert p.status == 0 and p.action == RUN and p.message == "", (args, p.message)
    return p


def refused(args, message, precision="double", stream="stderr"):
    """the command line is refused with a message that holds `message`, one line on that stream"""
    p = parse(args, precision)
    assert p.status == 1 and message in p.message and p.stream == stream, (args, p.status, p.message, p.stream)
    assert p.message.endswith("\n") and p.message.count("\n") == 1, p.message
    return p


def help_text():
    return _lib("double").sbh_help_text().decode()


def no_device_was_touched():
    from sparsebench_amd import capi
    return capi.load().sb_is_initialized() == 0


def run_dropin_symbol(tmp_path, fmt, define, args, env=None):
    """The driver calls sbh_solve_precond itself, so a drop-in solve* symbol is executed by its own caller: tests/c/solver_driver.c,
    written against the public header alone, built with -D<define> for fmt ("CRS" or "SCS") against that format's drop-in library
    and run with args (<n | file.mtx> <itermax> <eps>).  Returns its standard output and the k that the symbol returned"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "sparsebench_amd", "lib")
    exe = os.path.join(str(tmp_path), "%s_%s" % (define.lower(), fmt))
    subprocess.check_call(["gcc", "-std=gnu11", "-O1", "-Wall", "-D" + fmt, "-I" + os.path.join(root, "include"), "-D" + define,
                           os.path.join(root, "tests", "c", "solver_driver.c"), "-o", exe, "-L" + lib, "-lsparsebench_%s" % fmt.lower(),
                           "-lsparsebench_host", "-lsbhip", "-Wl,-rpath," + lib, "-lm"])
    out = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                         env=dict(os.environ, **(env or {})))
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    txt = out.stdout.decode()
    return txt, int(re.search(r"^k (\d+)$", txt, re.M).group(1))
