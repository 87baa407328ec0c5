#!/usr/bin/env bash
# build_ref_sp.sh -- the reference's own sources as its SINGLE-PRECISION build (FLOAT_TYPE=SP: -DPRECISION=1), CRS, into
# oracle/_ref/libsbref_crs_sp.so (git-ignored).  The recipe of DESIGN 5 "Single precision" for tests/golden/cg_hist_sp_ref*.json.
#
# TEST INFRASTRUCTURE ONLY.  As in build_ref.sh nothing from the reference is copied into the repository: the compiler reads
# the sources where they lie and writes one shared object.  Same compiler, the same strict flags and the same --wrap=ddot as
# build_ref.sh's libsbref_crs.so; oracle/ref_shim.c unchanged.  Of the shim only sbref_setup, sbref_solve_cg and sbref_hist_*
# are meaningful here (its other helpers are double-typed, hence -Wno-error=incompatible-pointer-types); the logged dots are
# the reference's floats widened to double.
#
# Then: python tests/golden/make_golden_sp_odd.py
set -euo pipefail
REF=${SB_REFERENCE:-/root/reference}
HERE=$(cd "$(dirname "$0")" && pwd)
OUT=$HERE/_ref
S=$REF/src
if [ ! -d "$S" ]; then
  echo "build_ref_sp: $S not present" >&2
  exit 1
fi
CLANG=${CLANG:-/opt/rocm/lib/llvm/bin/clang}
mkdir -p "$OUT"
DEFS="-DPRECISION=1 -DUINT_TYPE=1 -D_GNU_SOURCE -DARRAY_ALIGNMENT=64 -DOMP_SCHEDULE=static"
STRICT="-O2 -fno-fast-math -ffp-contract=off -std=c23 -w -Wno-error=incompatible-pointer-types -fPIC"
COMMON="$S/CGSolver.c $S/solver.c $S/matrix.c $S/mmio.c $S/allocate.c $S/comm.c $S/bstree.c $S/timing.c $S/profiler.c $S/util.c"

$CLANG -DCRS $DEFS $STRICT -I"$S" -shared -o "$OUT/libsbref_crs_sp.so" \
  "$HERE/ref_shim.c" $COMMON "$S/matrix-CRS.c" -Wl,--wrap=ddot -Wl,-Bsymbolic -lm
ls -la "$OUT/libsbref_crs_sp.so"
