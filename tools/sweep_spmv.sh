#!/usr/bin/env bash
# Sweep the SCS C=64 SpMV block mapping through the C driver's -t spmv mode (the resident share is the upload's rule:
# tools/resident_share_ab.py sweeps it inside a CG loop, where it matters).
# Prints the reference-convention MB/s line (12*27*nr bytes per SpMV) per variant.
set -u
cd "$(dirname "$0")/../sparsebench_amd/bin"
N=${1:-128}
for xcd in 1 0; do
  r=$(SB_SCS_XCD=$xcd ./sparseBench-SCS-HIP -x $N -y $N -z $N -i 300 -t spmv -C 64 -s ${2:-1} | grep "spMVM:")
  echo "n=$N sigma=${2:-1} xcd=$xcd $r"
done
