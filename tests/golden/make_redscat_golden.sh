#!/bin/bash
# Regenerates tests/golden/redscat_golden.npz, redscat_golden_n6_n8.npz,
# redscat_golden_n7.npz and redscat_golden_manifest.json from
# MPICH 3.3.2 (/opt/conda): MPI_Reduce_scatter_block / MPI_Reduce_scatter at
# n = 1..8 (gen_redscat_golden.c).  Run in the build container
# (needs /opt/conda MPICH); the outputs are committed.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
work="$(mktemp -d)"
gcc -O2 -std=c99 -o "$work/gen" "$here/gen_redscat_golden.c" -I/opt/conda/include \
    -L/opt/conda/lib -lmpi -lm -Wl,-rpath,/opt/conda/lib
mkdir -p "$work/raw"
for n in 1 2 3 4 5 6 7 8; do
  /opt/conda/bin/mpiexec -n $n "$work/gen" "$work/raw"
done
PYTHONPATH="$here/../..:$here/.." python3 "$here/pack_redscat_golden.py" "$work/raw" "$here"
rm -rf "$work"
