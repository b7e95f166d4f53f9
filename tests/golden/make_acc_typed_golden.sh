#!/bin/bash
# Regenerates tests/golden/acc_typed_golden.json: the MPICH-expressible cases
# of tests/spmd/acc_typed_cases.py (Accumulate / Get_accumulate through
# non-contiguous derived datatypes) run by tests/spmd/acc_typed_worker.py on
# host arrays at n = 3 under MPICH 3.3.2 (/opt/conda), the libmpi MPI.jl
# ccalls (src/onesided.jl).  Run in the build container; the JSON is committed,
# the model (tests/test_acc_typed_cpu.py) and the device run
# (tests/test_acc_typed_gpu.py) must reproduce it exactly.  Whole windows,
# result and origin allocations are stored as hex bytes, or as their SHA-256
# when longer than 256 bytes (acc_typed_cases.enc); inputs come from the
# table's seeds and are not stored.
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
root="$(dirname "$(dirname "$here")")"
work="$(mktemp -d)"
n=3
MPIGX_HOST_ONLY=1 OMP_NUM_THREADS=1 ACC_TYPED_OUT="$work/n$n" /opt/conda/bin/mpiexec -n $n \
  python3 "$root/tests/spmd/acc_typed_worker.py"
python3 - "$work" "$here/acc_typed_golden.json" $n <<'PY'
import json, sys
work, dest, n = sys.argv[1], sys.argv[2], int(sys.argv[3])
recs = []
for r in range(n):
    d = json.load(open(f"{work}/n{n}.{r}"))
    assert d["failed"] is None, d["failed"]
    recs.append(d["records"])
json.dump({"source": "MPICH 3.3.2 (/opt/conda), tests/spmd/acc_typed_worker.py on host arrays", "n": n,
           "records": recs}, open(dest, "w"), indent=None, separators=(",", ":"))
PY
rm -rf "$work"
