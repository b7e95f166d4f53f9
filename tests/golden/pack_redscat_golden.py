"""Pack gen_redscat_golden.c's dumps into tests/golden/redscat_golden.npz (n <= 5),
redscat_golden_n6_n8.npz and redscat_golden_n7.npz (one uint8 array per case, `<id>`: every rank's
output bytes in rank order, each in full or at the case's spans; tests/redscat_model.py split_outputs cuts it) +
redscat_golden_manifest.json.  Load with numpy.load (no pickle).

Refuses to pack fixtures that would not discriminate (tests/redscat_model.py
regenerates the inputs): for every FLOAT SUM case at n >= 4 the rank-ordered
left fold of the same inputs must differ from what MPICH returned, and for the
MIN / MAX cases on NaN / signed-zero inputs the model with swapped operand
roles must."""
import json
import os
import sys

import numpy as np

import redscat_model as R


def discriminates(case, arrays):
    """None when the case carries no such duty, else whether it meets it."""
    n = case["n"]
    fsum = case["dtype"] == "FLOAT" and case["op"] == "SUM" and n >= 4
    roles = case["op"] in ("MIN", "MAX") and case["mode"] in (R.G_NAN, R.G_SZERO) and n >= 2
    if not (fsum or roles):
        return None
    counts = R.counts_of(case, n)
    ins = R.case_inputs(case)
    if fsum:
        other = R.reduce_scatter(ins, counts, case["dtype"], case["op"], order="linear")
    else:
        other = R.reduce_scatter(ins, counts, case["dtype"], case["op"], swap=True)
    return any(R.sample(other[r], case).tobytes() != arrays[case["id"]][r].tobytes()
               for r in range(n))


def main(raw, dest):
    cases = []
    for fn in sorted(os.listdir(raw)):
        if fn.startswith("manifest_redscat_") and fn.endswith(".jsonl"):
            with open(os.path.join(raw, fn)) as f:
                cases += [json.loads(l) for l in f if l.strip()]
    # the manifest follows the files (tests/redscat_model.py GOLDEN_FILES): a world size recorded
    # later gets a file of its own and its cases go to the end, behind the ones already there
    cases.sort(key=lambda c: next(i for i, (_, keep) in enumerate(R.GOLDEN_FILES) if c["n"] in keep))
    arrays = {}
    for c in cases:
        arrays[c["id"]] = [np.fromfile(os.path.join(raw, f"{c['id']}.r{r}.bin"), dtype=np.uint8)
                           for r in range(c["n"])]
    weak = [c["id"] for c in cases if discriminates(c, arrays) is False]
    if weak:
        raise SystemExit(f"fixtures that do not discriminate: {weak}")
    arrays = {k: np.concatenate(v) for k, v in arrays.items()}
    # one file per group of world sizes, each under the repository's 1 MiB per file
    for name, keep in R.GOLDEN_FILES:
        part = {c["id"]: arrays[c["id"]] for c in cases if c["n"] in keep}
        np.savez_compressed(os.path.join(dest, name), **part)
        print(name, os.path.getsize(os.path.join(dest, name)), "bytes")
    with open(os.path.join(dest, "redscat_golden_manifest.json"), "w") as f:
        json.dump(cases, f, indent=0)
    print(f"{len(cases)} cases, {len(arrays)} arrays, {sum(a.size for a in arrays.values())} bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
