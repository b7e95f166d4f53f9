"""Pack the raw MPICH golden dumps (gen_mpich_golden.c) into .npz files.

Each case becomes arrays `<id>.in` (uint8, [n, in_bytes]) and `<id>.out`
(uint8, [n, out_bytes]); the manifest (JSON lines) and the op x type error
matrix are stored as JSON text next to it.  Load with numpy.load (no pickle).

The world sizes in OWN_FILES were recorded after mpich_golden.npz was first
committed; each gets files of its own (mpich_golden_n<k>_a.npz, _b.npz, ... cut
in manifest order so that every part stays under PART_LIMIT, and
mpich_golden_n<k>_manifest.json), so that adding one leaves the earlier files'
bytes alone.  tests/golden_io.py load() returns the union.
"""
import json
import os
import string
import sys

import numpy as np

OWN_FILES = (7,)
PART_LIMIT = 1 << 20  # the repository's limit per committed file


def read_case(raw, c):
    out = {}
    nr = c["n"]  # rows = ranks (reduce_local: in = [in, inout])
    for tag in ("in", "out"):
        b = np.fromfile(os.path.join(raw, f"{c['id']}.{tag}.bin"), dtype=np.uint8)
        per = c[f"{tag}_bytes"]
        rows = b.size // per if per else nr
        out[f"{c['id']}.{tag}"] = b.reshape(rows, per)
    return out


def pack_parts(raw, dest, n, cases):
    """n's cases into the fewest parts, contiguous in manifest order and about
    equal in raw bytes, that each compress to less than PART_LIMIT."""
    per_case = [read_case(raw, c) for c in cases]
    size = np.cumsum([sum(a.nbytes for a in d.values()) for d in per_case])
    for k in range(1, len(string.ascii_lowercase) + 1):
        cuts = [int(np.searchsorted(size, size[-1] * i / k)) for i in range(k + 1)]
        cuts[0], cuts[-1] = 0, len(cases)
        names = [os.path.join(dest, f"mpich_golden_n{n}_{string.ascii_lowercase[i]}.npz") for i in range(k)]
        for i, name in enumerate(names):
            part = {}
            for d in per_case[cuts[i]:cuts[i + 1]]:
                part.update(d)
            np.savez_compressed(name, **part)
        if all(os.path.getsize(name) < PART_LIMIT for name in names):
            break
        for name in names:
            os.remove(name)
    else:
        raise SystemExit(f"n = {n}: no split under {PART_LIMIT} bytes per part")
    with open(os.path.join(dest, f"mpich_golden_n{n}_manifest.json"), "w") as f:
        json.dump(cases, f, indent=0)
    print(f"n = {n}: {len(cases)} cases, {int(size[-1])} raw bytes,",
          ", ".join(f"{os.path.basename(x)} {os.path.getsize(x)}" for x in names))


def main(raw, dest):
    cases = []
    for fn in sorted(os.listdir(raw)):
        if fn.startswith("manifest_") and fn.endswith(".jsonl"):
            with open(os.path.join(raw, fn)) as f:
                cases += [json.loads(l) for l in f if l.strip()]
    for n in OWN_FILES:
        own = [c for c in cases if c["n"] == n]
        if own:
            pack_parts(raw, dest, n, own)
    cases = [c for c in cases if c["n"] not in OWN_FILES]
    arrays = {}
    for c in cases:
        arrays.update(read_case(raw, c))
    np.savez_compressed(os.path.join(dest, "mpich_golden.npz"), **arrays)
    with open(os.path.join(dest, "mpich_golden_manifest.json"), "w") as f:
        json.dump(cases, f, indent=0)
    with open(os.path.join(raw, "op_type_matrix.json")) as f:
        matrix = json.load(f)
    with open(os.path.join(dest, "op_type_matrix.json"), "w") as f:
        json.dump(matrix, f, indent=1, sort_keys=True)
    print(f"packed {len(cases)} cases, {sum(a.nbytes for a in arrays.values())} raw bytes")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
