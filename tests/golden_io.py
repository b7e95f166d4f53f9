"""Loader for the MPICH golden fixtures (tests/golden/, made by make_golden.sh)."""
import glob
import json
import os

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# world sizes recorded later, in files of their own (tests/golden/pack_golden.py OWN_FILES)
OWN_FILES = (7,)


def golden_files():
    """The .npz files load() reads, the first fixture first."""
    files = [os.path.join(HERE, "mpich_golden.npz")]
    for n in OWN_FILES:
        parts = sorted(glob.glob(os.path.join(HERE, f"mpich_golden_n{n}_[a-z].npz")))
        assert parts, f"no mpich_golden_n{n}_*.npz"
        files += parts
    return files


class Arrays:
    """Read-only union of .npz files: arrays[key], loaded on first use."""

    def __init__(self, paths):
        self._of = {}
        for z in (np.load(p, allow_pickle=False) for p in paths):
            for k in z.files:
                assert k not in self._of, k
                self._of[k] = z
        self.files = list(self._of)

    def __getitem__(self, key):
        return self._of[key][key]

    def __contains__(self, key):
        return key in self._of


def load():
    """(cases, arrays): every manifest in turn, and the arrays of every file."""
    cases = []
    for name in ["mpich_golden_manifest.json"] + [f"mpich_golden_n{n}_manifest.json" for n in OWN_FILES]:
        with open(os.path.join(HERE, name)) as f:
            cases += json.load(f)
    return cases, Arrays(golden_files())


def op_type_matrix():
    with open(os.path.join(HERE, "op_type_matrix.json")) as f:
        return json.load(f)


def typed(raw_rows, npdtype):
    """[n, bytes] uint8 -> list of per-rank typed arrays."""
    return [np.ascontiguousarray(r).view(npdtype) for r in raw_rows]


def same_bits(a, b, bf16=False):
    """Bitwise equality, except any NaN matches any NaN (payloads and the sign
    of a generated NaN differ by ISA: x86 default NaN is 0xFFC00000, AMDGPU
    0x7FC00000).  bf16=True compares uint16 bf16 patterns that way too."""
    a = np.asarray(a)
    b = np.asarray(b)
    if bf16:
        a = (a.astype(np.uint32) << 16).view(np.float32)
        b = (b.astype(np.uint32) << 16).view(np.float32)
    if a.shape != b.shape:
        return False
    if a.dtype.kind in "fc":
        fa = a.view(a.real.dtype) if a.dtype.kind == "c" else a
        fb = b.view(b.real.dtype) if b.dtype.kind == "c" else b
        na, nb = np.isnan(fa), np.isnan(fb)
        if not np.array_equal(na, nb):
            return False
        return np.array_equal(fa[~na].view(np.uint8 if False else fa.dtype).tobytes(), fb[~nb].tobytes()) and \
            np.array_equal(np.signbit(fa[~na]), np.signbit(fb[~nb]))
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))
