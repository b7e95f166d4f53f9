"""bench.py as the driver runs it (N = 1, no --full): one JSON line whose
`steps` is the number asked for, and --dump-outputs writing the timed path's
last output — the fold of the seeded inputs, bit-exact against the
MPICH-pinned oracle and the same on a second run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(dump, steps):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--mib", "4", "--dump-outputs", dump],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """Two plain runs of bench.py at 8 x 4 MiB, each a process of its own (~8 s)."""
    import torch
    from oracle import mpich_model as M

    a_dir, b_dir = str(tmp_path / "a"), str(tmp_path / "b")
    line = _run(a_dir, 3)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["higher_is_better"] is True
    assert (line["unit"], line["dtype"]) == ("GB/s", "f32")
    # value is the algorithmic bytes of one step over ms_per_step (printed to 1e-4 ms, value to 0.01)
    tol = line["value"] * 0.5e-4 / (line["ms_per_step"] - 0.5e-4) + 0.01
    assert abs(line["value"] - 9 * (4 << 20) / (line["ms_per_step"] / 1e3) / 1e9) <= tol
    # nothing beside the headline ran
    assert line["cpu_baseline"] is None and line["variants"] is None and line["sweep_local_f32_sum"] is None
    assert os.listdir(a_dir) == ["out.npy"]
    out = np.load(os.path.join(a_dir, "out.npy"))
    count = 4 << 18
    assert out.dtype == np.float32 and out.shape == (count,)
    # bench.py's inputs, regenerated from its seed
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1234)
    ins = [(torch.rand(count, device=dev, generator=g) * 2 - 1).cpu().numpy() for _ in range(8)]
    ref = M.fold_rsag(ins, "FLOAT", "SUM")
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    # the same arguments give the same output, whatever the number of steps
    assert _run(b_dir, 5)["steps"] == 5
    assert np.array_equal(out.view(np.uint32), np.load(os.path.join(b_dir, "out.npy")).view(np.uint32))
