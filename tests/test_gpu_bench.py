"""bench.py as the driver runs it: a plain `--gpus 1 --steps K --warmup W` run prints the headline line, and
`--dump-outputs DIR` holds the solutions of its last timed step -- checked against the fp64 Woodbury closed form of the
same seeded systems."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dumped_solutions(tmp_path):
    out_dir = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["metric"] == "cg_member_matvecs_per_sec" and line["unit"] == "member-matvecs/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 5 and line["warmup"] == 2 and line["step_ms"]["steps"] == 5
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["engine"].startswith("resident R-space, diagonal form")  # the engine the ramp leaves the cache on
    x = np.load(out_dir / "x.npy")
    assert x.dtype == np.float32 and x.shape == (512, 8192, 1)

    import bench

    Cm, d, rhs = bench.make_problem(torch.device("cuda"), 1234)
    assert bench.woodbury_fp64_rel_err(Cm, d, rhs, torch.from_numpy(x).cuda()) < 1e-4  # north_star's bar
