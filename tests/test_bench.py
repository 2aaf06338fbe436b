"""bench.py: the plain line, --dump-outputs and --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("kernels", "roofline", "cpu_baseline")


class _FakeProblem:
    """The three members bench.dump_outputs reads, over host arrays."""

    def __init__(self, n):
        self._bs = {"T": 1, "phi": 1, "Tf": 1, "xi": 1, "sigma": 9}
        self._n = n
        self._v = {f: np.arange(n * b, dtype=np.float64) + 1000.0 * i for i, (f, b) in enumerate(self._bs.items())}

    def num_dofs(self, space=0):
        return self._n, 0

    def get_field(self, f):
        return self._v[f].copy()


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    import bench
    n = 1000
    p = _FakeProblem(n)
    bench.dump_outputs(p, str(tmp_path / "whole"), 0, 1)
    for f, b in p._bs.items():
        v = np.load(tmp_path / "whole" / f"{f}.npy")
        assert v.dtype == np.float64 and v.shape == (n, b)
        assert np.array_equal(v.reshape(-1), p._v[f])
    # cap below the whole: the same sorted sample of the dofs in every field and every call
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 13 * 100)
    bench.dump_outputs(p, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(p, str(tmp_path / "b"), 0, 1)
    T = np.load(tmp_path / "a" / "T.npy")
    assert T.shape == (100, 1)
    idx = T[:, 0].astype(np.int64)  # T holds its own dof index
    assert np.all(np.diff(idx) > 0) and idx[-1] < n
    total = 0
    for f, b in p._bs.items():
        va, vb = np.load(tmp_path / "a" / f"{f}.npy"), np.load(tmp_path / "b" / f"{f}.npy")
        assert np.array_equal(va, vb)
        assert np.array_equal(va, p._v[f].reshape(n, b)[idx])
        total += va.nbytes
    assert total <= 8 * 13 * 100
    # partitioned runs name the rank
    bench.dump_outputs(p, str(tmp_path / "p"), 1, 2)
    assert sorted(os.listdir(tmp_path / "p")) == sorted(f"{f}_part1.npy" for f in p._bs)


def _bench(*args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cells", "12,10,6",
                          "--lengths", "2,2,1", *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_line_and_dump(tmp_path):
    """A plain run prints the headline line without the --full records, and
    --dump-outputs holds the fields of the last timed step.  With --restart-steps 3
    and one warm-up step the five timed steps run as segments of 2, 2 and 1 on
    fresh problems, so the last one is step 2 of the transient: two steps taken
    through ThermoViscoProblem give the dumped fields back."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rec = _bench("--steps", "5", "--warmup", "1", "--restart-steps", "3", "--dump-outputs", str(tmp_path))
    assert all(k in rec for k in HEADLINE) and not any(k in rec for k in FULL_ONLY)
    assert rec["steps"] == 5 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["dtype"] == "f64"
    assert rec["value"] == pytest.approx(13 * 11 * 7 * 5 / (rec["ms_per_step"] * 5e-3), rel=1e-9)

    import bench
    from tvfem import box_mesh
    from tvfem.problem import ThermoViscoProblem
    mp = {"f": 0.0, "epsilon": 0.93, "sigma": 5.670e-8, "T_ambient": 600.0, "T_0": 800.0, "alpha": 1.0,
          "htc": 280.1, "rho": 2500.0, "cp": 1433.0, "k": 1.0, "H": 627.8e3, "Tb": 869.0e0, "Rg": 8.314,
          "alpha_solid": 9.10e-6, "alpha_liquid": 25.10e-6, "Tf_init": 873.0}
    cfg = {"T": {"element": "CG", "degree": 1}, "sigma": {"element": "CG", "degree": 1}}
    prob = ThermoViscoProblem(box_mesh([2.0, 2.0, 1.0], [12, 10, 6]), (0.0, 50.0), 0.1, cfg, mp, device=0,
                              materialize=False, verbose=False, write_output=False, n_parts=1, part=0, part_axis=1)
    prob.setup()
    for _ in range(2):  # timed: steps 2, 3 | 2, 3 | 2 of the transient
        prob.solve_timestep()
    n = 13 * 11 * 7
    for f in bench.DUMP_FIELDS:
        v = np.load(tmp_path / f"{f}.npy")
        ref = prob.get_field(f).reshape(n, -1)
        assert v.dtype == np.float64 and v.shape == ref.shape and np.all(np.isfinite(v))
        # the same kernels on the same inputs (steps repeat bitwise in tests/test_loopback.py);
        # 1e-12 is the f64 rounding of a differently ordered reduction through the Newton solve
        assert np.linalg.norm(v - ref) <= 1e-12 * np.linalg.norm(ref) + 1e-300, f
    assert float(np.ptp(np.load(tmp_path / "T.npy"))) > 0.0  # the plate has started to cool from its faces
    prob.close()


@pytest.mark.gpu
def test_bench_full_adds_the_measured_records():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    rec = _bench("--steps", "1", "--warmup", "1", "--full", "--kernel-reps", "2", "--cpu-seconds", "0.2")
    assert all(k in rec for k in HEADLINE + FULL_ONLY)
    assert rec["roofline"]["frac"] > 0 and rec["kernels"]["visco_update"]["ms"] > 0
    assert rec["cpu_baseline"]["value"] is None or rec["cpu_baseline"]["value"] > 0
