"""bench.py's plain run and --dump-outputs: the headline line alone, --steps timed steps, and the last timed step's results as
.npy files that repeat bit for bit from run to run (seeded inputs), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fake_window():
    """CPU stand-ins of the S-B window's state at its real shapes (8 keyframes in a 16-frame buffer, 36 edges, 48 x 64 maps)"""
    import bench
    g = torch.Generator().manual_seed(0)
    E, H, W, n = 36, bench.H8, bench.W8, bench.NKF
    video = SimpleNamespace(poses=torch.randn(16, 7, generator=g), disps=torch.rand(16, H, W, generator=g))
    # (the hidden state is a permuted view, as the graph keeps it: the sample is taken in logical order)
    net = torch.randn(1, E, H, W, 128, generator=g).half().permute(0, 1, 4, 2, 3)
    graph = SimpleNamespace(nkf=n, net=net, damping=torch.rand(16, H, W, generator=g),
                            ii=torch.randint(n, (E,), generator=g), jj=torch.randint(n, (E,), generator=g),
                            **{k: torch.randn(1, E, H, W, 2, generator=g) for k in ("target_cam", "weight", "raw_mask", "delta_dy")})
    last = (torch.rand(n, n, generator=g), torch.rand(1, generator=g))
    return video, graph, last


def test_step_outputs_fit_the_dump_limit_and_sample_the_hidden_state_in_a_fixed_order(tmp_path):
    import bench
    video, graph, last = _fake_window()
    a = bench.step_outputs(video, graph, last)
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_LIMIT_BYTES
    assert a["net_sample"].size == bench.NET_SAMPLE and a["poses"].shape == (bench.NKF, 7)
    b = bench.step_outputs(video, graph, last)
    assert np.array_equal(a["net_sample"], b["net_sample"])
    contiguous = SimpleNamespace(**dict(vars(graph), net=graph.net.contiguous()))
    assert np.array_equal(bench.step_outputs(video, contiguous, last)["net_sample"], a["net_sample"])
    bench.write_outputs(str(tmp_path), a)
    assert sorted(p.stem for p in tmp_path.glob("*.npy")) == sorted(a)
    assert np.array_equal(np.load(tmp_path / "target.npy"), a["target"])
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, np.float32)})
    with pytest.raises(ValueError):
        bench.write_outputs(str(tmp_path / "int"), {"x": np.zeros(4, np.int64)})


def _plain_run(out_dir, steps, warmup):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out_dir)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), {p.stem: np.load(p) for p in out_dir.glob("*.npy")}


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step_reproducibly(cuda, tmp_path):
    line, a = _plain_run(tmp_path / "a", 3, 1)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6
    assert not {"roofline", "step_ms_blocks", "cpu_baseline", "sequence", "edge_sharded"} & set(line)
    assert {"poses", "disps", "target", "weight", "net_sample", "distance_matrix"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    # another number of timed and warm-up steps: every step starts from the restored state, so the last one is the same
    _, b = _plain_run(tmp_path / "b", 5, 2)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
