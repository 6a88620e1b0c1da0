"""bench.py on the device: the plain run's line and what --dump-outputs
writes, against the same launch made in this process."""

from __future__ import annotations

import numpy as np
import pytest

from helpers import assert_bitwise_equal
from test_bench_cpu import _run_bench

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_timed_path_output(tmp_path):
    """`bench.py --steps K --warmup W --dump-outputs DIR` at a size whose
    float32 output exceeds 64 MB (4500^2: partial edge tiles): K sets the
    timed steps, the line carries none of the --full measurements, and the
    file holds the seeded sample of the raster the bench's launch computes
    from the seeded source, bit for bit."""
    import torch

    import bench
    from xcube_resampling_amd import kernels

    size, tile = 4500, 512
    d = tmp_path / "dump"
    r, line = _run_bench(["--gpus", "1", "--size", str(size), "--tile", str(tile), "--steps", "3",
                          "--warmup", "2", "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stderr[-3000:]
    assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0
    assert line["unit"] == "Mpixels/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(size * size / (line["ms_per_step"] / 1e3) / 1e6, rel=1e-3)
    assert not {"cpu_baseline", "f64_out"} & set(line) and line["roofline"]["traffic"] is None
    assert [f.name for f in d.iterdir()] == ["reproject_bilinear.npy"]
    got = np.load(d / "reproject_bilinear.npy")

    _, _, plan, _, _ = bench.workload(size, tile)
    src = bench.synthetic_rows(0, size, size, torch.device("cuda", 0))
    out = kernels.reproject(src, plan, "bilinear", float("nan"), out_dtype=np.float32)
    idx = bench.dump_sample_index(out.numel(), 4)
    assert idx is not None and got.dtype == np.float32 and got.shape == idx.shape
    assert got.nbytes <= bench.DUMP_MAX_BYTES
    assert_bitwise_equal(got, out.cpu().numpy().reshape(-1)[idx], "dumped sample")
    assert np.isfinite(got).any()
