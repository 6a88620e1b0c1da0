"""The Albers and sinusoidal pipelines timed against config 2u, with time_polar.py's
harness: 8192^2 bilinear reprojections, float32 in, float64 out, each through the
fused gather (K1p) and through tables made per call (xrs_transform + K1c), the cases
alternating within every round of one run.
    python scripts/time_aea_sinu.py [--rounds N] [--reps K] [--out FILE]"""
from __future__ import annotations

import os
import sys

import time_polar

SIZE = time_polar.SIZE


def cases():
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd.crs import sinusoidal_crs

    modis = sinusoidal_crs()   # the MODIS / VIIRS land grid's sphere
    # name: source (xy_min, res, crs), target (xy_min, res, crs); every target pixel
    # lies inside its source (and inside the lobes / the cone's domain)
    return {
        "2u_utm_to_laea": (((400000.0, 5400000.0), 30.0, "EPSG:32632"),
                           ((4180000.0, 2870000.0), 30.0, "EPSG:3035")),
        "modis_sinu_to_latlon": (((-1.0e5, 3.3e6), 500.0, modis),
                                 ((0.0, 30.0), (40.0 / SIZE, 30.0 / SIZE), "EPSG:4326")),   # [sinu_fwd]
        "latlon_to_5070": (((-120.0, 27.0), (48.0 / SIZE, 29.0 / SIZE), "EPSG:4326"),
                           ((-1.2e6, 0.8e6), 300.0, "EPSG:5070")),                        # [aea_inv]
    }, xrs


if __name__ == "__main__":
    time_polar.cases = cases
    if "--out" not in sys.argv:
        sys.argv += ["--out", os.path.join(time_polar.ROOT, "profiles", "aea_sinu.jsonl")]
    time_polar.main()
