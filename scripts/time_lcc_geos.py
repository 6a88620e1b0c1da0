"""The Lambert conformal conic and geostationary pipelines timed against config
2u, with time_polar.py's harness: 8192^2 bilinear reprojections, float32 in,
float64 out, each through the fused gather (K1p) and through tables made per
call (xrs_transform + K1c), the cases alternating within every round of one run.
    python scripts/time_lcc_geos.py [--rounds N] [--reps K] [--out FILE]"""
from __future__ import annotations

import os
import sys

import time_polar

SIZE = time_polar.SIZE


def cases():
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd.crs import geostationary_crs

    goes = geostationary_crs(-75.0, 35786023.0, "x", 6378137.0, 298.257222101)   # GOES-East
    # name: source (xy_min, res, crs), target (xy_min, res, crs); every target pixel
    # lies inside its source (for geos: inside the disc, 75.5 deg from its centre at most)
    return {
        "2u_utm_to_laea": (((400000.0, 5400000.0), 30.0, "EPSG:32632"),
                           ((4180000.0, 2870000.0), 30.0, "EPSG:3035")),
        "latlon_to_3034": (((-25.0, 35.0), (70.0 / SIZE, 35.0 / SIZE), "EPSG:4326"),
                           ((2.8e6, 1.6e6), 300.0, "EPSG:3034")),            # [lcc_inv]
        "geos_disc_to_latlon": (((-5.5e6, -5.5e6), 11.0e6 / SIZE, goes),
                                ((-135.0, -60.0), 120.0 / SIZE, "EPSG:4326")),   # [geos_fwd]
    }, xrs


if __name__ == "__main__":
    time_polar.cases = cases
    if "--out" not in sys.argv:
        sys.argv += ["--out", os.path.join(time_polar.ROOT, "profiles", "lcc_geos.jsonl")]
    time_polar.main()
