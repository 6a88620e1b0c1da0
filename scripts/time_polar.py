"""The polar stereographic and rotated-pole pipelines timed against config 2u:
8192^2 bilinear reprojections, float32 in, float64 out, each through the fused
gather (xrs_reproject_proj, K1p) and through tables made per call
(xrs_transform + K1c).  The cases alternate within every round of one run, so
they share whatever else the machine is doing; one JSON line per case (median
of the rounds, their spread, ns per pixel and the ratio to 2u's) goes to --out.
    python scripts/time_polar.py [--rounds N] [--reps K] [--out FILE]"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 8192


def cases():
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd.crs import rotated_pole_crs

    rot = rotated_pole_crs(39.25, -162.0)   # CORDEX EUR-11
    # name: source (xy_min, res, crs), target (xy_min, res, crs); every target pixel
    # lies inside its source
    return {
        "2u_utm_to_laea": (((400000.0, 5400000.0), 30.0, "EPSG:32632"),
                           ((4180000.0, 2870000.0), 30.0, "EPSG:3035")),
        "latlon_to_3413": (((-75.0, 58.0), (60.0 / SIZE, 26.0 / SIZE), "EPSG:4326"),
                           ((-600.0e3, -2700.0e3), 150.0, "EPSG:3413")),
        "rotated_to_3035": (((-14.336, -14.336), 0.0035, rot),
                            ((3.66e6, 1.87e6), 300.0, "EPSG:3035")),
    }, xrs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--size", type=int, default=SIZE, help="rehearsals only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_rotated.jsonl"))
    args = ap.parse_args()
    import torch

    from xcube_resampling_amd import kernels

    assert torch.cuda.is_available(), "time_polar needs a HIP device"
    specs, xrs = cases()
    n = args.size
    src = torch.rand((1, n, n), device="cuda", dtype=torch.float32)
    out = torch.empty((1, n, n), device="cuda", dtype=torch.float64)
    flags = kernels.ErrorFlags(src.device)
    plans = {}
    for name, ((smin, sres, scrs), (tmin, tres, tcrs)) in specs.items():
        sgm = xrs.GridMapping.regular((n, n), smin, sres, scrs, tile_size=2048)
        tgm = xrs.GridMapping.regular((n, n), tmin, tres, tcrs, tile_size=2048)
        plan = xrs.plan_reproject(sgm, tgm, xrs.Transformer.from_crs(tgm.crs, sgm.crs,
                                                                     always_xy=True))
        assert plan.coord_mode == 1
        plans[name, "tables"] = plan
        plans[name, "fused"] = dataclasses.replace(plan, fuse_transform=True, _device_cache={})

    def run(key, k):
        p = plans[key]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(k):
            if key[1] == "tables":
                p._device_cache.clear()   # the tables are made again: xrs_transform + K1c
            kernels.reproject(src, p, "bilinear", float("nan"), out=out, flags=flags, check=False)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k

    times = {key: [] for key in plans}
    finite = {}
    for key in plans:   # warm-up: code objects, allocator
        run(key, 2)
        finite[key] = float(torch.isfinite(out).double().mean())
    for _ in range(args.rounds):
        for key in plans:
            times[key].append(run(key, args.reps))
    flags.raise_if_set("time_polar")
    med = {key: statistics.median(v) for key, v in times.items()}
    lines = []
    for name in specs:
        rec = {"case": name, "size": n, "interp": "bilinear", "dtype": "float32->float64",
               "rounds": args.rounds, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
        for path in ("fused", "tables"):
            key = (name, path)
            rec[f"{path}_ms"] = round(med[key], 4)
            rec[f"{path}_ms_min_max"] = [round(min(times[key]), 4), round(max(times[key]), 4)]
            rec[f"{path}_ns_per_px"] = round(med[key] * 1e6 / (n * n), 4)
            rec[f"{path}_vs_2u"] = round(med[key] / med["2u_utm_to_laea", path], 4)
            rec[f"{path}_finite"] = round(finite[key], 4)
        lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
