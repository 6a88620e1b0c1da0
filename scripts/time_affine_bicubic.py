"""Bicubic K2q on the same-CRS affine path timed against its two neighbours at
the x2 upsample (float32 source size^2 -> (2 size)^2, 2048^2 tiles), one plan
geometry, interleaved in one process:
  (a) order 1 through K2 (xrs_affine),
  (b) bicubic K2q (the LDS-tiled separable kernel), optionally at other tile
      heights (--tile-h, through the affine_bicubic_tile_h testing knob),
  (c) bicubic through the per-pixel 16-tap kernel (affine_bicubic_direct knob).
(b) and (c) are compared bit for bit first.  Every arm replays its launches
from a captured graph; the median over --rounds interleaved rounds is
reported.  Appends one JSON line to --out.
    python scripts/time_affine_bicubic.py --size 10240"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=10240, help="source edge; the target is twice it")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tile-h", type=int, nargs="*", default=[])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM rate for the fraction")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_bicubic_k2q.jsonl"))
    args = ap.parse_args()
    import torch

    import bench_configs as bc
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import _native, kernels
    from xcube_resampling_amd.affine import plan_affine

    n, m = args.size, 2 * args.size
    sgm = xrs.GridMapping.regular((n, n), (600000.0, 5000000.0), 20.0, "EPSG:32632")
    tgm = xrs.GridMapping.regular((m, m), (600000.0, 5000000.0), 10.0, "EPSG:32632",
                                  tile_size=2048)
    matrix = tgm.ij_transform_to(sgm)
    plans = {k: plan_affine((1, n, n), np.float32, matrix, (m, m), (2048, 2048), k, "mean", False,
                            np.nan) for k in (1, "bicubic")}
    assert plans["bicubic"].method == "bicubic" and plans[1].t_next is None
    g = torch.Generator(device="cuda")
    g.manual_seed(20250905)
    src = torch.rand((1, n, n), generator=g, device="cuda", dtype=torch.float32)
    out = torch.empty((1, m, m), device="cuda", dtype=torch.float32)
    ref = kernels.affine(src, plans["bicubic"]).clone()
    with _native.testing_knob("affine_bicubic_direct", 1):
        kernels.affine(src, plans["bicubic"], out=out)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "K2q != per-pixel kernel"
    del ref

    def run(key):
        return lambda: kernels.affine(src, plans[key], out=out)

    # arm: (call, testing knob held while its graph is captured)
    arms = {"a_order1_k2": (run(1), ("affine_bicubic_direct", 0)),
            "b_bicubic_k2q": (run("bicubic"), ("affine_bicubic_direct", 0)),
            "c_bicubic_per_pixel": (run("bicubic"), ("affine_bicubic_direct", 1))}
    for th in args.tile_h:
        arms[f"b_bicubic_k2q_tile_h{th}"] = (run("bicubic"), ("affine_bicubic_tile_h", th))
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, (fn, knob) in arms.items():
            with _native.testing_knob(*knob):
                ms[k].append(bc._timed(fn, args.steps, 1, graph=True)[0])
    med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    bytes_alg = 4 * (m * m + n * n)   # the output once plus the source once
    gbs = bytes_alg / (med["b_bicubic_k2q"] / 1e3) / 1e9
    line = json.dumps({"size": n, "target": m, "dtype": "float32", "ms_median": med,
                       "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
                       "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
                       "k2q_algorithmic_GBs": round(gbs, 1),
                       "k2q_hbm_fraction": round(gbs / args.hbm_gbs, 3),
                       "k2q_over_order1": round(med["b_bicubic_k2q"] / med["a_order1_k2"], 3),
                       "per_pixel_over_k2q": round(med["c_bicubic_per_pixel"] /
                                                   med["b_bicubic_k2q"], 3)})
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
