"""Bicubic K6q on the rectify route timed against its two neighbours on config
4's swath (scripts/bench_configs.py: 4000 x 4800, float64 lon / lat, one
float32 variable), once onto its own-resolution grid and once onto the 2x finer
grid, interleaved in one process:
  (a) bilinear through K6 (xrs_rectify_var, unfused),
  (b) bicubic K6q with LDS staging,
  (c) bicubic with every tile on the 16-tap global path (rectify_bicubic_direct).
The ij image is computed once per geometry, outside the timed region; (b) and
(c) are compared bit for bit first.  Every arm replays its launches from a
captured graph; the median over --rounds interleaved rounds is reported.
Appends one JSON line per geometry to --out.  --label names a build (a tile
height arm loaded through XRS_LIBRARY).
    python scripts/time_rectify_bicubic.py"""
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
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--height", type=int, default=4800)
    ap.add_argument("--divs", type=float, nargs="*", default=[1.0, 2.0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rectify_bicubic_k6q.jsonl"))
    args = ap.parse_args()
    import torch

    import bench_configs as bc
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import _native, kernels
    from xcube_resampling_amd import rectify as R

    w, h = args.width, args.height
    rng = np.random.default_rng(20250905)
    i = np.arange(w)[None, :].astype(np.float64)
    j = np.arange(h)[:, None].astype(np.float64)
    lat = 60 - 0.0027 * j - 0.0004 * i + 1e-9 * (i - w / 2) ** 2 \
        + rng.normal(0, 0.05 * 0.0027, (h, w))
    lon = 5 + 0.0045 * i + 0.0009 * j + rng.normal(0, 0.05 * 0.0045, (h, w))
    src = torch.from_numpy(rng.random((1, h, w), dtype=np.float32)).cuda()
    sgm = xrs.GridMapping.from_coords(xrs.DataArray(lon, ("y", "x"), name="lon"),
                                      xrs.DataArray(lat, ("y", "x"), name="lat"), "EPSG:4326")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for div in args.divs:
        res = 0.0027 / div
        x0, y0 = float(np.floor(lon.min() / res) * res), float(np.floor(lat.min() / res) * res)
        tw, th = int(np.ceil((lon.max() - x0) / res)), int(np.ceil((lat.max() - y0) / res))
        tgm = xrs.GridMapping.regular((tw, th), (x0, y0), res, "EPSG:4326", tile_size=512)
        ij = R._compute_target_source_ij(sgm, tgm, 1e-3)
        flags = kernels.ErrorFlags(src.device)
        out = torch.empty((1, th, tw), device="cuda", dtype=torch.float32)
        ref = kernels.rectify_var(ij, src, "bicubic", float("nan")).clone()
        with _native.testing_knob("rectify_bicubic_direct", 1):
            kernels.rectify_var(ij, src, "bicubic", float("nan"), out=out, flags=flags)
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "staged != 16-tap path"
        covered = int(torch.sum(~torch.isnan(ij[0])).item())
        del ref

        def run(interp):
            return lambda: kernels.rectify_var(ij, src, interp, float("nan"), out=out,
                                               flags=flags)

        # arm: (call, testing knob held while its graph is captured)
        arms = {"a_bilinear_k6": (run("bilinear"), ("rectify_bicubic_direct", 0)),
                "b_bicubic_k6q_staged": (run("bicubic"), ("rectify_bicubic_direct", 0)),
                "c_bicubic_16tap_global": (run("bicubic"), ("rectify_bicubic_direct", 1))}
        ms = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, (fn, knob) in arms.items():
                with _native.testing_knob(*knob):
                    ms[k].append(bc._timed(fn, args.steps, 1, graph=True)[0])
        flags.raise_if_set("time_rectify_bicubic")
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        line = json.dumps({"label": args.label, "swath": [w, h], "target": [tw, th], "div": div,
                           "dtype": "float32", "covered_px": covered, "ms_median": med,
                           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
                           "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
                           "global_over_staged": round(med["c_bicubic_16tap_global"] /
                                                       med["b_bicubic_k6q_staged"], 3),
                           "staged_over_bilinear": round(med["b_bicubic_k6q_staged"] /
                                                         med["a_bilinear_k6"], 3)})
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del ij, out


if __name__ == "__main__":
    main()
