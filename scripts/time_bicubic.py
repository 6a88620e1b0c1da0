"""Bicubic K1q timed against its two neighbours at config-5 geometry (float32
source, EPSG:4326 -> EPSG:3857, 2048^2 tiles), interleaved in one process:
  (a) bilinear K1b,
  (b) bicubic K1q (the separable rolling-row kernel), optionally at other
      band heights (--bands, through the reproject_band testing knob),
  (c) bicubic through the per-pixel 16-tap gather: the same plan with its
      separable coordinates expanded to 2-D tables on the device.
(b) and (c) are compared bit for bit first.  Every arm replays its launches
from a captured graph; the median over --rounds interleaved rounds is
reported.  Prints one JSON line per output dtype.
    python scripts/time_bicubic.py --size 40960"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=40960)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bands", type=int, nargs="*", default=[])
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="peak HBM rate for the fraction")
    args = ap.parse_args()
    import torch

    import bench_configs as bc
    import configs
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import _native, kernels

    size = args.size
    scale = 40960 / size
    xres, yres = 0.0015 * scale, 0.001 * scale
    sgm = xrs.GridMapping.regular((size, size), (configs.REPROJECT_SRC_X0,
                                                 configs.REPROJECT_SRC_Y0 - size * yres),
                                  (xres, yres), "EPSG:4326")
    tgm = xrs.GridMapping.regular((size, size), configs.REPROJECT_TGT_MIN,
                                  (166 * scale, 190 * scale), "EPSG:3857", tile_size=2048)
    plan = xrs.plan_reproject(sgm, tgm, xrs.Transformer.from_crs(tgm.crs, sgm.crs, always_xy=True))
    assert plan.coord_mode == 0
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cuda")
    g.manual_seed(20250905)
    src = torch.rand((1, size, size), generator=g, device="cuda", dtype=torch.float32)
    # (c): the separable coordinates as 2-D tables, made on the device
    tabs = plan.device_tables(dev)
    plan2d = dataclasses.replace(plan, coord_mode=1, x_gen=None, _device_cache={})
    plan2d._device_cache[str(dev)] = dict(
        src_x=tabs["src_x"][None, :].expand(size, size).contiguous(),
        src_y=tabs["src_y"][:, None].expand(size, size).contiguous(), **plan2d._tile_tables(dev))
    lo, hi = plan.row_source_extent()
    src_rows = int(hi.max() - lo[hi >= lo].min() + 1)
    flags = kernels.ErrorFlags(dev)
    for od in (np.float32, np.float64):
        out = torch.empty((1, size, size), device="cuda",
                          dtype=torch.float32 if od == np.float32 else torch.float64)
        ref = kernels.reproject(src, plan, "bicubic", np.nan, out_dtype=od).clone()
        kernels.reproject(src, plan2d, "bicubic", np.nan, out_dtype=od, out=out)
        bits = torch.int32 if od == np.float32 else torch.int64
        assert torch.equal(out.view(bits), ref.view(bits)), "K1q != per-pixel gather"
        del ref

        def run(p, interp):
            return lambda: kernels.reproject(src, p, interp, np.nan, out_dtype=od, out=out,
                                             flags=flags, check=False)

        arms = {"a_bilinear_k1b": (run(plan, "bilinear"), 0), "b_bicubic_k1q": (run(plan, "bicubic"), 0),
                "c_bicubic_per_pixel": (run(plan2d, "bicubic"), 0)}
        for b in args.bands:
            arms[f"b_bicubic_k1q_band{b}"] = (run(plan, "bicubic"), b)
        ms = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, (fn, band) in arms.items():
                with _native.testing_knob("reproject_band", band):
                    ms[k].append(bc._timed(fn, args.steps, 1, graph=True)[0])
        flags.raise_if_set("time_bicubic")
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        bytes_alg = size * size * np.dtype(od).itemsize + 4 * src_rows * plan.source_cols_read()
        gbs = bytes_alg / (med["b_bicubic_k1q"] / 1e3) / 1e9
        print(json.dumps({"size": size, "out": np.dtype(od).name, "ms_median": med,
                          "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
                          "k1q_algorithmic_GBs": round(gbs, 1),
                          "k1q_hbm_fraction": round(gbs / args.hbm_gbs, 3),
                          "k1q_over_k1b": round(med["b_bicubic_k1q"] / med["a_bilinear_k1b"], 3),
                          "per_pixel_over_k1q": round(med["c_bicubic_per_pixel"] /
                                                      med["b_bicubic_k1q"], 3)}), flush=True)
        del out


if __name__ == "__main__":
    main()
