"""Bicubic K1pq (projection fused, taps staged in LDS) timed against its
neighbours on config 2u's geometry (scripts/bench_configs.py: 8192^2 float32,
UTM 32N -> LAEA Europe, 2048^2 tiles, float64 out), once onto the 30 m target
and once onto a finer one, interleaved in one process:
  (a) bicubic K1pq (xrs_reproject_proj) with a 32 KiB staging budget
      (reproject_proj_bicubic_lds: every rectangle of these targets is staged),
  (b) K1pq with every patch on the 16-tap global path (the product's launch),
  (c) xrs_transform + the 2-D-table bicubic kernel (tables rebuilt every step:
      what one variable pays), and (c_k) that kernel alone on resident tables,
  (d) bilinear with the projection fused (K1p), for scale.
(a), (b) and (c) are compared bit for bit first.  (a), (b), (d) and (c_k) replay
their launches from a captured graph; (c) allocates its tables and runs eagerly.
The median over --rounds interleaved rounds is reported.  Appends one JSON line
per geometry to --out.
    python scripts/time_proj_bicubic.py"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--divs", type=float, nargs="*", default=[1.0, 1.5])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--label", default="product")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proj_bicubic_k1pq.jsonl"))
    args = ap.parse_args()
    import torch

    import bench_configs as bc
    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import _native, kernels

    size, res = args.size, 30.0
    sgm = xrs.GridMapping.regular((size, size), (400000.0, 5400000.0), res, "EPSG:32632",
                                  tile_size=2048)
    g = torch.Generator(device="cuda")
    g.manual_seed(20250905)
    src = torch.rand((1, size, size), generator=g, device="cuda", dtype=torch.float32)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    nan = float("nan")
    for div in args.divs:
        tsize = int(size * div)   # the same extent at res / div
        tgm = xrs.GridMapping.regular((tsize, tsize), (4180000.0, 2870000.0), res / div,
                                      "EPSG:3035", tile_size=2048)
        tr = xrs.Transformer.from_crs(tgm.crs, sgm.crs, always_xy=True)
        plan = xrs.plan_reproject(sgm, tgm, tr)
        assert plan.coord_mode == 1
        fplan = dataclasses.replace(plan, fuse_transform=True, _device_cache={})
        out = torch.empty((1, tsize, tsize), device="cuda", dtype=torch.float64)
        flags = kernels.ErrorFlags(src.device)

        def run(p, interp):
            return lambda: kernels.reproject(src, p, interp, nan, out=out, flags=flags,
                                             check=False)

        def tables_end_to_end():
            plan._device_cache.clear()
            kernels.reproject(src, plan, "bicubic", nan, out=out, flags=flags, check=False)

        ref = kernels.reproject(src, plan, "bicubic", nan).view(torch.int64)
        staged, direct = ("reproject_proj_bicubic_lds", 32768), ("reproject_proj_bicubic_direct", 1)
        for knob in (staged, direct):
            with _native.testing_knob(*knob):
                run(fplan, "bicubic")()
            assert torch.equal(out.view(torch.int64), ref), f"K1pq {knob} != tables path"
        assert str(src.device) not in fplan._device_cache
        covered = int(torch.isfinite(out).sum().item())
        del ref

        # arm: (call, testing knob held while it is captured / runs, graph replay)
        arms = {"a_k1pq_staged": (run(fplan, "bicubic"), staged, True),
                "b_k1pq_16tap_global": (run(fplan, "bicubic"), direct, True),
                "c_transform_plus_tables_kernel": (tables_end_to_end, direct, False),
                "ck_tables_kernel_alone": (run(plan, "bicubic"), direct, True),
                "d_bilinear_fused_k1p": (run(fplan, "bilinear"), direct, True)}
        ms = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, (fn, knob, graph) in arms.items():
                if k == "ck_tables_kernel_alone":
                    plan.device_tables(src.device)
                with _native.testing_knob(*knob):
                    ms[k].append(bc._timed(fn, args.steps, 1, graph=graph)[0])
        flags.raise_if_set("time_proj_bicubic")
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        a = med["a_k1pq_staged"]
        line = json.dumps({"label": args.label, "source": [size, size], "target": [tsize, tsize],
                           "div": div, "dtype": "float32", "out": "float64",
                           "covered_px": covered, "ms_median": med,
                           "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
                           "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
                           "global_over_staged": round(med["b_k1pq_16tap_global"] / a, 3),
                           "tables_over_staged":
                               round(med["c_transform_plus_tables_kernel"] / a, 3),
                           "staged_over_bilinear": round(a / med["d_bilinear_fused_k1p"], 3)})
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        plan._device_cache.clear()
        del out


if __name__ == "__main__":
    main()
