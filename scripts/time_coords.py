"""K8 (xrs_coords_stats) and GridMapping.from_coords timed on one box, one run:
  * the K8 launch pair (pass + fold) on a 4000 x 4800 swath (config 4's size),
    geographic and projected, and K4 (xrs_ij_bboxes_fill over a tile grid, with
    its small upload) on the same arrays for scale — device events around
    `reps` launches, the three alternating within every round;
  * GridMapping.from_coords on that swath (geographic): numpy input with the
    device path forced off (the parent commit's host analysis) and forced on
    (upload + K8), and device-tensor input — host clock around the call, which
    ends in the read-back, alternating within every round;
  * the same off / on pair for square numpy swaths of growing size: the
    smallest size from which "on" stays quicker is the crossover that sets the
    default of the ``coords_device_min_points`` option.
Writes one JSON line (medians over the rounds, all samples kept).
    python scripts/time_coords.py [--rounds N] [--reps K] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 4000, 4800
CROSSOVER_SIDES = (128, 256, 512, 724, 1024, 1448, 2048)


def swath(h, w, geographic):
    jj, ii = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64),
                         indexing="ij")
    u = ii + 0.2 * jj + 40.0 * np.sin(0.3 + 0.0011 * ii + 0.0007 * jj)
    v = jj - 0.15 * ii + 30.0 * np.cos(0.9 + 0.0005 * ii + 0.0013 * jj)
    if geographic:
        return 5.0 + 0.003 * u, 62.0 - 0.0027 * v
    return 4.0e6 + 300.0 * u, 3.2e6 - 270.0 * v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coords_stats.jsonl"))
    args = ap.parse_args()

    import torch

    import xcube_resampling_amd as xrs
    from xcube_resampling_amd import _native, kernels
    from xcube_resampling_amd.device import ptr, stream_handle

    assert torch.cuda.is_available(), "time_coords.py needs a HIP device"
    dev = torch.device("cuda", 0)
    lib = _native.lib()
    geo = swath(H, W, True)
    prj = swath(H, W, False)
    geo_d = tuple(torch.from_numpy(a).to(dev) for a in geo)
    prj_d = tuple(torch.from_numpy(a).to(dev) for a in prj)
    nbytes = lib.xrs_coords_stats_workspace_size(H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rec = torch.empty(48, dtype=torch.uint8, device=dev)

    def k8(xy, geographic):
        rc = lib.xrs_coords_stats(ptr(xy[0]), ptr(xy[1]), H, W, W, geographic, ptr(rec), ptr(ws),
                                  nbytes, stream_handle(dev))
        _native.check(rc, "xrs_coords_stats")

    # K4 over a 10 x 8 grid of tiles covering the projected swath
    xe = np.linspace(prj[0].min(), prj[0].max(), 11)
    ye = np.linspace(prj[1].min(), prj[1].max(), 9)
    boxes = np.array([[xe[i], ye[j], xe[i + 1], ye[j + 1]] for j in range(8) for i in range(10)])

    def k4():
        kernels._ij_bboxes_launch(prj_d[0], prj_d[1], boxes, 0.0, (10, 8), dev, None)

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def from_coords_s(xy, min_points, crs):
        with xrs.set_options(coords_device_min_points=min_points):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gm = xrs.GridMapping.from_coords(xrs.DataArray(xy[0], ("y", "x")),
                                             xrs.DataArray(xy[1], ("y", "x")), crs)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, gm

    launches = {"k8_geographic": lambda: k8(geo_d, 1), "k8_projected": lambda: k8(prj_d, 0),
                "k4_ij_bboxes": k4}
    hosts = {"numpy_off": (geo, 1 << 60), "numpy_on": (geo, 0), "device": (geo_d, 1 << 60)}
    for fn in launches.values():   # warm-up: code objects, clocks
        device_ms(fn)
    gms = {k: from_coords_s(xy, mp, "EPSG:4326")[1] for k, (xy, mp) in hosts.items()}
    fields = ("xy_res", "xy_bbox", "is_regular", "is_lon_360", "is_j_axis_up", "size")
    for k, gm in gms.items():   # faster and different is not faster
        assert all(getattr(gm, f) == getattr(gms["numpy_off"], f) for f in fields), k

    samples = {k: [] for k in list(launches) + list(hosts)}
    for _ in range(args.rounds):
        for k, fn in launches.items():
            samples[k].append(device_ms(fn))
        for k, (xy, mp) in hosts.items():
            samples[k].append(from_coords_s(xy, mp, "EPSG:4326")[0])

    cross = []
    for side in CROSSOVER_SIDES:
        xy = swath(side, side, True)
        t = {"off": [], "on": []}
        from_coords_s(xy, 0, "EPSG:4326")
        for _ in range(max(3, args.rounds)):
            t["off"].append(from_coords_s(xy, 1 << 60, "EPSG:4326")[0])
            t["on"].append(from_coords_s(xy, 0, "EPSG:4326")[0])
        cross.append({"points": side * side, "off_s": statistics.median(t["off"]),
                      "on_s": statistics.median(t["on"])})
    slower = [i for i, c in enumerate(cross) if c["on_s"] >= c["off_s"]]
    first = slower[-1] + 1 if slower else 0
    med = {k: statistics.median(v) for k, v in samples.items()}
    line = {
        "what": "coords_stats", "device": torch.cuda.get_device_name(0), "shape": [H, W],
        "rounds": args.rounds, "reps": args.reps,
        "k8_geographic_ms": med["k8_geographic"], "k8_projected_ms": med["k8_projected"],
        "k4_ij_bboxes_ms": med["k4_ij_bboxes"],
        "k8_bytes": 16 * H * W,
        "k8_geographic_gbps": 16 * H * W / med["k8_geographic"] / 1e6,
        "k8_projected_gbps": 16 * H * W / med["k8_projected"] / 1e6,
        "from_coords_numpy_off_s": med["numpy_off"], "from_coords_numpy_on_s": med["numpy_on"],
        "from_coords_device_s": med["device"],
        "ratio_numpy_off_over_on": med["numpy_off"] / med["numpy_on"],
        "ratio_numpy_off_over_device": med["numpy_off"] / med["device"],
        "crossover": cross,
        "crossover_points": cross[first]["points"] if first < len(cross) else None,
        "samples": samples,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps({k: v for k, v in line.items() if k != "samples"}))


if __name__ == "__main__":
    main()
