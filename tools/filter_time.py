"""Times of the denoise mode (settings "filter" and "TAA") on one MI355X, and the regression of the frame with the filter
off, and with the filter on but TAA off, against another build.

  python tools/filter_time.py --out profiles/NAME_filter_time.json [--parent-tree DIR]

Per configuration (config 2: 100k random triangles, primary + one bounce; config 3: the 1M-triangle room, maxPathLength 4;
both 1920 x 1080, 1 spp): CoreStats::filterTime and the kernels' times (HIP events: the launches' own stop events), means
over --frames frames after --warmup, for the taps (of the a-trous passes and the TAA pass) from the LDS tile, through
L1 / L2, and the default pick, without TAA
(four kernels) and with it (six: rows "taa_lds", "taa_l2", "taa_default"); the frame time with the filter off, on, and on
with TAA; and the bytes-per-pixel floor of each kernel against 8 TB/s.
With --parent-tree (a built checkout of the parent commit: its lighthouse2_amd package with the library) the frame times
with the filter off, and with "filter" 1 and "TAA" left alone, of this build and of that one are taken in fresh child
processes, alternating, --repeats times each: the parent's own spread is the yardstick of the difference."""
from __future__ import annotations

import argparse
import json
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
# child mode (--off-only --tree DIR): the package of that tree, not this one
TREE = pathlib.Path(sys.argv[sys.argv.index("--tree") + 1]).resolve() if "--tree" in sys.argv else ROOT
sys.path.insert(0, str(TREE))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime in the process)

from lighthouse2_amd import core as lh2core, scene  # noqa: E402

W, H = 1920, 1080
# unique bytes per pixel each kernel has to move (16 B records unless noted)
FLOOR_BYTES = {
    "prepare": 32 + 16 + 16 + 16 + 16 + 16 + 16 + 8 + 16 + 4,   # acc x 2, features, worldPos, deltaDepth, prevWorldPos, prevMoments in; shading, motion (8), moments, features.w (4) out
    "atrous1": 80 + 16 + 16 + 16 + 8,                           # + previous pass-1 output, worldPos, prevWorldPos, motion (8)
    "atrous2": 80,                                              # A, features, deltaDepth, moments in; C out
    "atrous3": 80,
    "taa": 16 + 8 + 16 + 16,                                    # linear, motion (8), the history in; the TAA pixels out
    "unsharpen": 16 + 16,                                       # the TAA pixels in; the frame out
}
PEAK = 8e12


def configs(room_tris):
    yield "config2", scene.config2_scene(n=100_000, width=W, height=H), {}
    yield "config3", scene.room_scene(room_tris, W, H), {"maxPathLength": 4}


def frame_ms(core, sc, frames, warmup):
    for i in range(warmup):
        sc.render_frame(core, converge=1 if i == 0 else 0)
    core.sync()
    t0 = time.perf_counter()
    for i in range(frames):
        sc.render_frame(core, converge=0)
    core.sync()
    return (time.perf_counter() - t0) / frames * 1e3


def filter_ms(core, sc, frames, warmup, taa=False):
    """Mean filterTime and kernel times (ms) over `frames` frames, each read after its frame; taa: the TAA stage's two as well."""
    for i in range(warmup):
        sc.render_frame(core, converge=1 if i == 0 else 0)
    rows, total = [], []
    for i in range(frames):
        sc.render_frame(core, converge=0)
        total.append(core.stats().filterTime * 1e3)
        rows.append(np.concatenate([core.filter_times(), core.taa_times()]) if taa else core.filter_times())
    k = np.mean(rows, 0)
    return float(np.mean(total)), {n: float(v) for n, v in zip(("prepare", "atrous1", "atrous2", "atrous3", "taa", "unsharpen"), k)}


def off_only(args):
    out = {"version": lh2core.load_library().lh2_version().decode()}
    for name, sc, settings in configs(args.room_tris):
        c = lh2core.RenderCore(device=0)
        for k, v in settings.items():
            c.setting(k, v)
        sc.load_into(c)
        c.set_target(W, H, 1)
        out[name] = round(frame_ms(c, sc, args.frames, args.warmup), 4)
        c.setting("filter", 1)      # "TAA" as the build has it: off, or not known
        out[name + "_filter_on"] = round(frame_ms(c, sc, args.frames, args.warmup), 4)
        c.close()
    print("FILTER_OFF " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--room-tris", type=int, default=1_000_000)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--off-only", action="store_true", help="child mode: print the frame times, filter off and on, of the build in --tree")
    ap.add_argument("--tree", default="")
    args = ap.parse_args()
    if args.off_only:
        return off_only(args)
    rec = {"size": [W, H], "frames": args.frames, "warmup": args.warmup, "version": lh2core.load_library().lh2_version().decode(),
           "floor": {k: {"bytes_per_pixel": b, "ms_at_8TBs": round(b * W * H / PEAK * 1e3, 4)} for k, b in FLOOR_BYTES.items()}}
    for name, sc, settings in configs(args.room_tris):
        c = lh2core.RenderCore(device=0)
        for k, v in settings.items():
            c.setting(k, v)
        sc.load_into(c)
        c.set_target(W, H, 1)
        r = {"frame_ms_filter_off": round(frame_ms(c, sc, args.frames, args.warmup), 4)}
        c.setting("filter", 1)
        for label, lds in (("lds", 1), ("l2", 0), ("default", -1)):
            c.setting("filterLds", lds)
            total, kernels = filter_ms(c, sc, args.frames, args.warmup)
            r[label] = {"filterTime_ms": round(total, 4), "kernels_ms": {k: round(v, 4) for k, v in kernels.items()}}
        r["frame_ms_filter_on"] = round(frame_ms(c, sc, args.frames, args.warmup), 4)
        c.setting("TAA", 1)
        for label, lds in (("taa_lds", 1), ("taa_l2", 0), ("taa_default", -1)):
            c.setting("filterLds", lds)
            total, kernels = filter_ms(c, sc, args.frames, args.warmup, taa=True)
            r[label] = {"filterTime_ms": round(total, 4), "kernels_ms": {k: round(v, 4) for k, v in kernels.items()}}
        r["frame_ms_filter_taa_on"] = round(frame_ms(c, sc, args.frames, args.warmup), 4)
        c.close()
        rec[name] = r
        print(name, json.dumps(r), flush=True)
    if args.parent_tree:
        runs = {"parent": [], "branch": []}
        for _ in range(args.repeats):
            for label, tree in (("parent", args.parent_tree), ("branch", "")):
                cmd = [sys.executable, __file__, "--off-only", "--frames", str(args.frames), "--warmup", str(args.warmup),
                       "--room-tris", str(args.room_tris)] + (["--tree", tree] if tree else [])
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("FILTER_OFF ")]
                if p.returncode != 0 or not line:
                    raise SystemExit(f"{label} run failed ({p.returncode}): {p.stderr[-2000:]}")
                runs[label].append(json.loads(line[0][len("FILTER_OFF "):]))
                print(label, runs[label][-1], flush=True)
        reg = {"parent_version": runs["parent"][0]["version"], "branch_version": runs["branch"][0]["version"]}
        for cfg in ("config2", "config3", "config2_filter_on", "config3_filter_on"):
            pa, br = [r[cfg] for r in runs["parent"]], [r[cfg] for r in runs["branch"]]
            reg[cfg] = {"parent_ms": pa, "branch_ms": br, "parent_spread_ms": round(max(pa) - min(pa), 4),
                        "difference_of_means_ms": round(float(np.mean(br) - np.mean(pa)), 4)}
        rec["filter_off_regression"] = reg
        print("regression", json.dumps(reg), flush=True)
    if args.out:
        pathlib.Path(args.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
