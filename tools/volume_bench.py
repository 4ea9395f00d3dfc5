"""What the volume map (Engine.set_volume) costs: traces of
1 M emitted rays in aggregate mode (lpc_trace_run on device-resident rays), one
trace at a time --

    cube        the dissipative cube (scenes.cube): every ray that enters the cube
                dissipates along its path through it; grids of 64^3 and 256^3
                voxels over the cube
    eye         the eye, whose media do not dissipate: no segment is booked, the
                cost of the map is the zeroing and the commit of its table

The map is switched off and on in alternation within one process, `reps` timed
traces each after one untimed trace per setting; per workload and grid the
median trace time off and on with the range of the timed traces, the segments
booked and the voxels touched.

    python tools/volume_bench.py [--rays N] [--reps 7] [--scenes cube,eye] [--grids 64,256]
                                 [--out profiles/volume_bench.json] [--md FILE]

Writes the JSON record and prints a markdown table (also to --md)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOXES = {"cube": ((-5.0, -5.0, 15.0), (5.0, 5.0, 25.0)),      # the cube itself
         "eye": None}                                         # the scene's bounding box


def rays_of(sc):
    o = np.concatenate([np.asarray(s.rays_origin, np.float32) for s in sc.sources])
    d = np.concatenate([np.asarray(s.rays_dir, np.float32) for s in sc.sources])
    p = np.concatenate([np.asarray(s.rays_power, np.float32).reshape(-1) for s in sc.sources])
    return o, d, p


def scene_box(sc):
    v = np.concatenate([np.asarray(m.vertices, np.float64)[:, :3] for m in sc.meshes])
    return tuple(v.min(axis=0) - 1e-3), tuple(v.max(axis=0) + 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="cube,eye")
    ap.add_argument("--grids", default="64,256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume_bench.json"))
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    from lightpycl_amd import scenes
    from lightpycl_amd.build import build
    from lightpycl_amd.engine import Engine
    build(verbose=False)
    rows = []
    for name in a.scenes.split(","):
        sc = scenes.BUILDERS[name](n=a.rays)
        o, d, p = rays_of(sc)
        thr = (1.0 - sc.tau) * float(np.sum(p, dtype=np.float64))
        lo, hi = BOXES.get(name) or scene_box(sc)
        e = Engine(0)
        try:
            e.upload_meshes(sc.meshes)
            e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
            for g in (int(x) for x in a.grids.split(",")):
                times = {False: [], True: []}
                base = vol = None
                for rep in range(1 + a.reps):           # rep 0: untimed (buffers, speculation history)
                    for on in (False, True):
                        if on:
                            e.set_volume(lo, hi, (g, g, g))
                        else:
                            e.set_volume(None)
                        e.sync()
                        t0 = time.perf_counter()
                        stats, (cnt, mp) = e.run_local(sc.iterations, thr, reset=True)
                        e.sync()                        # (the last commit included)
                        dt = (time.perf_counter() - t0) * 1e3
                        got = ([int(s.n_in) for s in stats], int(cnt), [float(x) for x in mp],
                               [float(s.power_next) for s in stats])
                        if base is not None and got != base:    # the map changes no result
                            raise SystemExit("%s: trace (map %s) differs from the first" % (name, on))
                        base = base or got
                        if on:
                            vol = e.volume()
                        if rep > 0:
                            times[on].append(dt)
                off, on = statistics.median(times[False]), statistics.median(times[True])
                rows.append(dict(scene=name, rays=len(p), grid=g, voxels=g ** 3, iterations=len(base[0]),
                                 ray_bounces=int(sum(base[0])), segments=vol["segments"],
                                 voxels_touched=int(np.count_nonzero(vol["deposited"])),
                                 deposited=float(vol["deposited"].sum()), outside=vol["outside"],
                                 ms_off=off, ms_on=on, ms_off_all=times[False], ms_on_all=times[True]))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            e.close()
    lines = ["| workload | grid | iterations | ray-bounces | segments | voxels touched | ms / trace, map off "
             "(median of %d; min - max) | map on | cost | cost per segment [ns] |" % a.reps,
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s, %d rays | %d^3 | %d | %d | %d | %d | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %+.1f %% | %s |" % (
            r["scene"], r["rays"], r["grid"], r["iterations"], r["ray_bounces"], r["segments"], r["voxels_touched"],
            r["ms_off"], min(r["ms_off_all"]), max(r["ms_off_all"]), r["ms_on"], min(r["ms_on_all"]),
            max(r["ms_on_all"]), 100.0 * (r["ms_on"] / r["ms_off"] - 1.0),
            "%.3f" % (1e6 * (r["ms_on"] - r["ms_off"]) / r["segments"]) if r["segments"] else "-"))
    md = "\n".join(lines)
    print(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(workload="aggregate trace (lpc_trace_run, reset + trace, then lpc_sync), device-resident rays, "
                                "volume map off / on alternating", reps=a.reps, rows=rows), fh, indent=1)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(md + "\n")


if __name__ == "__main__":
    main()
