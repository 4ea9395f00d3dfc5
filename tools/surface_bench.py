"""What the surface map (Engine.set_surface) costs: three
workloads of 1 M emitted rays in aggregate mode (lpc_trace_run on device-resident
rays) --

    synthetic   the synthetic scene: an iteration spreads over ~100 000 triangles
    eye         the eye: many iterations
    beam        a collimated beam onto one face of a terminator cube: a whole
                1 M-ray iteration on two triangles, the case that shows whether
                k_surface_sum's merge works

The map is switched off and on in alternation within one process, `reps` timed
traces each after one untimed trace per setting; per workload the median trace
time off and on, the triangles hit and the largest count on one triangle.

    python tools/surface_bench.py [--rays N] [--reps 7] [--scenes synthetic,eye,beam]
                                  [--out profiles/surface_bench.json] [--md FILE]

Writes the JSON record and prints a markdown table (also to --md)."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rays_of(sc):
    o = np.concatenate([np.asarray(s.rays_origin, np.float32) for s in sc.sources])
    d = np.concatenate([np.asarray(s.rays_dir, np.float32) for s in sc.sources])
    p = np.concatenate([np.asarray(s.rays_power, np.float32).reshape(-1) for s in sc.sources])
    return o, d, p


def beam_scene(n):
    """n parallel rays along +z, uniform over an 8 x 8 square, onto the z = 15 face
    of a terminator cube of edge 10 centred at (0, 0, 20): every ray ends on one of
    the face's two triangles in the first iteration."""
    from lightpycl_amd import geo_optical_elements as goe
    cube = goe.optical_elements().cube(center=(0, 0, 20, 0), size=[10, 10, 10, 0])
    cube.setMaterial(mat_type="terminator")
    rng = np.random.RandomState(7)
    o = np.zeros((n, 4), np.float32)
    o[:, :2] = rng.uniform(-4.0, 4.0, (n, 2))
    d = np.zeros((n, 4), np.float32)
    d[:, 2] = 1.0
    p = np.full(n, 1000.0 / n, np.float32)
    src = types.SimpleNamespace(rays_origin=o, rays_dir=d, rays_power=p)
    return types.SimpleNamespace(name="beam", meshes=[cube], sources=[src], iterations=4, tau=0.99,
                                 max_ray_len=np.float32(1e3), ior_env=np.float32(1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="synthetic,eye,beam")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_bench.json"))
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    from lightpycl_amd import scenes
    from lightpycl_amd.build import build
    from lightpycl_amd.engine import Engine
    build(verbose=False)
    rows = []
    for name in a.scenes.split(","):
        sc = beam_scene(a.rays) if name == "beam" else scenes.BUILDERS[name](n=a.rays)
        o, d, p = rays_of(sc)
        in_pow = float(np.sum(p, dtype=np.float64))
        thr = (1.0 - sc.tau) * in_pow
        e = Engine(0)
        try:
            e.upload_meshes(sc.meshes)
            e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
            times = {False: [], True: []}
            base = surf = None
            for rep in range(1 + a.reps):               # rep 0: untimed (buffers, speculation history)
                for on in (False, True):
                    e.set_surface(on)
                    e.sync()
                    t0 = time.perf_counter()
                    stats, (cnt, mp) = e.run_local(sc.iterations, thr, reset=True)
                    e.sync()                            # (the last commit included)
                    dt = (time.perf_counter() - t0) * 1e3
                    got = ([int(s.n_in) for s in stats], int(cnt), [float(x) for x in mp],
                           [float(s.power_next) for s in stats])
                    if base is not None and got != base:  # the map changes no result
                        raise SystemExit("%s: trace (map %s) differs from the first" % (name, on))
                    base = base or got
                    if on:
                        surf = e.surface()
                    if rep > 0:
                        times[on].append(dt)
        finally:
            e.close()
        off, on = statistics.median(times[False]), statistics.median(times[True])
        hits = int(surf["count"].sum())
        rows.append(dict(scene=name, rays=len(p), meshes=len(sc.meshes), triangles=len(surf["count"]),
                         iterations=len(base[0]), ray_bounces=int(sum(base[0])), hits=hits,
                         triangles_hit=int(np.count_nonzero(surf["count"])), max_count=int(surf["count"].max()),
                         incident=float(surf["incident"].sum()), deposited=float(surf["deposited"].sum()),
                         ms_off=off, ms_on=on, ms_off_all=times[False], ms_on_all=times[True]))
        print(json.dumps(rows[-1]), flush=True)
    lines = ["| workload | triangles | iterations | ray-bounces | hits | triangles hit | most hits on one triangle | "
             "ms / trace, map off (median of %d) | map on | cost | cost per hit [ns] |" % a.reps,
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s, %d rays, %d meshes | %d | %d | %d | %d | %d | %d | %.3f | %.3f | %+.1f %% | %.3f |" % (
            r["scene"], r["rays"], r["meshes"], r["triangles"], r["iterations"], r["ray_bounces"], r["hits"],
            r["triangles_hit"], r["max_count"], r["ms_off"], r["ms_on"], 100.0 * (r["ms_on"] / r["ms_off"] - 1.0),
            1e6 * (r["ms_on"] - r["ms_off"]) / max(r["hits"], 1)))
    md = "\n".join(lines)
    print(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(workload="aggregate trace (lpc_trace_run, reset + trace, then lpc_sync), device-resident rays, "
                                "surface map off / on alternating", reps=a.reps, rows=rows), fh, indent=1)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(md + "\n")


if __name__ == "__main__":
    main()
