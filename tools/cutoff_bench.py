"""What the per-ray power cutoff (Engine.set_min_power) buys
on the multi-bounce scenes: eye and synthetic_dense, 1 M emitted rays, aggregate
mode (lpc_trace_run on device-resident rays), cut in {0, 1e-6 p0, 1e-4 p0} with
p0 = input power / ray count.  Per cut: one cold trace (no speculation history
under that cutoff), then the median of 5; ray-bounces, peak population, measured
power and its difference from cut 0, culled count and power.

    python tools/cutoff_bench.py [--rays N] [--reps 5] [--scenes eye,synthetic_dense]
                                 [--out profiles/cutoff_bench.json] [--md FILE]

Writes the JSON record and prints a markdown table (also to --md)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rays_of(sc):
    o = np.concatenate([np.asarray(s.rays_origin, np.float32) for s in sc.sources])
    d = np.concatenate([np.asarray(s.rays_dir, np.float32) for s in sc.sources])
    p = np.concatenate([np.asarray(s.rays_power, np.float32).reshape(-1) for s in sc.sources])
    return o, d, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="eye,synthetic_dense")
    ap.add_argument("--fractions", default="0,1e-6,1e-4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cutoff_bench.json"))
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
        in_pow = float(np.sum(p, dtype=np.float64))
        thr = (1.0 - sc.tau) * in_pow
        e = Engine(0)
        try:
            e.upload_meshes(sc.meshes)
            e.set_rays(o, d, p, sc.max_ray_len, sc.ior_env)
            base = None
            for f in [float(x) for x in a.fractions.split(",")]:
                cut = np.float32(f * in_pow / len(p))
                e.set_min_power(cut)
                times, last, cold = [], None, None
                for rep in range(1 + a.reps):
                    e.sync()
                    t0 = time.perf_counter()
                    stats, (cnt, mp) = e.run_local(sc.iterations, thr, reset=True)
                    times.append((time.perf_counter() - t0) * 1e3)
                    cc, cp = e.culled()
                    got = ([int(s.n_in) for s in stats], int(cnt), [float(x) for x in mp], cc.tolist(),
                           cp.tolist())
                    # counts and per-mesh power repeat exactly; the ledger's float64 sums bit
                    # for bit between traces that take the same launch path (the warm ones),
                    # and to summation order against the cold trace
                    if rep == 0:
                        cold = got
                    for k, what in enumerate(("populations", "measured count", "mesh power", "culled counts")):
                        if got[k] != cold[k]:
                            raise SystemExit("trace %d differs in %s: %r != %r" % (rep, what, cold[k], got[k]))
                    if not np.allclose(got[4], cold[4], rtol=1e-12, atol=0.0):
                        raise SystemExit("trace %d: culled power %r != %r" % (rep, cold[4], got[4]))
                    if rep >= 2 and got != last:
                        raise SystemExit("warm traces differ: %r != %r" % (last, got))
                    last = got
                cold_bits = cold[4] == last[4]
                counts, cnt, mp, cc, cp = last
                measured = math.fsum(mp)
                base = measured if base is None else base
                rows.append(dict(scene=name, rays=len(p), fraction=f, cut=float(cut), iterations=len(counts),
                                 ms_cold=times[0], ms_median=statistics.median(times[1:]), ms_all=times[1:],
                                 ray_bounces=int(sum(counts)), peak_population=int(max(counts)),
                                 measured_count=cnt, measured_power=measured, measured_power_diff=base - measured,
                                 culled_count=int(sum(cc)), culled_power=math.fsum(cp), populations=counts,
                                 ledger_bits_cold_equals_warm=bool(cold_bits)))
                print(json.dumps(rows[-1]), flush=True)
        finally:
            e.close()
    lines = ["| scene | cut | iterations | ms / trace (cold) | ms / trace (median of %d) | ray-bounces | "
             "peak population | measured power | difference from cut 0 | culled power (rays) |" % a.reps,
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s, %d rays | %s | %d | %.1f | %.1f | %d | %d | %.9g | %.3g | %.3g (%d) |" % (
            r["scene"], r["rays"], "0" if r["fraction"] == 0 else "%g·p0" % r["fraction"], r["iterations"],
            r["ms_cold"], r["ms_median"], r["ray_bounces"], r["peak_population"], r["measured_power"],
            r["measured_power_diff"], r["culled_power"], r["culled_count"]))
    md = "\n".join(lines)
    print(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(workload="aggregate trace (lpc_trace_run, reset + trace), device-resident rays",
                       reps=a.reps, rows=rows), fh, indent=1)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(md + "\n")


if __name__ == "__main__":
    main()
