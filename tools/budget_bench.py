"""What the power budget (Engine.set_budget) costs and how
well it closes: the synthetic scene and the eye, 1 M emitted rays, aggregate
mode (lpc_trace_run on device-resident rays).  The ledger is switched off and on
in alternation within one process, `reps` timed traces each after one untimed
trace per setting; per scene the median trace time off and on, the ledger's
categories, `left` and the `closure` observed.

    python tools/budget_bench.py [--rays N] [--reps 7] [--scenes synthetic,eye]
                                 [--out profiles/budget_bench.json] [--md FILE]

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


def rays_of(sc):
    o = np.concatenate([np.asarray(s.rays_origin, np.float32) for s in sc.sources])
    d = np.concatenate([np.asarray(s.rays_dir, np.float32) for s in sc.sources])
    p = np.concatenate([np.asarray(s.rays_power, np.float32).reshape(-1) for s in sc.sources])
    return o, d, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--scenes", default="synthetic,eye")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "budget_bench.json"))
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    from lightpycl_amd import scenes
    from lightpycl_amd.build import build
    from lightpycl_amd.engine import Engine
    from lightpycl_amd.iterative_tracer import budget_dict
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
            times = {False: [], True: []}
            base = bud = None
            for rep in range(1 + a.reps):               # rep 0: untimed (buffers, speculation history)
                for on in (False, True):
                    e.set_budget(on)
                    e.sync()
                    t0 = time.perf_counter()
                    stats, (cnt, mp) = e.run_local(sc.iterations, thr, reset=True)
                    dt = (time.perf_counter() - t0) * 1e3
                    got = ([int(s.n_in) for s in stats], int(cnt), [float(x) for x in mp],
                           [float(s.power_next) for s in stats])
                    if base is not None and got != base:  # the ledger changes no result
                        raise SystemExit("%s: trace (ledger %s) differs from the first" % (name, on))
                    base = base or got
                    if on:
                        bud = budget_dict(e.budget())
                        if [int(v) for v in bud["n_in"]] != got[0]:
                            raise SystemExit("%s: the ledger's populations differ from the trace's" % name)
                    if rep > 0:
                        times[on].append(dt)
        finally:
            e.close()
        off, on = statistics.median(times[False]), statistics.median(times[True])
        cat = {k: float(np.sum(bud[k])) for k in ("dissipated", "escaped", "terminated", "measured", "absorbed")}
        rows.append(dict(scene=name, rays=len(p), meshes=len(sc.meshes), iterations=len(base[0]),
                         ray_bounces=int(sum(base[0])), ms_off=off, ms_on=on, ms_off_all=times[False],
                         ms_on_all=times[True], power_in=float(bud["power_in"][0]), left=bud["left"],
                         closure=bud["closure"], closure_rel=abs(bud["closure"]) / abs(float(bud["power_in"][0])),
                         **cat))
        print(json.dumps(rows[-1]), flush=True)
    lines = ["| scene | iterations | ray-bounces | ms / trace, ledger off (median of %d) | ledger on | cost | "
             "power in | measured | escaped | dissipated | absorbed | terminated | left | closure |" % a.reps,
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s, %d rays, %d meshes | %d | %d | %.3f | %.3f | %+.1f %% | %.9g | %.9g | %.6g | %.6g | %.6g | "
                     "%.6g | %.6g | %.3g |" % (
                         r["scene"], r["rays"], r["meshes"], r["iterations"], r["ray_bounces"], r["ms_off"],
                         r["ms_on"], 100.0 * (r["ms_on"] / r["ms_off"] - 1.0), r["power_in"], r["measured"],
                         r["escaped"], r["dissipated"], r["absorbed"], r["terminated"], r["left"], r["closure"]))
    md = "\n".join(lines)
    print(md)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(dict(workload="aggregate trace (lpc_trace_run, reset + trace), device-resident rays, "
                                "ledger off / on alternating", reps=a.reps, rows=rows), fh, indent=1)
    if a.md:
        with open(a.md, "w") as fh:
            fh.write(md + "\n")


if __name__ == "__main__":
    main()
