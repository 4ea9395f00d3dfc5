"""GPU box: the 2-D maps after an aggregate-mode trace, host path against device
path on the same trace.

Lens scene, ``keep_results=False``; then ``replicate_lightsources_and_plot(plot=False)``
with 36 sources at ``points=500`` and ``points=100`` and ``get_binned_data`` at
``points=500``, each timed once cold and as the median of 5 further calls, with
``on_device=False`` (what the parent commit runs: one projection launch per source,
points copied back, np.histogram2d on one core) and ``on_device=True`` (one
``lpc_map_hist`` call); the bytes the engine returns to the host; the map kernel's
own time from the launch's HIP events (``lpc_prof``'s kernel_ms), without and with
the per-bin statistics, and the bytes it accumulates per second.  ``--sweep`` adds
the kernel's time under the A/B switches (LPC_MAP_SLICES, LPC_MAP_PER_CU) on engines of
their own, fed the same measured rays as host points.  Prints one JSON line.

    python tools/map_bench.py [rays] [--sweep] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightpycl_amd import scenes  # noqa: E402
from lightpycl_amd.engine import Engine  # noqa: E402
from lightpycl_amd.iterative_tracer import CL_Tracer  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--out" in sys.argv:
    out = sys.argv[sys.argv.index("--out") + 1]
    args = [a for a in args if a != out]
else:
    out = None
n = int(args[0]) if args else 1_000_000
REPS = 5
ATOMIC_FLOOR_TBS = 1.3          # chip-wide rate of global float atomics in their best shape (added bytes)

# bytes that cross to the host: the arrays the engine's calls return
fetched = [0]


def _count(x):
    if isinstance(x, np.ndarray):
        fetched[0] += x.nbytes
    elif isinstance(x, (tuple, list)):
        for y in x:
            _count(y)


def _wrap(name):
    fn = getattr(Engine, name)

    def counted(self, *a, **k):
        r = fn(self, *a, **k)
        _count(r)
        return r
    setattr(Engine, name, counted)


for name in ("fetch_measured", "project_hist", "map_hist"):
    _wrap(name)


def note(msg):
    print("[map_bench] " + msg, file=sys.stderr, flush=True)


sc = scenes.lens(n=n, seed=7)
tr = CL_Tracer(device=0)
t = time.perf_counter()
tr.iterative_tracer(sc.sources, sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                    max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=False)
trace_ms = (time.perf_counter() - t) * 1e3
measured = int(tr.engine.measured()[0])
note("traced %d rays in %.1f ms, %d measured" % (n, trace_ms, measured))

ANG = ((-np.pi / 2, np.pi / 2), (-np.pi / 2, np.pi / 2))
PLANE = ((-1000.0, 1000.0), (-1000.0, 1000.0))
ROWS = dict(
    replicate36_p500=(lambda dev: tr.replicate_lightsources_and_plot(limits=ANG, points=500, sources=36, plot=False,
                                                                     on_device=dev), 0, ANG, 500, 36),
    replicate36_p100=(lambda dev: tr.replicate_lightsources_and_plot(limits=ANG, points=100, sources=36, plot=False,
                                                                     on_device=dev), 0, ANG, 100, 36),
    planar_p500=(lambda dev: tr.get_binned_data(limits=PLANE, points=500, on_device=dev), 2, PLANE, 500, 1),
)


def kernel_ms(eng, reps, **kw):
    """Median of the map kernel's own time over `reps` calls (HIP events of the launch)."""
    eng.prof_enable(True)
    ms = []
    try:
        for _ in range(reps):
            eng.prof_read(reset=True)
            eng.map_hist(**kw)
            ms.append(eng.prof_read(reset=True)["kernel_ms"])
    finally:
        eng.prof_enable(False)
    return statistics.median(ms)


rec = dict(tool="map_bench", scene="lens", rays=n, measured_rays=measured, first_trace_ms=round(trace_ms, 3),
           reps=REPS, atomic_floor_TBps=ATOMIC_FLOOR_TBS, results={})
for name, (call, mode, lim, pts, sources) in ROWS.items():
    row = {}
    H = {}
    for dev in (False, True):
        times = []
        for k in range(REPS + 1):
            fetched[0] = 0
            t = time.perf_counter()
            H[dev] = call(dev)[0]
            times.append((time.perf_counter() - t) * 1e3)
            note("%s %s call %d: %.1f ms" % (name, "device" if dev else "host", k, times[-1]))
        row["device" if dev else "host"] = dict(cold_ms=round(times[0], 3),
                                                median_ms=round(statistics.median(times[1:]), 3),
                                                bytes_returned=fetched[0])
    row["speedup_median"] = round(row["host"]["median_ms"] / row["device"]["median_ms"], 2)
    row["max_rel_diff"] = float(np.max(np.abs(H[True] - H[False])) / max(np.max(np.abs(H[False])), 1e-300))
    rots = CL_Tracer._source_rots("z", sources) if sources > 1 else None
    for stats in (False, True):
        ms = kernel_ms(tr.engine, REPS, pos4=None, pwr=None, limits=lim, points=pts, mode=mode, rots=rots, stats=stats)
        added = measured * sources * 8 * (3 if stats else 1)
        row["kernel_stats" if stats else "kernel"] = dict(median_ms=round(ms, 4), accumulated_bytes=added,
                                                          accumulated_TBps=round(added / (ms * 1e-3) / 1e12, 4))
    rec["results"][name] = row

if "--sweep" in sys.argv:
    # the A/B switches are read when a handle opens: engines of their own, the same rays as host points
    pos, pw, _ = tr.engine.fetch_measured()
    sweep = {}
    rots36 = CL_Tracer._source_rots("z", 36)
    shapes = {("p%d%s" % (pts, "_stats" if st else "")): (pts, st)
              for pts in (30, 100, 128, 200, 300, 500) for st in (False, True)}
    variants = [("lds_sliced", dict(LPC_MAP_SLICES="64"), None), ("global_8", dict(LPC_MAP_SLICES="0"), None)] + [
        ("global_%d" % c, dict(LPC_MAP_SLICES="0", LPC_MAP_PER_CU=str(c)), 500) for c in (2, 32)]
    for vname, env, only in variants:
        os.environ.update(env)
        eng = Engine(0)
        try:
            for sname, (pts, stats) in shapes.items():
                if only is not None and pts != only:
                    continue
                ms = kernel_ms(eng, 3, pos4=pos, pwr=pw, limits=ANG, points=pts, mode=0, rots=rots36, stats=stats)
                sweep.setdefault(sname, {})[vname] = round(ms, 4)
                note("sweep %s %s: %.3f ms" % (sname, vname, ms))
        finally:
            eng.close()
            for k in env:
                os.environ.pop(k, None)
    rec["sweep_kernel_ms_36_sources"] = sweep

line = json.dumps(rec)
print(line, flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
