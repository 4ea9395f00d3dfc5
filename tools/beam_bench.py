"""GPU box: the beam analyses after an aggregate-mode trace, host path against
device path on the same trace.

Lens scene, ``keep_results=False``; then ``get_beam_width_half_power``,
``get_beam_HWHM`` (500 bins) and the 90-bin elevation histogram
(``plot_elevation_histogram`` with the PDF left out: drawing and saving cost the
same on both paths), each timed once cold and as the median of 5 further calls,
with ``on_device=False`` (fetch the measured record, numpy on one core) and
``on_device=True`` (passes over the device-resident record); last, the histogram's
GPU passes alone (``Engine.elev_hist``).  Prints one JSON line.

    python tools/beam_bench.py [rays] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import matplotlib  # noqa: E402

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402

from lightpycl_amd import scenes  # noqa: E402
from lightpycl_amd.engine import Engine  # noqa: E402
from lightpycl_amd.iterative_tracer import CL_Tracer  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 1_000_000
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
REPS = 5

plt.savefig = lambda *a, **k: None

# bytes that cross to the host: the arrays the engine's fetch / pass calls return
fetched = [0]


def _count(x):
    if isinstance(x, np.ndarray):
        fetched[0] += x.nbytes
    elif isinstance(x, (tuple, list)):
        for y in x:
            _count(y)
    elif isinstance(x, (int, float)):
        fetched[0] += 8


def _wrap(name):
    fn = getattr(Engine, name)

    def counted(self, *a, **k):
        r = fn(self, *a, **k)
        _count(r)
        return r
    setattr(Engine, name, counted)


for name in ("fetch_measured", "elev_scan", "elev_hist", "elev_digit_pass", "elev_power_below"):
    _wrap(name)

sc = scenes.lens(n=n, seed=7)
tr = CL_Tracer(device=0)
t = time.perf_counter()
tr.iterative_tracer(sc.sources, sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                    max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=False)
trace_ms = (time.perf_counter() - t) * 1e3
measured = int(tr.engine.measured()[0])

CALLS = dict(half_power=lambda dev: tr.get_beam_width_half_power(on_device=dev),
             hwhm=lambda dev: tr.get_beam_HWHM(points=500, on_device=dev),
             hist90=lambda dev: tr.plot_elevation_histogram(points=90, on_device=dev))
rec = dict(tool="beam_bench", scene="lens", rays=n, measured_rays=measured, first_trace_ms=round(trace_ms, 3),
           reps=REPS, results={})
for name, call in CALLS.items():
    row = {}
    for dev in (False, True):
        times, val = [], None
        for k in range(REPS + 1):
            fetched[0] = 0
            t = time.perf_counter()
            val = call(dev)
            times.append((time.perf_counter() - t) * 1e3)
            plt.close("all")
        row["device" if dev else "host"] = dict(cold_ms=round(times[0], 3),
                                                median_ms=round(statistics.median(times[1:]), 3),
                                                bytes_fetched=fetched[0])
        if name != "hist90":
            row.setdefault("angle_deg", []).append(float(np.asarray(val[1]).reshape(-1)[0]))
    row["speedup_median"] = round(row["host"]["median_ms"] / row["device"]["median_ms"], 2)
    rec["results"][name] = row
# the histogram's GPU passes alone (scan for the range + binning), without numpy's and matplotlib's part
times = []
for k in range(REPS + 1):
    fetched[0] = 0
    t = time.perf_counter()
    tr.engine.elev_hist(90, [0, 0, 1, 0])
    times.append((time.perf_counter() - t) * 1e3)
rec["results"]["hist90_passes_only"] = dict(device=dict(cold_ms=round(times[0], 3),
                                                        median_ms=round(statistics.median(times[1:]), 3),
                                                        bytes_fetched=fetched[0]))
line = json.dumps(rec)
print(line, flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
