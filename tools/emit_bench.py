"""GPU box: making a light source and tracing it, host generation against device
emission.

Lens scene, ``keep_results=False``, the default cosine source of ``rays`` rays:
  * host: ``light_source(ray_count=n)`` (float64 numpy), then the trace, which stages
    the host arrays (``lpc_trace_stage_rays``) -- the only path before device sources;
  * device: ``light_source(ray_count=n, on_device=True)``, then the trace from the
    device source (``lpc_trace_set_rays_dev``);
and the parts alone: the generator filling 2 n doubles (its copy to the host
included), a skip of 4 M words (no stores, no copy: the recurrence alone), the whole
hemisphere emission, the emission of an empty shard (generator + weight sum), and
the transform as their difference.  Every call is synchronous (it ends with a
stream wait), so each is timed by the wall clock: once cold, then the median of
``REPS`` further calls.  Prints one JSON line.

    python tools/emit_bench.py [rays] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lightpycl_amd import light_source as lsrc  # noqa: E402
from lightpycl_amd import scenes  # noqa: E402
from lightpycl_amd.iterative_tracer import CL_Tracer  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if args else 1_000_000
out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
REPS = 5

sc = scenes.lens(n=10, seed=7)
tr = CL_Tracer(device=0)
eng = lsrc.default_engine(0)


def timed(fn):
    ts = []
    for _ in range(REPS + 1):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return dict(cold_ms=round(ts[0], 3), median_ms=round(statistics.median(ts[1:]), 3))


def source(on_device):
    np.random.seed(7)
    return lsrc.light_source(power=1000., ray_count=n, on_device=on_device)


def trace(src):
    tr.iterative_tracer([src], sc.meshes, trace_iterations=sc.iterations, trace_until_dissipated=sc.tau,
                        max_ray_len=sc.max_ray_len, ior_env=sc.ior_env, keep_results=False)
    return list(tr.iteration_counts)


counts = {}


def end_to_end(on_device):
    counts[on_device] = trace(source(on_device))


key, pos = np.random.RandomState(7).get_state()[1:3]
ident = np.eye(3)
c4 = np.zeros(4, np.float32)
rec = dict(tool="emit_bench", scene="lens", rays=n, reps=REPS, results={})
R = rec["results"]
R["host_generate"] = timed(lambda: source(False))
R["device_emit"] = timed(lambda: source(True))
R["host_generate_and_trace"] = timed(lambda: end_to_end(False))
R["device_emit_and_trace"] = timed(lambda: end_to_end(True))
R["generator_fill_2n_doubles_with_host_copy"] = timed(lambda: eng.rng_mt19937(key, pos, 2 * n))
R["generator_skip_4m_words"] = timed(lambda: eng.rng_mt19937(key, pos, 2_000_000, skip=True))
R["emit_hemisphere"] = timed(lambda: eng.emit_hemisphere(key, pos, n, c4, ident, ident))
R["emit_empty_shard"] = timed(lambda: eng.emit_hemisphere(key, pos, n, c4, ident, ident, first=0, count=0))
R["transform_by_difference_ms"] = round(R["emit_hemisphere"]["median_ms"] - R["emit_empty_shard"]["median_ms"], 3)
R["speedup_generate"] = round(R["host_generate"]["median_ms"] / R["device_emit"]["median_ms"], 2)
R["speedup_generate_and_trace"] = round(R["host_generate_and_trace"]["median_ms"] /
                                        R["device_emit_and_trace"]["median_ms"], 2)
rec["iteration_counts"] = dict(host=counts[False], device=counts[True])
line = json.dumps(rec)
print(line, flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(line + "\n")
