"""The power budget formed on the host -- TEST INFRASTRUCTURE.

``cutoff_ref.trace_rays`` (the reference's host loop, with ``cut = 0``
``oracle.trace_rays`` operation for operation) run with a ``bounce_fn`` wrapper
around ``oracle.bounce`` (the CPU oracle) or the reference's own kernels
(``tests/ref_gpu.py``).  From each bounce's per-ray outputs -- the power before
and after (``pow``), ``n1``, ``isect_mid``, ``r_pow`` / ``r_meas``, ``t_pow`` /
``t_meas`` -- the wrapper forms the ledger's float64 terms by the operations
include/lpc.h fixes, in that order:

    dissipated  float64(p_in) - float64(p)           mesh n1, the dissipation branch taken
    escaped     float64(p)                           no hit
    terminated  float64(p)                           hit mesh of material type 2
    measured    float64(p)                           hit mesh of material type 3
    absorbed    (float64(p) - float64(kr)) - float64(kt)   every other hit
    kept        float64(kr) + float64(kt)            every ray

with kr = r_pow where r_meas == 0 else 0, kt likewise, before any cutoff.  The
terms are kept per iteration, category and mesh, so a ledger summed in any order
can be compared by the rule of ``cutoff_ref.assert_ledger``: counts equal, each
float64 sum within (n - 1) 2^-53 sum|terms| of ``math.fsum(terms)``.
"""
from __future__ import annotations

import math

import numpy as np

import cutoff_ref

MESH_CATS = ("dissipated", "absorbed", "terminated", "measured")        # the per-mesh table's columns
SUMS = ("power_in", "dissipated", "escaped", "terminated", "measured", "absorbed", "kept")
COUNTS = dict(n_in="power_in", n_dissipated="dissipated", n_escaped="escaped", n_terminated="terminated",
              n_measured="measured", n_absorbed="absorbed")
U = 2.0 ** -53


def bounce_terms(scene, p_in, out):
    """One iteration's terms -> {category: (float64 terms, int32 meshes)} (the
    scene-wide categories carry mesh -1)."""
    f64 = np.float64
    p_in = np.asarray(p_in, np.float32).reshape(-1)
    p = np.asarray(out["pow"], np.float32).reshape(-1)
    n1 = np.asarray(out["n1"], np.int32).reshape(-1)
    hit = np.asarray(out["isect_mid"], np.int32).reshape(-1)
    kr = np.where(np.asarray(out["r_meas"]).reshape(-1) == 0, np.asarray(out["r_pow"], np.float32).reshape(-1),
                  np.float32(0.0)).astype(np.float32)
    kt = np.where(np.asarray(out["t_meas"]).reshape(-1) == 0, np.asarray(out["t_pow"], np.float32).reshape(-1),
                  np.float32(0.0)).astype(np.float32)
    K = scene.mesh_count
    n1c = np.clip(n1, 0, K - 1)
    dis = (n1 >= 0) & (scene.mat_type[n1c] == 0) & (scene.diss[n1c] > np.float32(0.000001))
    mt = np.where(hit >= 0, scene.mat_type[np.clip(hit, 0, K - 1)], -1)
    esc = hit < 0
    term = (hit >= 0) & (mt == 2)
    meas = (hit >= 0) & (mt == 3)
    absd = (hit >= 0) & ~term & ~meas
    none = np.zeros(len(p), np.int32) - 1
    with np.errstate(invalid="ignore"):
        return dict(power_in=(p_in.astype(f64), none),
                    dissipated=((p_in.astype(f64) - p.astype(f64))[dis], n1[dis]),
                    escaped=(p.astype(f64)[esc], none[esc]),
                    terminated=(p.astype(f64)[term], hit[term]),
                    measured=(p.astype(f64)[meas], hit[meas]),
                    absorbed=(((p.astype(f64) - kr.astype(f64)) - kt.astype(f64))[absd], hit[absd]),
                    kept=(kr.astype(f64) + kt.astype(f64), none))


def trace(oracle_mod, meshes, origin, dirs, power, iterations, tau, max_ray_len, ior_env, cut=0.0, bounce_fn=None,
          keep_results=False):
    """-> dict(iters: [bounce_terms per iteration], culled: the culled float32
    powers per iteration, counts, mesh_power (the loop's own float64 per-mesh
    measured power), K, results)."""
    inner = oracle_mod.bounce if bounce_fn is None else bounce_fn
    iters = []

    def wrapped(scene, o, d, pw, ms, mid, mrl, ior):
        p_in = np.array(pw, dtype=np.float32).reshape(-1)          # the power as this iteration reads it
        out = inner(scene, o, d, pw, ms, mid, mrl, ior)
        iters.append(bounce_terms(scene, p_in, out))
        return out

    res, info = cutoff_ref.trace_rays(oracle_mod, origin, dirs, power, meshes, iterations, tau, max_ray_len, ior_env,
                                      cut=cut, keep_results=keep_results, bounce_fn=wrapped)
    return dict(iters=iters, culled=info["culled"], counts=list(info["counts"]),
                mesh_power=np.asarray(info["mesh_power"]), K=len(meshes), results=res)


def totals(ref):
    """Category counts over all iterations."""
    return {c: sum(len(it[c][0]) for it in ref["iters"]) for c in SUMS}


def mesh_terms(ref, cat, mesh):
    """Every term of a per-mesh category booked to `mesh`, over the trace."""
    parts = [it[cat][0][it[cat][1] == mesh] for it in ref["iters"]]
    return np.concatenate(parts) if parts else np.zeros(0)


def sum_tol(terms):
    return max(len(terms) - 1, 0) * U * math.fsum(abs(float(v)) for v in terms)


def assert_sum(got, terms, what):
    want = math.fsum(float(v) for v in terms)
    tol = sum_tol(terms)
    assert abs(float(got) - want) <= tol, (what, float(got), want, tol)


def residues(ref):
    """The identities on the helper's own terms, exactly summed: per iteration
    (power_in minus the six categories) and between iterations (kept_i -
    culled_i - power_in_{i+1}), each with its n 2^-52 sum|terms| bound.
    -> [(residue, bound)] per iteration, [(residue, bound)] per iteration pair."""
    per, between = [], []
    for i, it in enumerate(ref["iters"]):
        terms = [float(v) for v in it["power_in"][0]]
        for c in SUMS[1:]:
            terms += [-float(v) for v in it[c][0]]
        per.append((math.fsum(terms), len(terms) * 2.0 ** -52 * math.fsum(abs(v) for v in terms)))
        if i + 1 < len(ref["iters"]):
            t2 = ([float(v) for v in it["kept"][0]] + [-float(v) for v in ref["culled"][i]] +
                  [-float(v) for v in ref["iters"][i + 1]["power_in"][0]])
            between.append((math.fsum(t2), len(t2) * 2.0 ** -52 * math.fsum(abs(v) for v in t2)))
    return per, between


def assert_budget(b, ref, what=""):
    """A library ledger (``Engine.budget()``'s dict, or the tracer's: per-iteration
    arrays; ``mesh_power`` / ``mesh_count`` (K, 4), or ``mesh`` / ``mesh_count``
    dicts by category) against the helper's terms."""
    n = len(ref["iters"])
    assert len(b["n_in"]) == n, (what, len(b["n_in"]), n)
    for i, it in enumerate(ref["iters"]):
        for cn, cat in COUNTS.items():
            assert int(b[cn][i]) == len(it[cat][0]), (what, i, cn, int(b[cn][i]), len(it[cat][0]))
        for cat in SUMS:
            assert_sum(b[cat][i], it[cat][0], (what, i, cat))
    assert [int(v) for v in b["n_in"]] == ref["counts"], (what, "populations")
    for j, cat in enumerate(MESH_CATS):
        if "mesh" in b:
            mp, mc = b["mesh"][cat], b["mesh_count"][cat]
        else:
            mp, mc = b["mesh_power"][:, j], b["mesh_count"][:, j]
        assert len(mp) == ref["K"] and len(mc) == ref["K"], (what, cat)
        for m in range(ref["K"]):
            t = mesh_terms(ref, cat, m)
            assert int(mc[m]) == len(t), (what, cat, m, int(mc[m]), len(t))
            assert_sum(mp[m], t, (what, cat, m))


def closure_tol(ref):
    """Bound of the tracer's ``closure``.  It combines, by an exact sum rounded
    once, power_in[0], every iteration's five spent sums, the culled sums and
    ``left`` (= kept - culled of the last iteration, one rounding).  Each ledger
    sum is within its (n - 1) 2^-53 sum|terms| of the exact sum of its terms; the
    exact sums satisfy the identities up to the helper's own residues; the final
    roundings add at most 2^-52 of the magnitudes combined."""
    tol = 0.0
    mag = 0.0
    per, between = residues(ref)
    for i, it in enumerate(ref["iters"]):
        for cat in SUMS:
            tol += sum_tol(it[cat][0])
            mag += math.fsum(abs(float(v)) for v in it[cat][0])
        c = [float(v) for v in ref["culled"][i]]
        tol += sum_tol(c)
        mag += math.fsum(abs(v) for v in c)
    tol += sum(abs(r) for r, _ in per) + sum(abs(r) for r, _ in between)
    return tol + 2.0 ** -52 * mag
