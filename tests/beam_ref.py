"""Test oracles for lightpycl_amd.beam: the half-power answer from a sort and a
cumulative sum, and a numpy stand-in for the three device passes.  Not test
cases themselves; tests/test_beam_host.py checks half_power_sorted against an
independent plain-Python restatement."""
import numpy as np
import pytest

from lightpycl_amd.beam import KEY_BITS, HalfPower, NonMonotonePower, Summary, key_of


# Tolerances of the float64 beam outputs (derivation: tests/test_gpu_beam.py's docstring)
ULP_PI = float(np.spacing(np.pi))
ELEV_MEASURED = 4.44e-16                       # max |elev_out - host elevation|, traced cases
ELEV_TOL = max(8 * ELEV_MEASURED, 4 * ULP_PI)
SUM_RTOL = 1e-12                               # float64 sums in atomic order (as test_gpu_postproc.py)


@pytest.fixture()
def no_pdf(monkeypatch, tmp_path):
    """plot_elevation_histogram draws and saves a PDF: keep the drawing, skip the file.
    (Test modules import this fixture by name.)"""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(plt, "savefig", lambda *a, **k: None)
    yield
    plt.close("all")


def half_power_sorted(elevation, power):
    """The same answer from a sort and a cumulative sum over the groups of equal
    elevation (host arrays; the definition the tests check the descent against)."""
    e = np.asarray(elevation, np.float64).reshape(-1)
    p = np.asarray(power, np.float64).reshape(-1)
    ok = np.isfinite(e)
    e, p = e[ok], p[ok]
    if e.size == 0:
        raise ValueError("half_power: no measured ray with a finite elevation")
    if np.any(~(p >= 0.0)):
        raise NonMonotonePower("negative or NaN power")
    order = np.argsort(e, kind="stable")
    e, p = e[order], p[order]
    ue, start = np.unique(e, return_index=True)
    cum = np.cumsum(p)
    total = float(cum[-1])
    cg = cum[np.append(start[1:], e.size) - 1]          # C at the end of each group
    half = total / 2.0
    hit = np.flatnonzero(cg >= half)
    j = int(hit[0]) if hit.size else ue.size - 1
    if j > 0 and abs(cg[j - 1] - half) <= abs(cg[j] - half):
        j -= 1
    return HalfPower(total, float(ue[j]), float(cg[j]), int(key_of(ue[j])), 0)


class NumpyPasses:
    """The three passes over host arrays of elevations and powers: what the
    device passes compute, in numpy.  ``perturb`` (a ``numpy.random.Generator``)
    moves every float64 sum of a pass by -1, 0 or +1 ulp, as a different atomic
    order could."""

    def __init__(self, elevation, power, perturb=None):
        self.e = np.asarray(elevation, np.float64).reshape(-1)
        self.p = np.asarray(power, np.float32).reshape(-1)
        self.ok = np.isfinite(self.e)
        self.key = np.where(self.ok, self.e, 0.0).view(np.uint64)
        self.perturb = perturb

    def _jitter(self, x):
        if self.perturb is None:
            return x
        x = np.asarray(x, np.float64)
        d = self.perturb.integers(-1, 2, x.shape)
        return np.where(d > 0, np.nextafter(x, np.inf), np.where(d < 0, np.nextafter(x, -np.inf), x))

    def scan(self):
        e, p = self.e[self.ok], self.p[self.ok].astype(np.float64)
        return Summary(int(e.size), int((~self.ok).sum()), int((~(p >= 0.0)).sum()),
                       float(e.min()) if e.size else float("nan"), float(e.max()) if e.size else float("nan"),
                       float(self._jitter(p.sum())))

    def digit_pass(self, prefix, shift, bits):
        nb = 1 << bits
        sel = self.ok.copy()
        if shift + bits < KEY_BITS:
            sel &= (self.key >> np.uint64(shift + bits)) == np.uint64(prefix)
        k = self.key[sel]
        d = ((k >> np.uint64(shift)) & np.uint64(nb - 1)).astype(np.int64)
        bin_pow = np.bincount(d, weights=self.p[sel].astype(np.float64), minlength=nb)
        bin_cnt = np.bincount(d, minlength=nb).astype(np.int64)
        bin_max = np.zeros(nb, np.uint64)
        np.maximum.at(bin_max, d, k)
        return self._jitter(bin_pow), bin_cnt, bin_max

    def power_below(self, thr, inclusive):
        sel = self.ok & ((self.e <= thr) if inclusive else (self.e < thr))
        n = int(sel.sum())
        return (float(self._jitter(self.p[sel].astype(np.float64).sum())), n,
                float(self.e[sel].max()) if n else float("nan"))
