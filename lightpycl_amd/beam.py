"""Beam-width selection over elevation passes.

``get_beam_width_half_power`` (reference ``iterative_tracer.py:443-466``) sorts
every measured ray by elevation, forms the cumulative power and reports the ray
whose cumulative power is closest to half of the total.  :func:`half_power`
finds the same ray without a sort and without the rays: a radix descent over
the 64-bit key of an elevation (the bit pattern of the float64, monotone since
an elevation is never negative), each step one *pass* over the rays that returns
a few thousand per-bin sums.  The passes are callables, so the same driver runs
over the device-resident record (``Engine.elev_digit_pass``), over a numpy
stand-in (``tests/beam_ref.py``, the CPU tests) and, later, over passes that
all-reduce their small outputs between ranks.

Callables
---------
``scan()``
    object with ``n_valid, n_invalid, n_negative, e_min, e_max, total_power``.
``digit_pass(prefix, shift, bits)``
    ``(bin_pow float64[1 << bits], bin_cnt int64[...], bin_maxkey uint64[...])``
    over the valid rays with ``key >> (shift + bits) == prefix`` (all of them when
    ``shift + bits == 64``), binned by ``(key >> shift) & ((1 << bits) - 1)``.
``power_below(thr, inclusive)``
    ``(power, count, e_max)`` of the valid rays with ``e < thr`` (``<=`` when
    inclusive).

Groups of equal elevation
-------------------------
Rays of equal elevation form one group: ``C(e)`` is the power of all rays with
elevation ``<= e``.  The answer is the reference's whenever the elevation of the
crossing ray is unique.  Within a tied group the reference's cumulative sum also
takes values *inside* the group (its stable sort orders the group by ray index)
and may report one of them; the elevation it reports is the group's all the
same, only the cumulative percentage can differ.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

KEY_BITS = 64
MAX_PASS_BITS = 12

Summary = namedtuple("Summary", "n_valid n_invalid n_negative e_min e_max total_power")
HalfPower = namedtuple("HalfPower", "total elevation cum_power key passes")


class NonMonotonePower(ValueError):
    """Some measured ray has a negative (or NaN) power: the cumulative power is not
    monotone in the elevation and the descent's selection is undefined.  The caller
    takes the host path (sort and cumsum) instead."""


def key_of(e):
    """uint64 key(s) of elevation(s) e >= 0."""
    return np.asarray(e, np.float64).view(np.uint64)


def elev_of(key):
    return float(np.array([key], np.uint64).view(np.float64)[0])


def half_power(scan, digit_pass, power_below=None, bits=11):
    """The distinct elevation whose cumulative power ``C(e)`` is closest to half of
    the total, and that ``C(e)``: with ``e1`` the smallest distinct elevation whose
    ``C(e1) >= total / 2`` and ``e0`` the distinct elevation before it, whichever of
    ``(e0, C(e0))``, ``(e1, C(e1))`` is closer to half, the lower one on a tie.

    The descent takes ceil(64 / bits) passes.  Per pass it looks for the first
    non-empty bin at which the running sum reaches half.  The float64 sums of two
    passes over the same rays need not agree in their last bits (atomic order is
    not fixed), so a refinement may find that no bin of the chosen range reaches
    half: it then takes the range's last non-empty bin.  The counts are exact, so
    the descent always ends on the key of an existing ray; after such a step the
    two candidates' cumulative powers are re-read with ``power_below`` (one pass
    each) so that the values compared come from whole passes.
    """
    if not 1 <= bits <= MAX_PASS_BITS:
        raise ValueError("half_power: 1 <= bits <= %d" % MAX_PASS_BITS)
    s = scan()
    if s.n_negative > 0:
        raise NonMonotonePower("%d measured rays have a negative or NaN power" % s.n_negative)
    if s.n_valid <= 0:
        raise ValueError("half_power: no measured ray with a finite elevation")
    total = float(s.total_power)
    half = total / 2.0
    prefix, top, passes = 0, KEY_BITS, 0
    below, c1 = 0.0, 0.0             # C just under the current range; C at the end of the chosen bin
    prev_key = None                  # largest key under the chosen bin
    forced = False
    while top > 0:
        b = min(bits, top)
        shift = top - b
        bin_pow, bin_cnt, bin_maxkey = digit_pass(prefix, shift, b)
        passes += 1
        ne = np.flatnonzero(np.asarray(bin_cnt) > 0)
        if ne.size == 0:
            raise RuntimeError("half_power: a pass found no ray under a prefix that the pass before counted")
        cum = below + np.cumsum(np.asarray(bin_pow, np.float64)[ne])
        hit = np.flatnonzero(cum >= half)
        if hit.size:
            j = int(hit[0])
        else:
            j, forced = ne.size - 1, True
        if j > 0:
            prev_key = int(np.asarray(bin_maxkey)[ne[j - 1]])
            below = float(cum[j - 1])
        c1 = float(cum[j])
        prefix = (prefix << b) | int(ne[j])
        top = shift
    e1 = elev_of(prefix)
    e0 = elev_of(prev_key) if prev_key is not None else None
    c0 = below
    if forced and power_below is not None:
        c0, n0, e0 = power_below(e1, 0)
        c0, e0 = float(c0), (float(e0) if n0 > 0 else None)
        c1 = float(power_below(e1, 1)[0])
        passes += 2
    if e0 is not None and abs(c0 - half) <= abs(c1 - half):
        return HalfPower(total, e0, c0, int(key_of(e0)), passes)
    return HalfPower(total, e1, c1, prefix, passes)
