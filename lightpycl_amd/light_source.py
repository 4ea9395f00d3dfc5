"""Ray sources -- drop-in for LightPyCL's ``light_source`` module.

Mirrors ``/root/reference/light_source.py`` (class ``light_source``, :28-204):
same constructor signature, same attributes (``rays_origin`` (N,4) f32,
``rays_dir`` (N,4) f32, ``rays_power``), and the same numpy RNG draw sequence,
so ``np.random.seed(s)`` before construction yields the same rays as the
reference.  The default path is host-side float64 numpy (91 ms per million rays
on an MI355X host, 140 times their trace: DESIGN.md section 10).
``light_source(..., on_device=True)`` emits the same rays on the GPU instead:
numpy's random stream continued there bit for bit, the float64 transform to
within the final float32 rounding, and ``np.random``'s state left exactly where
the host path leaves it.
"""
from __future__ import annotations

import numpy as np
import numpy.linalg as la


def _rot(axis):
    """4x4 homogeneous rotation builders with a zero [3][3] entry, as every
    reference module defines them (light_source.py:64-66, 115-117, ...)."""
    if axis in ("x", "X"):
        return lambda a: np.matrix([[1, 0, 0, 0], [0, np.cos(a), -np.sin(a), 0],
                                    [0, np.sin(a), np.cos(a), 0], [0, 0, 0, 0]])
    if axis in ("y", "Y"):
        return lambda a: np.matrix([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0],
                                    [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 0]])
    if axis in ("z", "Z"):
        return lambda a: np.matrix([[np.cos(a), -np.sin(a), 0, 0], [np.sin(a), np.cos(a), 0, 0],
                                    [0, 0, 1, 0], [0, 0, 0, 0]])
    return _rot("x")


_Rx, _Rz = _rot("x"), _rot("z")


def _pointing(direction, use_arctan2_always):
    """Elevation/azimuth of the beam axis (light_source.py:106-113 and :146-147)."""
    elev = np.arccos(direction[2] / la.norm(direction))
    if use_arctan2_always:
        return elev, np.arctan2(direction[1], direction[0])
    if direction[0] == 0:
        az = np.pi / 2.0 if direction[1] >= 0 else -np.pi / 2.0
    else:
        az = np.arctan2(direction[1], direction[0])
    return elev, az


def cos_power(m):
    """The directivity ``cos(elevation) ** m`` (m >= 0; 1 is the reference's default
    lambda, 0 isotropic): a host directivity like any other callable, and the
    family ``light_source(..., on_device=True)`` evaluates on the GPU."""
    if not float(m) >= 0.0:
        raise ValueError("cos_power: m >= 0")

    def directivity(azimuth, elevation):
        return np.cos(elevation) ** m
    directivity.cos_power = m
    return directivity


_ENGINES = {}


def default_engine(device=None):
    """The process-wide engine device sources of GPU ``device`` are emitted on
    (None: ``$LPC_DEVICE``, ``$LOCAL_RANK`` or 0).  Raises without a GPU."""
    from .engine import Engine, default_device
    d = default_device() if device is None else int(device)
    e = _ENGINES.get(d)
    if e is None or e.h is None:
        e = _ENGINES[d] = Engine(d)
    return e


def _ray_attr(name):
    """rays_origin / rays_dir / rays_power: plain instance attributes of a host
    source; fetched from the GPU on access while the source lives there, and an
    assignment brings the whole source to the host first."""
    def get(self):
        if self.__dict__.get("_dev") is not None:
            return self._fetch(name)
        return self.__dict__.get(name)

    def put(self, value):
        if self.__dict__.get("_dev") is not None:
            self._to_host()
        self.__dict__[name] = value
    return property(get, put)


class light_source:
    """A point (or collimated-disc) source of ``ray_count`` rays.

    Constructing one draws random hemisphere rays immediately, exactly like the
    reference constructor (light_source.py:37-43).

    ``on_device=True`` makes the rays on GPU ``device`` from ``np.random``'s current
    state and leaves that state advanced as the host path would, so any later
    draw, host or device, continues the reference's sequence.  ``directivity`` must
    then be the default or a :func:`cos_power`.  ``random_collimated_rays`` and
    ``rotate_rays`` act on the device source; ``rays_origin``, ``rays_dir`` and
    ``rays_power`` fetch a host copy on every access (changing that copy in place
    does not reach the GPU); assigning to one of them, or ``grid_rays``, turns the
    source into an ordinary host source.  ``shard=(first, count)`` keeps only rays
    [first, first + count) of the ``ray_count``-ray source (a rank of a sharded
    trace, ``distributed.emit_shard``); the stream still advances over all draws
    and the powers are normalised over all rays."""

    center = None
    direction = None
    directivity = None
    power = 1
    ray_count = None
    rays_origin = _ray_attr("rays_origin")
    rays_dir = _ray_attr("rays_dir")
    rays_power = _ray_attr("rays_power")

    def __init__(self, center=np.array([0, 0, 0, 0], dtype=np.float32), direction=(0, 0, 1),
                 directivity=lambda x, y: np.cos(y), power=1, ray_count=500, on_device=False, device=None,
                 shard=None):
        self.center = center
        self.direction = direction
        self.directivity = directivity
        self.power = power
        self.ray_count = ray_count
        if on_device:
            self._device_init(device, shard)
        self.random_rays()

    # -- the source on the GPU ---------------------------------------------
    def _device_init(self, device, shard):
        if self.directivity is _DEFAULT_DIRECTIVITY:
            m = 1.0
        elif hasattr(self.directivity, "cos_power"):
            m = float(self.directivity.cos_power)
        else:
            raise TypeError("light_source(on_device=True) evaluates the directivity on the GPU: pass "
                            "lightpycl_amd.light_source.cos_power(m) (or leave the default), not an arbitrary "
                            "callable")
        n = int(self.ray_count)
        first, count = (0, n) if shard is None else (int(shard[0]), int(shard[1]))
        if n < 1 or first < 0 or count < 0 or first + count > n:
            raise ValueError("light_source(on_device=True): shard (first=%d, count=%d) outside [0, %d]"
                             % (first, count, n))
        c4 = np.asarray(self.center, dtype=np.float32).reshape(-1)
        if c4.size != 4:
            raise ValueError("light_source(on_device=True): center must have 4 components")
        self._dev_engine = default_engine(device)       # raises without a GPU, before any draw
        self._dev_m, self._dev_shard, self._dev_center = m, (first, count), c4

    def _emit(self, call, pow_shape):
        """Emit from np.random's state, then leave it advanced."""
        st = np.random.get_state()
        if st[0] != "MT19937":
            raise RuntimeError("np.random's legacy generator is not MT19937")
        old = self.__dict__.get("_dev")
        rays, key, pos = call(st[1], st[2])
        np.random.set_state((st[0], key, pos) + tuple(st[3:]))
        if old is not None:
            old.free()
        self._dev, self._dev_pow_shape = rays, pow_shape
        self.rays_dest = np.zeros((rays.n, 4)).astype(np.float32)

    def _fetch(self, name):
        o, d, p = self._dev.fetch(origin=name == "rays_origin", dirs=name == "rays_dir", power=name == "rays_power")
        return p.reshape(self._dev_pow_shape) if name == "rays_power" else o if name == "rays_origin" else d

    def _to_host(self):
        o, d, p = self._dev.fetch()
        self._dev.free()
        self._dev = self._dev_engine = None
        self.__dict__.update(rays_origin=o, rays_dir=d, rays_power=p.reshape(self._dev_pow_shape))

    # -- light_source.py:98-137 -------------------------------------------
    def random_rays(self):
        """Random directions over the +z hemisphere (u -> elevation = arccos(u),
        v -> azimuth = 2 pi v), power weighted by ``directivity`` and normalised to
        ``power``, then rotated onto ``direction``."""
        if self.__dict__.get("_dev_engine") is not None:
            eng, n = self._dev_engine, int(self.ray_count)
            elev0, az0 = _pointing(self.direction, use_arctan2_always=False)
            first, count = self._dev_shard
            return self._emit(lambda key, pos: eng.emit_hemisphere(
                key, pos, n, self._dev_center, _Rx(elev0), _Rz(az0), power=self.power, m=self._dev_m,
                first=first, count=count), (count, 1))
        n = self.ray_count
        self.rays_origin = np.zeros((n, 4)).astype(np.float32) + self.center
        self.rays_dest = np.zeros((n, 4)).astype(np.float32)
        elev0, az0 = _pointing(self.direction, use_arctan2_always=False)
        u = np.random.rand(n, 1)
        v = np.random.rand(n, 1)
        pad = np.zeros((n, 1))
        elevation = np.arccos(u)
        azimuth = 2.0 * np.pi * v
        xs = np.sin(elevation) * np.cos(azimuth)
        ys = np.sin(elevation) * np.sin(azimuth)
        zs = np.cos(elevation)
        dirs = np.concatenate((xs, ys, zs, pad), axis=1)
        pw = np.float32(self.directivity(azimuth, elevation))
        self.rays_power = pw * self.power / np.sum(pw)
        dirs = np.dot(dirs, _Rx(elev0))
        self.rays_dir = np.dot(dirs, _Rz(az0)).astype(np.float32)

    # -- light_source.py:45-95 --------------------------------------------
    def grid_rays(self):
        """Regular elevation x azimuth grid of floor(sqrt(N))**2 rays.  (The
        reference's ``np.float`` / float ``linspace`` count no longer run under
        numpy 2; this keeps its arithmetic with integer counts.)"""
        if self.__dict__.get("_dev") is not None:
            self._to_host()                     # no device grid: an ordinary host source from here on
        self.rays_origin = np.zeros((self.ray_count, 4)).astype(np.float32) + self.center
        self.rays_dest = np.zeros((self.ray_count, 4)).astype(np.float32)
        side = int(np.floor(np.sqrt(self.ray_count)))
        self.ray_count = np.floor(np.sqrt(self.ray_count)) ** 2
        elev0 = np.arccos(self.direction[2] / la.norm(self.direction))
        if self.direction[0] == 0:
            az0 = np.pi / 2.0 if self.direction[1] >= 0 else -np.pi / 2.0
        else:
            az0 = np.arctan(self.direction[1] / self.direction[0])
        el_col = np.transpose(np.matrix(np.linspace(0.0, np.pi / 2.0, side)))
        az_col = np.transpose(np.matrix(np.linspace(0.0, 2.0 * np.pi, side)))
        elevation = azimuth = None
        for k in range(side):
            if k == 0:
                elevation, azimuth = el_col, az_col
            else:
                elevation = np.concatenate((elevation, el_col), axis=0)
                azimuth = np.concatenate((azimuth, 0.0 * az_col + float(az_col[k])), axis=0)
        sa, ca = np.sin(azimuth), np.cos(azimuth)
        se, ce = np.sin(elevation), np.cos(elevation)
        self.rays_power = np.array(self.directivity(azimuth, elevation), dtype=np.float32) * self.power
        cnt = int(self.ray_count)
        dirs = np.array(np.append(np.append(np.append(np.multiply(se, ca), np.multiply(se, sa), axis=1),
                                            ce, axis=1), np.zeros((cnt, 1)), axis=1), dtype=np.float32)
        dirs = np.dot(dirs, _Rx(elev0))
        self.rays_dir = np.dot(dirs, _Rz(az0))

    # -- light_source.py:139-170 ------------------------------------------
    def random_collimated_rays(self, diameter=1.0):
        """Parallel rays (+z before rotation) with origins uniform in a
        ``diameter`` square, equal power.  Draws x then y after the
        constructor's own draws, as the reference does."""
        if self.__dict__.get("_dev_engine") is not None:
            eng, n = self._dev_engine, int(self.ray_count)
            elev0, az0 = _pointing(self.direction, use_arctan2_always=True)
            row = np.zeros((1, 4)).astype(np.float32)
            row[:, 2] = 1.0
            row = np.dot(row, _Rx(elev0))
            row = np.array(np.dot(row, _Rz(az0))).astype(np.float32)
            first, count = self._dev_shard
            return self._emit(lambda key, pos: eng.emit_collimated(
                key, pos, n, diameter, self._dev_center, _Rx(elev0), _Rz(az0), row, power=self.power,
                first=first, count=count), (count,))
        n = self.ray_count
        self.rays_dest = np.zeros((n, 4)).astype(np.float32)
        elev0, az0 = _pointing(self.direction, use_arctan2_always=True)
        x = (np.random.rand(n, 1) - 0.5) * diameter
        y = (np.random.rand(n, 1) - 0.5) * diameter
        z = np.zeros((n, 1))
        pad = np.zeros((n, 1))
        org = np.concatenate((x, y, z, pad), axis=1)
        dirs = np.zeros((n, 4)).astype(np.float32)
        dirs[:, 2] = 1.0
        pw = np.ones(n).astype(np.float32)
        self.rays_power = pw * self.power / np.sum(pw)
        org = np.dot(org, _Rx(elev0))
        self.rays_origin = np.array(np.dot(org, _Rz(az0)).astype(np.float32) + self.center).astype(np.float32)
        dirs = np.dot(dirs, _Rx(elev0))
        self.rays_dir = np.array(np.dot(dirs, _Rz(az0))).astype(np.float32)

    # -- light_source.py:173-188 ------------------------------------------
    def rotate_rays(self, axis="z", pivot=[0, 0, 0, 0], ang=np.pi / 2.0):
        R = _rot(axis)
        piv = np.array(pivot)
        if self.__dict__.get("_dev") is not None:
            return self._dev.rotate(R(ang), piv)
        self.rays_origin = np.array(np.add(np.dot(np.subtract(self.rays_origin, piv), R(ang)), piv)).astype(np.float32)
        self.rays_dir = np.array(np.dot(self.rays_dir, R(ang))).astype(np.float32)

    # -- light_source.py:191-204 ------------------------------------------
    def save_dxf(self, dxf_file):
        """DXF export needs the optional ``dxfwrite`` package (not part of the hot path)."""
        from dxfwrite import DXFEngine as dxf  # noqa: optional dependency, raises if absent
        drawing = dxf.drawing(dxf_file)
        drawing.add_layer('Rays', color=3)
        for r0, rd in zip(self.rays_origin, self.rays_origin + self.rays_dir):
            drawing.add(dxf.face3d([r0[0:3], rd[0:3], rd[0:3]], layer="Rays"))
        drawing.save()


# the constructor's own default lambda: the device path reads it as cos_power(1)
_DEFAULT_DIRECTIVITY = light_source.__init__.__defaults__[2]
