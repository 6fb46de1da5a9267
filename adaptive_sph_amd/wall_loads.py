"""Wall loads (include/sph_wall_load.h): the force, the torque and the normal force the fluid puts on every element of its boundary --
the planes of the box in the order given to the context, or the one polygon -- with the peak pressure at each and, along a plane, the
binned profile of the normal force.  Reduced on the device; the force is the one the pressure solve exchanges with the wall.

    load = wall_load(ctx, P)                                   # right behind a step
    load.force[2], load.torque[2], load.normal[2]              # the floor of a box: planes are left, right, floor, ceiling
    load = wall_load(ctx, P, bins=64, ranges=plane_ranges(planes, scene.boundary))
    s, q = load.profile(1)                                     # bin centres along the right wall, line pressure there

The sums are 128-bit fixed-point integers: `load.raw[k][name]` is the Python int, `load.exact(k, name)` the Fraction it stands for.
Pressure and density are the last STEP's, the positions are where that step left the particles: ask right behind the step, before
anything edits the particle vector.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import ffi


def _lib(lib):
    if any(getattr(lib, s, None) is None for s in ffi.WALL_LOAD_SYMBOLS):
        raise ffi.SphError(30, f"{lib.path.name} computes no wall loads (sph_wall_load.h is implemented by the product library only)")
    return lib


def _ffi_params(P):
    return P.to_ffi() if hasattr(P, "to_ffi") else P


def wall_load_spec(bins: int = 0, ranges=None, exponents=None) -> "ffi.SphWallLoadSpec":
    """The sph_wall_load_spec of a call.  `ranges`: per element None (no profile) or (s_lo, s_hi) or (s_lo, s_hi, B) with B <= bins
    (default: bins); `exponents`: None (all automatic), or per element None or four ints / None (force_x, force_y, torque, normal)."""
    spec = ffi.SphWallLoadSpec()
    spec.bins = int(bins)
    for k in range(ffi.WALL_LOAD_MAX_ELEMENTS):
        row = None if exponents is None or k >= len(exponents) else exponents[k]
        for s in range(ffi.WALL_LOAD_N_SUMS):
            e = None if row is None else row[s]
            spec.exponent[k][s] = ffi.LEDGER_AUTO_EXPONENT if e is None else int(e)
        r = None if ranges is None or k >= len(ranges) else ranges[k]
        if r is not None:
            spec.s_lo[k], spec.s_hi[k] = float(r[0]), float(r[1])
            spec.n_bins[k] = int(r[2]) if len(r) > 2 else int(bins)
    return spec


def plane_ranges(planes, boundary) -> List[Optional[Tuple[float, float]]]:
    """The extent of every plane of a box inside the box, in the plane's tangential coordinate s = -dir_y x + dir_x y: the default
    ranges of a profile.  None for a plane that is not axis-aligned."""
    hw, hh = float(boundary.width) / 2.0, float(boundary.height) / 2.0
    out: List[Optional[Tuple[float, float]]] = []
    for dx, dy, _ in planes:
        if dy == 0 and dx != 0:
            out.append((-hh, hh))
        elif dx == 0 and dy != 0:
            out.append((-hw, hw))
        else:
            out.append(None)
    return out


class WallLoad:
    """A sph_wall_load_result by element and name, with the profile's words."""

    def __init__(self, result: "ffi.SphWallLoadResult", words: Optional[np.ndarray], spec: "ffi.SphWallLoadSpec"):
        self.result, self.words = result, words
        self.n_elements, self.bins, self.n = int(result.n_elements), int(result.bins), int(result.n)
        el = [result.element[k] for k in range(self.n_elements)]
        names = ffi.WALL_LOAD_SUMS
        self.exponents: List[Dict[str, int]] = [{name: int(e.exponent[s]) for s, name in enumerate(names)} for e in el]
        self.raw: List[Dict[str, int]] = [{name: e.raw[s].as_int() for s, name in enumerate(names)} for e in el]
        self.sums: List[Dict[str, float]] = [{name: float(e.sum[s]) for s, name in enumerate(names)} for e in el]
        self.force: List[Tuple[float, float]] = [(d["force_x"], d["force_y"]) for d in self.sums]
        self.torque: List[float] = [d["torque"] for d in self.sums]
        self.normal: List[float] = [d["normal"] for d in self.sums]
        self.n_entries: List[int] = [int(e.n_entries) for e in el]
        self.n_wet: List[int] = [int(e.n_wet) for e in el]
        self.n_unbinned: List[int] = [int(e.n_unbinned) for e in el]
        self._ranges = [(float(spec.s_lo[k]), float(spec.s_hi[k]), int(e.n_bins)) for k, e in enumerate(el)]

    def __bytes__(self):
        return bytes(self.result)

    def exact(self, k: int, name: str) -> Fraction:
        """The sum as the rational number its integer stands for: Q * 2^(e - 60)."""
        return Fraction(self.raw[k][name]) * (Fraction(2) ** (self.exponents[k][name] - 60))

    def peak_pressure(self, k: int) -> Tuple[float, int]:
        """(value, id) of the largest pressure among the particles with an entry at element k; id == ffi.LEDGER_NO_ID without entries."""
        e = self.result.element[k].max_pressure
        return float(e.value), int(e.id)

    @property
    def total_force(self) -> Tuple[float, float]:
        """The sum over the elements, added exactly and rounded once."""
        return (float(sum((self.exact(k, "force_x") for k in range(self.n_elements)), Fraction(0))),
                float(sum((self.exact(k, "force_y") for k in range(self.n_elements)), Fraction(0))))

    def bin_forces(self, k: int) -> np.ndarray:
        """The normal force of every bin of element k: (double)word * 2^(e_normal - 40)."""
        lo, hi, B = self._ranges[k]
        if self.words is None or B == 0:
            return np.zeros(0)
        return np.ldexp(self.words[k, :B].astype(np.float64), self.exponents[k]["normal"] - ffi.WALL_LOAD_BIN_SHIFT)

    def profile(self, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """(s_centres, line_pressure): the bins' centres along element k and the normal force per length there."""
        lo, hi, B = self._ranges[k]
        f = self.bin_forces(k)
        if B == 0 or not len(f):
            return np.zeros(0), np.zeros(0)
        width = (hi - lo) / B
        return lo + (np.arange(B) + 0.5) * width, f / width


def wall_load(ctx, P, bins: int = 0, ranges=None, exponents=None) -> WallLoad:
    """sph_wall_load_compute on a plain context (see wall_load_spec for `ranges` and `exponents`, or give a spec as `bins`)."""
    lib = _lib(ctx.lib)
    spec = bins if isinstance(bins, ffi.SphWallLoadSpec) else wall_load_spec(bins, ranges, exponents)
    p = _ffi_params(P)
    out = ffi.SphWallLoadResult()
    words = np.zeros((ffi.WALL_LOAD_MAX_ELEMENTS, max(int(spec.bins), 0)), np.int64) if spec.bins > 0 else None
    ctx._check(lib.wall_load_compute(ctx.handle, C.byref(p) if p is not None else None, C.byref(spec), C.byref(out),
                                     words.ctypes.data if words is not None else None))
    return WallLoad(out, None if words is None else words[:int(out.n_elements)], spec)


# ---- the run subcommand's --wall-loads FILE.csv and --wall-load-profile DIR ---------------------------------------------------------
ELEMENT_COLUMNS = ["fx", "fy", "torque", "normal", "n_wet", "peak_p", "peak_id"]


def csv_columns(n_elements: int) -> List[str]:
    return ["step", "time", "dt"] + [f"{c}_{k}" for k in range(n_elements) for c in ELEMENT_COLUMNS]


def csv_row(step: int, time: float, dt: float, load: WallLoad) -> List[str]:
    """One row of csv_columns(load.n_elements) as strings (repr of the doubles: they read back bit for bit)."""
    row = [str(int(step)), repr(float(time)), repr(float(dt))]
    for k in range(load.n_elements):
        value, pid = load.peak_pressure(k)
        row += [repr(load.force[k][0]), repr(load.force[k][1]), repr(load.torque[k]), repr(load.normal[k]), str(load.n_wet[k]), repr(value), str(pid)]
    return row


def profile_rows(load: WallLoad) -> Sequence[List[str]]:
    """The rows of a profile file: element, bin, s, line_pressure."""
    rows = [["element", "bin", "s", "line_pressure"]]
    for k in range(load.n_elements):
        s, q = load.profile(k)
        rows += [[str(k), str(b), repr(float(s[b])), repr(float(q[b]))] for b in range(len(s))]
    return rows
