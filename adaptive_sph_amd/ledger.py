"""The state ledger (include/sph_ledger.h): what a host asks of a running simulation to watch it, reduced on the device -- conserved
quantities as exact integers, extremes with the id of the particle that attains them, counts, and the refusal that names the smallest
particle that is not finite.

    led = ledger(ctx, P)                      # one context
    led = ledger_group(contexts, P)           # the slab contexts of one process
    # one process per rank: every rank computes its words, the words travel, every rank folds them; then the sums, then compose
    words = ledger_rank_words(ctx, P);  spec, _ = fold(all_words, what);  sums = ledger_rank_sums(ctx, P, spec)
    led = compose(all_words, all_sums, spec)

The sums are 128-bit fixed-point integers: `led.raw[name]` is the Python int, `led.exact(name)` the Fraction it stands for, `led.mass`,
`led.momentum`, ... its nearest double.  The three paths give the same result byte for byte for the same particles, whatever the cuts.
"""
from __future__ import annotations

import ctypes as C
import math
from fractions import Fraction
from typing import Dict, Optional, Sequence, Tuple

from . import ffi

ALL = ("carried", "step_outputs", "outside")


def _what_bits(what) -> int:
    if isinstance(what, int):
        return what
    if isinstance(what, str):
        what = [what]
    bits = 0
    for w in what:
        if w not in ffi.LEDGER_GROUPS:
            raise ValueError(f"unknown ledger group {w!r} (known: {sorted(ffi.LEDGER_GROUPS)})")
        bits |= ffi.LEDGER_GROUPS[w]
    return bits


def ledger_spec(what=ALL, exponents=None) -> "ffi.SphLedgerSpec":
    """The sph_ledger_spec of a call.  `what`: group names of ffi.LEDGER_GROUPS (or the bit set); `exponents`: None (all automatic), a
    dict sum name -> int, or one int / None per sum."""
    spec = ffi.SphLedgerSpec()
    spec.what = _what_bits(what)
    if isinstance(exponents, dict):
        unknown = set(exponents) - set(ffi.LEDGER_SUMS)
        if unknown:
            raise ValueError(f"unknown ledger sums {sorted(unknown)} (known: {ffi.LEDGER_SUMS})")
        exponents = [exponents.get(name) for name in ffi.LEDGER_SUMS]
    for s in range(ffi.LEDGER_N_SUMS):
        e = None if exponents is None else exponents[s]
        spec.exponent[s] = ffi.LEDGER_AUTO_EXPONENT if e is None else int(e)
    return spec


def _ledger_lib(lib):
    if any(getattr(lib, s, None) is None for s in ffi.LEDGER_SYMBOLS):
        raise ffi.SphError(30, f"{lib.path.name} keeps no ledger (sph_ledger.h is implemented by the product library only)")
    return lib


def _ffi_params(P):
    return P.to_ffi() if hasattr(P, "to_ffi") else P


def _spec_of(what, exponents):
    return what if isinstance(what, ffi.SphLedgerSpec) else ledger_spec(what, exponents)


class Ledger:
    """A sph_ledger_result by name."""

    def __init__(self, result: "ffi.SphLedgerResult"):
        self.result = result
        self.what = int(result.what)
        self.n, self.n_outside = int(result.n), int(result.n_outside)
        self.exponents: Dict[str, int] = {name: int(result.exponent[s]) for s, name in enumerate(ffi.LEDGER_SUMS)}
        self.raw: Dict[str, int] = {name: result.raw[s].as_int() for s, name in enumerate(ffi.LEDGER_SUMS)}
        self.sums: Dict[str, float] = {name: float(result.sum[s]) for s, name in enumerate(ffi.LEDGER_SUMS)}
        self.extremes: Dict[str, Tuple[float, int]] = {name: (float(result.extreme[k].value), int(result.extreme[k].id))
                                                       for k, name in enumerate(ffi.LEDGER_EXTREMES)}

    def __bytes__(self):
        return bytes(self.result)

    def has(self, group: str) -> bool:
        return bool(self.what & ffi.LEDGER_GROUPS[group])

    def __getattr__(self, name):
        if name in ffi.LEDGER_SUMS and "sums" in self.__dict__:
            return self.__dict__["sums"][name]
        raise AttributeError(name)

    def exact(self, name: str) -> Fraction:
        """The sum as the rational number its integer stands for: Q * 2^(e - 60)."""
        e = self.exponents[name] - 60
        return Fraction(self.raw[name]) * (Fraction(2) ** e)

    def extreme(self, name: str) -> Tuple[float, int]:
        """(value, id); id == ffi.LEDGER_NO_ID where no particle took part or the group was not asked for."""
        return self.extremes[name]

    @property
    def momentum(self) -> Tuple[float, float]:
        return self.sums["momentum_x"], self.sums["momentum_y"]

    @property
    def centre_of_mass(self) -> Tuple[float, float]:
        """(sum m x, sum m y) / sum m, each quotient taken exactly and rounded once; NaN without mass."""
        m = self.exact("mass")
        if m == 0:
            return float("nan"), float("nan")
        return float(self.exact("moment_x") / m), float(self.exact("moment_y") / m)

    @property
    def vmax(self) -> float:
        return math.sqrt(self.extremes["max_speed2"][0])

    def potential_energy(self, P) -> float:
        """- g sum m y with the step's gravity (the signed acceleration along y the step adds)."""
        return float(-Fraction(float(_ffi_params(P).gravity)) * self.exact("moment_y"))

    def mean_density_error(self, P) -> float:
        """The mean of max(rho - rest_density, 0) over the particles, relative to rest_density (the density solver's measure); NaN
        without particles."""
        if self.n == 0:
            return float("nan")
        return float(self.exact("compression") / self.n / Fraction(float(_ffi_params(P).rest_density)))


def ledger(ctx, P, what=ALL, exponents=None) -> Ledger:
    """sph_ledger_compute on a plain context.  Step outputs (density, pressure, h) are the last STEP's: ask right behind the step, before
    anything edits the particle vector; the carried group and the outside count are valid at any time."""
    lib = _ledger_lib(ctx.lib)
    spec = _spec_of(what, exponents)
    p = _ffi_params(P)
    out = ffi.SphLedgerResult()
    ctx._check(lib.ledger_compute(ctx.handle, C.byref(p) if p is not None else None, C.byref(spec), C.byref(out)))
    return Ledger(out)


def ledger_group(contexts, P, what=ALL, exponents=None) -> Ledger:
    """sph_group_ledger: the slab contexts of this process (the group sph_group_step steps)."""
    contexts = list(contexts)
    if not contexts:
        raise ffi.SphError(1, "sph_group_ledger: n < 1 (no contexts)")
    lib = _ledger_lib(contexts[0].lib)
    spec = _spec_of(what, exponents)
    p = _ffi_params(P)
    handles = (C.c_void_p * len(contexts))(*[c.handle for c in contexts])
    out = ffi.SphLedgerResult()
    rc = lib.group_ledger(handles, len(contexts), C.byref(p) if p is not None else None, C.byref(spec), C.byref(out))
    if rc != 0:   # (whichever member refused, the library leaves the sentence in member 0's last error)
        raise ffi.SphError(rc, lib.last_error(contexts[0].handle).decode(errors="replace"))
    return Ledger(out)


def ledger_rank_words(ctx, P, what=ALL, exponents=None) -> "ffi.SphLedgerWords":
    """sph_slab_ledger_range: this rank's words over its owned particles.  The ranks' words go to `fold`."""
    lib = _ledger_lib(ctx.lib)
    spec = _spec_of(what, exponents)
    p = _ffi_params(P)
    out = ffi.SphLedgerWords()
    ctx._check(lib.slab_ledger_range(ctx.handle, C.byref(p) if p is not None else None, C.byref(spec), C.byref(out)))
    return out


def ledger_rank_sums(ctx, P, spec: "ffi.SphLedgerSpec"):
    """sph_slab_ledger_sums: this rank's nine 128-bit sums under spec's explicit exponents (what `fold` returns) -> a list of Python ints."""
    lib = _ledger_lib(ctx.lib)
    p = _ffi_params(P)
    out = (ffi.SphLedgerSum * ffi.LEDGER_N_SUMS)()
    ctx._check(lib.slab_ledger_sums(ctx.handle, C.byref(p) if p is not None else None, C.byref(spec) if spec is not None else None, out))
    return [q.as_int() for q in out]


def _words_array(words):
    words = list(words)
    arr = (ffi.SphLedgerWords * max(1, len(words)))()
    for i, w in enumerate(words):
        arr[i] = w if isinstance(w, ffi.SphLedgerWords) else ffi.SphLedgerWords.from_tuple(w)
    return words, arr


def fold(words, what=ALL, exponents=None, lib: Optional["ffi.SphLibrary"] = None, msg_bytes: int = 512):
    """sph_ledger_fold_words (no device, no context): the ranks' words -> (a copy of the spec whose automatic exponents are those of the
    whole vector, the folded words).  Raises SphError(1) with the sentence `ledger` writes when a particle offends (the smallest id over
    the ranks) or an exponent is out of range: the same on every rank that folds the same words."""
    lib = _ledger_lib(lib if lib is not None else ffi.load_product())
    spec = _spec_of(what, exponents)
    words, arr = _words_array(words)
    out = ffi.SphLedgerSpec.from_buffer_copy(spec)
    folded = ffi.SphLedgerWords()
    msg = C.create_string_buffer(max(1, int(msg_bytes)))
    rc = lib.ledger_fold_words(len(words), arr, C.byref(out), C.byref(folded), msg, int(msg_bytes))
    if rc != 0:
        raise ffi.SphError(rc, msg.value.decode(errors="replace"))
    return out, folded


def compose(words, sums: Sequence[Sequence[int]], spec: "ffi.SphLedgerSpec", lib: Optional["ffi.SphLibrary"] = None) -> Ledger:
    """sph_ledger_compose (no device, no context): the ranks' words and their sums (one list of nine Python ints per rank) under the
    folded spec -> the Ledger of the whole vector."""
    lib = _ledger_lib(lib if lib is not None else ffi.load_product())
    words, arr = _words_array(words)
    sums = list(sums)
    if len(sums) != len(words):
        raise ValueError(f"{len(words)} ranks' words, {len(sums)} ranks' sums")
    flat = (ffi.SphLedgerSum * max(1, len(sums) * ffi.LEDGER_N_SUMS))()
    for r, row in enumerate(sums):
        for s in range(ffi.LEDGER_N_SUMS):
            flat[r * ffi.LEDGER_N_SUMS + s] = ffi.SphLedgerSum.from_int(row[s])
    out = ffi.SphLedgerResult()
    rc = lib.ledger_compose(len(words), arr, flat, C.byref(spec) if spec is not None else None, C.byref(out))
    if rc != 0:
        raise ffi.SphError(rc, "sph_ledger_compose: n < 1, a null pointer, no or an unknown group, an automatic or out-of-range exponent, or words that "
                               "name an offender (sph_ledger_fold_words comes first)")
    return Ledger(out)


# ---- the run subcommand's --ledger FILE.csv --------------------------------------------------------------------------------------
CSV_COLUMNS = (["step", "time", "dt", "n"] + ffi.LEDGER_SUMS +
               ["centre_of_mass_x", "centre_of_mass_y", "potential_energy", "mean_density_error", "vmax", "vmax_id", "y_min", "y_min_id", "rho_max",
                "rho_max_id", "p_max", "n_outside", "adapt_d_mass", "adapt_d_momentum_x", "adapt_d_momentum_y"])


def csv_row(step: int, time: float, dt: float, led: Ledger, P, after: Optional[Ledger] = None):
    """One row of CSV_COLUMNS as strings (repr of the doubles: they read back bit for bit).  `after`: the carried ledger taken behind the
    step's adaptivity; the adapt_d_* columns are its sums minus led's, computed exactly and rounded once (empty without it)."""
    cx, cy = led.centre_of_mass
    row = [str(int(step)), repr(float(time)), repr(float(dt)), str(led.n)] + [repr(led.sums[name]) for name in ffi.LEDGER_SUMS]
    row += [repr(cx), repr(cy), repr(led.potential_energy(P)), repr(led.mean_density_error(P)), repr(led.vmax), str(led.extreme("max_speed2")[1]),
            repr(led.extreme("min_y")[0]), str(led.extreme("min_y")[1]), repr(led.extreme("max_density")[0]), str(led.extreme("max_density")[1]),
            repr(led.extreme("max_pressure")[0]), str(led.n_outside)]
    if after is None:
        row += ["", "", ""]
    else:
        row += [repr(float(after.exact(name) - led.exact(name))) for name in ("mass", "momentum_x", "momentum_y")]
    return row
