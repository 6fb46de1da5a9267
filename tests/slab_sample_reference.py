"""TEST INFRASTRUCTURE: a numpy restatement of what include/sph_slab_sample.h adds to the field sampling -- the box of a particle and the
band of a rank's layer, every operation one float32 operation in the header's order, and the fold of the ranks' verdict words.  The
planes themselves are tests/sample_reference.py's.  Nothing here is imported by the product."""
import numpy as np

from tests import sample_reference as sr

f32 = np.float32
NONE = 0xFFFFFFFFFFFFFFFF
AUTO = 0x7FFFFFFF
MIN_EXPONENT, MAX_EXPONENT = -64, 64
FIELD_NAMES = {"density": "density", "pressure": "pressure", "velocity_x": "velocity", "velocity_y": "velocity",
               "constant_field": "constant_field", "level_estimation": "level_estimation"}


def boxes(x, y, h, nx, ny, origin, spacing):
    """-> (live[n], x0[n], x1[n], y0[n], y1[n]): sample_box per particle (the ints are meaningless where live is False)."""
    x, y, h = np.asarray(x, f32), np.asarray(y, f32), np.asarray(h, f32)
    ox, oy, sp = f32(origin[0]), f32(origin[1]), f32(spacing)
    with np.errstate(all="ignore"):
        gx = (x - ox) / sp - f32(0.5)
        gy = (y - oy) / sp - f32(0.5)
        rs = (f32(2.0) * h) / sp
        live = (np.abs(gx) < f32(1e30)) & (np.abs(gy) < f32(1e30)) & (rs >= f32(0.0))
        px = rs + (((np.abs(ox) + np.abs(x)) + f32(nx) * sp) * f32(4.8e-7)) / sp + rs * f32(1e-5)
        py = rs + (((np.abs(oy) + np.abs(y)) + f32(ny) * sp) * f32(4.8e-7)) / sp + rs * f32(1e-5)
        fx0 = np.maximum(np.floor(gx - px) - f32(1.0), f32(0.0))
        fx1 = np.minimum(np.ceil(gx + px) + f32(1.0), f32(nx - 1))
        fy0 = np.maximum(np.floor(gy - py) - f32(1.0), f32(0.0))
        fy1 = np.minimum(np.ceil(gy + py) + f32(1.0), f32(ny - 1))
        assert gx.dtype == px.dtype == fx0.dtype == f32
        live = live & (fx0 <= fx1) & (fy0 <= fy1)
    as_int = lambda v: np.where(live, v, f32(0)).astype(np.int64)   # noqa: E731
    return live, as_int(fx0), as_int(fx1), as_int(fy0), as_int(fy1)


def band(x, y, h, nx, ny, origin, spacing):
    """-> (sx0, sx1, n_boxes): the union of [x0, x1 + 1) over the particles whose box is live; (0, 0, 0) with none."""
    live, x0, x1, _, _ = boxes(x, y, h, nx, ny, origin, spacing)
    if not live.any():
        return 0, 0, 0
    return int(x0[live].min()), int(x1[live].max()) + 1, int(live.sum())


def reasons(p, exps=None):
    """int64[n]: the first failing precondition of every particle of the sr.Particles `p` (0: none), in sph_sample.h's order -- what
    sr.first_offender reports of the smallest index, for all of them."""
    with np.errstate(all="ignore"):
        ok_h = np.isfinite(p.h) & (p.h > 0)
        ok_v = np.isfinite(p.V) & (p.V >= 0)
        ok_vn = (p.V * p.norm).astype(f32) < f32(1048576.0)
        checks = [(~ok_h, sr.BAD_H), (~ok_v, sr.BAD_V), (~ok_vn, sr.BAD_VNORM)]
        for c in range(len(p.a)):
            lim = f32(np.inf) if exps is None or exps[c] is None else np.ldexp(f32(1.0), int(exps[c]))
            checks.append((~(np.abs(p.a[c]) < lim), sr.BAD_CHANNEL + c))
        bad = np.zeros(p.n, np.int64)
        for cond, code in checks:
            bad = np.where((bad == 0) & cond, code, bad)
    return bad


def words(p, ids, exps=None):
    """The verdict of one rank: `p` its owned particles, `ids` their global ids -> (first_bad, max_bits[6])."""
    bad = reasons(p, exps)
    idx = np.flatnonzero(bad)
    first = NONE
    if len(idx):
        i = idx[np.argmin(np.asarray(ids)[idx])]
        first = (int(ids[i]) << 8) | int(bad[i])
    bits = [int(np.abs(p.a[c]).max().view(np.uint32)) if p.n else 0 for c in range(len(p.a))]
    return first, tuple(bits + [0] * (6 - len(bits)))


def fold_words(words, channels, exps):
    """sph_sample_fold_words: `words` = [(first_bad, max_bits[6])] per rank, `channels` the channel names, `exps` one int or None (automatic)
    per channel -> ("ok", exponents) or ("refused", the sentence)."""
    first = min(w[0] for w in words)
    bits = [max(w[1][c] for w in words) for c in range(6)]
    if first != NONE:
        i, why = first >> 8, first & 0xFF
        if why == sr.BAD_H:
            return "refused", f"sample: the smoothing length is not finite and positive (particle i={i}; before the first step h is 0)"
        if why == sr.BAD_V:
            return "refused", f"sample: the volume m / rho is not finite and >= 0 (particle i={i})"
        if why == sr.BAD_VNORM:
            return "refused", f"sample: volume x kernel normalisation reaches 2^20 (particle i={i})"
        c = why - sr.BAD_CHANNEL
        name = FIELD_NAMES[channels[c]]
        if exps[c] is not None:
            return "refused", f"sample: channel {c} ({name}) is not finite or not below 2^exponent = {float(np.ldexp(f32(1.0), int(exps[c]))):g} (particle i={i})"
        return "refused", f"sample: channel {c} ({name}) is not finite (particle i={i})"
    out = []
    for c in range(len(channels)):
        if exps[c] is not None:
            out.append(int(exps[c]))
            continue
        e = max(sr.exponent_of(np.uint32(bits[c]).view(f32)), MIN_EXPONENT)
        if e > MAX_EXPONENT:
            return "refused", f"sample: channel {c} ({FIELD_NAMES[channels[c]]}) needs the exponent {e} (at most {MAX_EXPONENT})"
        out.append(e)
    return "ok", out
