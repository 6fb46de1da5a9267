"""The host side of sampling slab contexts (include/sph_slab_sample.h) without a device: sph_sample_fold_words through ctypes (it needs
no context) against its numpy restatement on hand-made words, and the twin's box and band (tests/slab_sample_reference.py) over
hand-placed particles."""
import numpy as np
import pytest

from adaptive_sph_amd import ffi, sampling
from tests import sample_reference as sr, slab_sample_reference as ssr

CH = ["density", "pressure", "velocity_x", "velocity_y", "level_estimation"]
GRID = sampling.GridSpec(40, 30, (-1.0, -0.5), 0.05)
NONE = ssr.NONE


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _w(first=NONE, **maxima):
    """One rank's words: max |a| per named channel of CH (0 elsewhere)."""
    return first, tuple(_bits(maxima.get(name, 0.0)) for name in CH) + (0,)


def _fold(lib, words, exps=None, msg_bytes=512):
    """-> ("ok", exponents) or ("refused", sentence) from the library, and the twin's answer beside it"""
    exps = [None] * len(CH) if exps is None else exps
    sp = sampling.sample_params(GRID, CH, exponents=exps)
    want = ssr.fold_words(words, CH, exps)
    try:
        out = ffi.sample_fold_words(lib, words, sp, msg_bytes)
    except ffi.SphError as e:
        assert e.status == 1
        return ("refused", str(e).split(": ", 1)[1]), want                     # (behind the status name)
    # the input is left alone, the copy carries the exponents
    assert [sp.channels[k].exponent for k in range(len(CH))] == [ffi.SAMPLE_AUTO_EXPONENT if e is None else e for e in exps]
    return ("ok", [int(out.channels[k].exponent) for k in range(len(CH))]), want


def _same(lib, words, exps=None):
    got, want = _fold(lib, words, exps)
    assert got[0] == want[0], (got, want)
    if got[0] == "ok":
        assert got[1] == want[1], (got, want)
    else:
        assert want[1] in got[1], (got, want)
    return got


def test_smallest_offending_id_wins_across_ranks(product_lib):
    a = _w((700 << 8) | sr.BAD_H, density=1.0)
    b = _w((41 << 8) | (sr.BAD_CHANNEL + 2), density=2.0)      # the higher rank holds the smaller id
    c = _w(NONE, density=3.0)
    for words in ([a, b, c], [c, b, a], [b, a]):
        got = _same(product_lib, words)
        assert got[0] == "refused" and "channel 2 (velocity) is not finite (particle i=41)" in got[1]
    got = _same(product_lib, [a, c])
    assert "smoothing length" in got[1] and "particle i=700; before the first step" in got[1]
    # the same id on two ranks cannot happen (one owner); equal ids with different reasons order by the reason all the same
    assert "volume m / rho" in _same(product_lib, [_w((9 << 8) | sr.BAD_V), _w((9 << 8) | sr.BAD_VNORM)])[1]
    assert "reaches 2^20 (particle i=9)" in _same(product_lib, [_w(NONE), _w((9 << 8) | sr.BAD_VNORM)])[1]
    # an explicit exponent: the sentence names 2^e
    got = _same(product_lib, [c, _w((12 << 8) | (sr.BAD_CHANNEL + 1))], [None, 3, None, None, None])
    assert "channel 1 (pressure) is not finite or not below 2^exponent = 8 (particle i=12)" in got[1]
    # a global id above 2^24 keeps all its bits (ids are 32-bit, the reason sits in the low byte)
    assert "(particle i=4000000000;" in _same(product_lib, [_w((4_000_000_000 << 8) | sr.BAD_H)])[1]


def test_exponents_of_the_whole_vector(product_lib):
    a = _w(density=1.01, pressure=300.0, velocity_x=0.3, velocity_y=2.0 ** -70)
    b = _w(density=0.99, pressure=5000.0, velocity_x=3.9, velocity_y=0.0)
    got = _same(product_lib, [a, b])
    # (the smallest e with max < 2^e; the ranks alone would take 9 and 13 for the pressure, -1 and 2 for velocity_x)
    assert got == ("ok", [1, 13, 2, -64, 0])                  # 2^-70 is raised to the lower end; a maximum of 0 gives 0
    assert ssr.fold_words([a], CH, [None] * 5)[1][:3] == [1, 9, -1] and ssr.fold_words([b], CH, [None] * 5)[1][:3] == [0, 13, 2]
    assert _same(product_lib, [b, a]) == got
    # exact powers of two: 2^e itself needs e + 1
    assert _same(product_lib, [_w(density=4.0), _w(density=3.9999)])[1][0] == 3
    # explicit exponents are left alone, whatever the maxima say
    assert _same(product_lib, [a, b], [7, None, -3, None, 20]) == ("ok", [7, 13, -3, -64, 20])
    # above the range: refused, on every order of the words
    big = _w(pressure=2.0 ** 70)
    for words in ([a, big], [big, a]):
        got = _same(product_lib, words)
        assert got[0] == "refused" and "channel 1 (pressure) needs the exponent 71 (at most 64)" in got[1]
    assert _same(product_lib, [_w(pressure=2.0 ** 63.5)])[1][1] == 64          # the upper end itself is allowed
    # an offender is reported before any exponent is looked at
    assert "particle i=3" in _same(product_lib, [big, _w((3 << 8) | sr.BAD_H)])[1]


def test_short_message_buffer_truncates(product_lib):
    words = [_w((41 << 8) | sr.BAD_H)]
    full = _fold(product_lib, words)[0][1]
    assert full.endswith("before the first step h is 0)")
    for size in (1, 2, 17, len(full), len(full) + 1):
        sp = sampling.sample_params(GRID, CH)
        with pytest.raises(ffi.SphError) as e:
            ffi.sample_fold_words(product_lib, words, sp, size)
        assert e.value.status == 1
        assert str(e.value).split(": ", 1)[1] == full[: size - 1]                  # size - 1 characters and the terminator
    # no buffer at all, and the malformed calls
    import ctypes as C
    arr = (ffi.SphSlabSampleWords * 1)(ffi.SphSlabSampleWords.from_tuple(words[0]))
    sp = sampling.sample_params(GRID, CH)
    assert product_lib.sample_fold_words(1, arr, C.byref(sp), None, 0) == 1
    assert product_lib.sample_fold_words(0, arr, C.byref(sp), None, 0) == 1
    assert product_lib.sample_fold_words(1, None, C.byref(sp), None, 0) == 1
    assert product_lib.sample_fold_words(1, arr, None, None, 0) == 1
    with pytest.raises(ffi.SphError, match="n < 1"):
        ffi.sample_fold_words(product_lib, [], sp)


def test_words_of_the_twin():
    """ssr.words against sr.first_offender, which the single-context tests pin: the same offender when the ids are the indices, the
    smallest ID -- not the smallest index -- when they are permuted."""
    rng = np.random.default_rng(2)
    n = 64
    f = {"position": rng.random((n, 2)).astype(np.float32), "h2": np.full(n, 0.05, np.float32), "mass": np.full(n, 1e-3, np.float32),
         "density": np.ones(n, np.float32), "pressure": (rng.random(n) * 300).astype(np.float32),
         "velocity": ((rng.random((n, 2)) - 0.5) * 7).astype(np.float32), "level_estimation": np.zeros(n, np.float32)}
    f["h2"][50] = 0.0
    f["velocity"][40, 0] = np.inf
    p = sr.Particles(f, CH, 1.0, 0.2)
    first, bits = ssr.words(p, np.arange(n))
    assert (first >> 8, first & 0xFF) == sr.first_offender(p) == (40, sr.BAD_CHANNEL + 2)
    assert bits[1] == _bits(np.abs(f["pressure"]).max()) and bits[5] == 0
    ids = np.arange(n)[::-1].copy()                              # index 50 now carries the id 13, index 40 the id 23
    first, _ = ssr.words(p, ids)
    assert (first >> 8, first & 0xFF) == (13, sr.BAD_H)
    assert ssr.words(p.subset(np.arange(30)), np.arange(30))[0] == NONE


def test_band_of_hand_placed_particles():
    nx, ny, origin, spacing = GRID.nx, GRID.ny, GRID.origin, GRID.spacing     # x in [-1, 1], y in [-0.5, 1]
    h = np.float32(0.05)                                                       # support radius 0.1: two samples
    inf, nan = np.float32(np.inf), np.float32(np.nan)

    def band(xs, ys, hs=None):
        hs = np.full(len(xs), h, np.float32) if hs is None else hs
        return ssr.band(np.array(xs, np.float32), np.array(ys, np.float32), np.array(hs, np.float32), nx, ny, origin, spacing)

    # inside: the box is the support in samples, one sample of slack and one of padding on either side
    live, x0, x1, y0, y1 = ssr.boxes(np.array([0.0], np.float32), np.array([0.0], np.float32), np.array([h]), nx, ny, origin, spacing)
    assert live[0] and (x0[0], x1[0]) == (16, 23) and (y0[0], y1[0]) == (6, 13)     # gx = 19.5, rs = 2: floor(17.5) - 1 .. ceil(21.5) + 1
    assert band([0.0], [0.0]) == (16, 24, 1)
    # clipped at column 0, at column nx - 1, and both in one band
    assert band([-0.98], [0.0]) == (0, 4, 1)
    assert band([0.98], [0.0]) == (36, 40, 1)
    assert band([-0.98, 0.98], [0.0, 0.0]) == (0, 40, 2)
    # outside the grid but within reach of the box's slack: still a (clipped) box; wholly outside: none
    assert band([-1.12], [0.0]) == (0, 2, 1)                      # gx = -2.9: x1 = ceil(-0.9) + 1 = 1
    assert band([-1.17], [0.0]) == (0, 1, 1)                      # gx = -3.9: x1 = ceil(-1.9) + 1 = 0
    assert band([-1.5], [0.0]) == (0, 0, 0) and band([1.5], [0.0]) == (0, 0, 0)
    assert band([0.0], [2.0]) == (0, 0, 0) and band([0.0], [-1.5]) == (0, 0, 0)     # the box must meet the grid in y as well
    assert band([0.0, -1.5, 0.0], [0.0, 0.0, 2.0]) == (16, 24, 1)
    # positions and smoothing lengths that are not finite: no box; the others' band is as without them
    for bad in ((nan, 0.0), (0.0, nan), (inf, 0.0), (0.0, -inf)):
        assert band([bad[0]], [bad[1]]) == (0, 0, 0)
        assert band([0.5, bad[0]], [0.0, bad[1]]) == band([0.5], [0.0])
    assert band([0.0], [0.0], [nan]) == (0, 0, 0) and band([0.0], [0.0], [-0.05]) == (0, 0, 0)
    assert band([0.0], [0.0], [0.0]) == (18, 22, 1)              # h = 0 (before the first step): floor(19.5) - 1 .. ceil(19.5) + 1, touching nothing
    assert band([], []) == (0, 0, 0)
    # every sample a particle touches lies in its box: brute force over the whole grid for particles all over the place
    rng = np.random.default_rng(7)
    xs = (rng.random(200) * 2.6 - 1.3).astype(np.float32)
    ys = (rng.random(200) * 2.0 - 0.8).astype(np.float32)
    hs = np.where(rng.random(200) < 0.3, 0.12, 0.03).astype(np.float32)
    live, x0, x1, y0, y1 = ssr.boxes(xs, ys, hs, nx, ny, origin, spacing)
    X, Y = sr.centers(nx, ny, origin, spacing)
    q = np.sqrt((X[None, None, :] - xs[:, None, None]) ** 2 + (Y[None, :, None] - ys[:, None, None]) ** 2) / (np.float32(2) * hs)[:, None, None]
    touch = q < 1
    assert live.sum() > 100 and (~live).sum() > 5 and not touch[~live].any()
    sxs, sys_ = np.arange(nx)[None, None, :], np.arange(ny)[None, :, None]
    inside = (sxs >= x0[:, None, None]) & (sxs <= x1[:, None, None]) & (sys_ >= y0[:, None, None]) & (sys_ <= y1[:, None, None])
    assert not (touch & ~inside).any()
