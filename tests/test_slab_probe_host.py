"""include/sph_slab_probe.h against the built product library and its ctypes mirror, the numpy twin of the compact layers and their
compose (tests/slab_probe_reference.py), and sph_probe_fold_words against sph_sample_fold_words (no GPU needed)."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import ffi, probes, sampling
from tests import probe_reference as pr
from tests import sample_reference as sr
from tests import slab_probe_reference as spr
from tests.test_probe_host import _synthetic

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "sph_slab_probe.h"
NAMES = ["sph_slab_probe_range", "sph_probe_fold_words", "sph_slab_probe_layer", "sph_slab_probe_layer_download", "sph_probe_compose",
         "sph_probe_compose_advect", "sph_group_probe_sample", "sph_group_probe_advect"]


def _code():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_library_exports_exactly_the_declared_functions():
    declared = re.findall(r"\bint\s+(sph_\w+)\s*\(", _code())
    assert sorted(declared) == sorted(NAMES)
    lib = C.CDLL(str(ffi.PRODUCT_LIB))
    for n in NAMES:
        assert hasattr(lib, n), n
    assert sorted("sph_" + s for s in ffi.SLAB_PROBE_SYMBOLS) == sorted(NAMES)
    others = [k for k in dir(ffi) if k.endswith("_SYMBOLS") and k != "SLAB_PROBE_SYMBOLS"]
    assert {"ABI_SYMBOLS", "PROBE_SYMBOLS", "SAMPLE_SYMBOLS", "SLAB_SAMPLE_SYMBOLS", "LEDGER_SYMBOLS", "SLAB_RENDER_SYMBOLS"} <= set(others)
    for other in others:
        assert not set(ffi.SLAB_PROBE_SYMBOLS) & set(getattr(ffi, other)), other
    # the headers beside it stay what they were
    for name in ("sph_ffi.h", "sph_sample.h"):
        assert "probe" not in (REPO / "include" / name).read_text()
    probe_h = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sph_probe.h").read_text(), flags=re.S)
    assert len(re.findall(r"\bint\s+(sph_\w+)\s*\(", probe_h)) == 8
    assert "sph_slab_probe.h" in (REPO / "include" / "sph_probe.h").read_text()


def test_struct_sizes_equal_the_header():
    pinned = dict(re.findall(r"SPH_PROBE_STATIC_ASSERT\(sizeof\((\w+)\) == (\d+)", _code()))
    assert pinned == {"sph_slab_probe_layer_info": "48", "sph_slab_sample_words": "32"}
    assert C.sizeof(ffi.SphSlabProbeLayerInfo) == 48 and C.sizeof(ffi.SphSlabSampleWords) == 32
    I = ffi.SphSlabProbeLayerInfo
    assert [f[0] for f in I._fields_] == ["exponents", "n_entries", "n_touching", "n_pairs"]
    assert (I.exponents.offset, I.n_entries.offset, I.n_touching.offset, I.n_pairs.offset) == (0, 24, 32, 40)
    body = re.search(r"typedef struct sph_slab_probe_layer_info \{(.*?)\}", _code(), re.S).group(1)
    assert re.search(r"int32_t\s+exponents\[SPH_SAMPLE_MAX_CHANNELS\];\s*uint64_t\s+n_entries;\s*uint64_t\s+n_touching;\s*uint64_t\s+n_pairs;", body)


def test_a_c_compiler_accepts_the_header():
    """The header's own static assertions, by a C compiler: gcc, else cc, else the clang beside the hipcc that built the library -- one of
    them exists wherever the library was built, so the check never passes unrun."""
    from adaptive_sph_amd.build import hipcc_path
    clang = Path(hipcc_path()).resolve().parent.parent / "llvm" / "bin" / "clang"
    cc = shutil.which("gcc") or shutil.which("cc") or (str(clang) if clang.exists() else None) or shutil.which("clang")
    assert cc, "no C compiler found (gcc, cc, clang): the header's static assertions were not checked"
    r = subprocess.run([cc, "-std=c11", "-fsyntax-only", "-I", str(REPO / "include"), "-x", "c", str(HEADER)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_ffi_signatures_agree_with_the_header(product_lib):
    decl = {}
    for name, args in re.findall(r"\bint\s+(sph_\w+)\s*\((.*?)\);", _code(), re.S):
        decl[name] = [re.sub(r"\s+", "", re.sub(r"\b\w+$", "", a.strip())) for a in args.split(",")]
    assert decl["sph_probe_fold_words"] == ["int", "constsph_slab_sample_words*", "sph_probe_params*", "char*", "uint64_t"]
    assert decl["sph_slab_probe_layer_download"] == ["sph_ctx*", "sph_probe_set*", "uint32_t*", "int64_t*", "uint64_t"]
    for name in NAMES:
        fn = getattr(product_lib, name[4:])
        assert fn is not None and fn.restype is C.c_int32 and len(fn.argtypes) == len(decl[name]), name
        for t, d in zip(fn.argtypes, decl[name]):
            if d == "int":
                assert t is C.c_int32, (name, d)
            elif d == "uint64_t":
                assert t is C.c_uint64, (name, d)
            else:
                assert d.endswith("*") and C.sizeof(t) == C.sizeof(C.c_void_p), (name, d)


# ---- the twin: the layers of x-slabs compose to the whole vector's words -----------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3])
def test_the_layers_of_slabs_compose_to_the_whole(k):
    f = _synthetic()
    channels = list(sr.CHANNELS)
    p = sr.Particles(f, channels, 1000.0, 0.25, "density")
    exps = sr.exponents(p)
    rng = np.random.default_rng(17)
    pts = rng.uniform([-0.8, -0.7], [1.2, 0.8], (257, 2)).astype(np.float32)
    PX, PY = pts[:, 0], pts[:, 1]
    whole, foot, touched = pr.raw_at_points(p, exps, PX, PY)
    cuts = np.quantile(p.x, np.arange(1, k) / k)
    rank = np.searchsorted(cuts, p.x, side="right")
    owns = [np.flatnonzero(rank == r) for r in range(k)]
    assert all(len(o) > 20 for o in owns) and sum(len(o) for o in owns) == p.n
    layers = [spr.layer(p, own, exps, PX, PY) for own in owns]
    for (idx, words, _), own in zip(layers, owns):
        assert idx.dtype == np.uint32 and words.shape == (7, len(idx)) and 0 < len(idx) < len(pts) and (np.diff(idx.astype(np.int64)) > 0).all()
    # two ranks contribute to the same point; the entries of the ranks overlap but none holds them all
    assert len(np.intersect1d(layers[0][0], layers[1][0])) > 0
    got, seen = spr.compose(7, len(pts), [(i, w) for i, w, _ in layers])
    assert np.array_equal(got, whole) and np.array_equal(seen, touched) and (~touched).any()
    assert sum(int(fr.sum()) for _, _, fr in layers) == int(foot.sum()) and sum(int((fr > 0).sum()) for _, _, fr in layers) == int((foot > 0).sum())
    # any order of the layers, and layers without entries among them
    for order in ([k - 1 - r for r in range(k)], list(np.random.default_rng(3).permutation(k))):
        again, _ = spr.compose(7, len(pts), [None] + [(layers[r][0], layers[r][1]) for r in order] + [(np.zeros(0, np.uint32), np.zeros((7, 0), np.int64))])
        assert np.array_equal(again, whole)
    assert not spr.compose(7, len(pts), [])[0].any()


def test_a_touched_point_with_all_zero_words_is_an_entry():
    """One particle whose weight term truncates to 0 at a point just inside its support, with a channel of zeros: q < 1 holds, every
    word is 0, the point is an entry all the same."""
    f32 = np.float32
    h = f32(0.05)
    fields = {"position": np.array([[0.0, 0.0]], f32), "h2": np.array([h]), "mass": np.array([1e-7], f32), "density": np.array([1000.0], f32),
              "pressure": np.zeros(1, f32), "velocity": np.zeros((1, 2), f32), "constant_field": np.zeros(1, f32), "level_estimation": np.zeros(1, f32)}
    p = sr.Particles(fields, ["pressure"], 1000.0, 0.25, "density")
    PX = np.array([2 * h * f32(0.999), 0.0, 1.0], f32)
    PY = np.zeros(3, f32)
    idx, words, foot = spr.layer(p, np.array([0]), [0], PX, PY)
    assert idx.tolist() == [0, 1] and foot.tolist() == [2]
    assert not words[:, 0].any() and words[0, 1] > 0, words
    got, seen = spr.compose(2, 3, [(idx, words)])
    assert seen.tolist() == [True, True, False] and not got[:, 0].any()


# ---- sph_probe_fold_words equals sph_sample_fold_words -----------------------------------------------------------------------------
def _words(first_bad, bits):
    return ffi.SphSlabSampleWords.from_tuple((first_bad, tuple(bits) + (0,) * (6 - len(bits))))


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_fold_words_is_the_lattice_fold(product_lib):
    names = ["density", "velocity_x", "velocity_y"]
    grid = sampling.GridSpec(4, 3, (0.0, 0.0), 0.1)
    none = ffi.SAMPLE_NO_OFFENDER
    ranks = [_words(none, [_bits(1020.5), _bits(0.3), _bits(0.0)]), _words(none, [_bits(998.0), _bits(3.75), _bits(0.0)]),
             _words(none, [_bits(5.0), _bits(0.001), _bits(0.0)])]
    for exps in (None, [None, 5, None], [11, 2, -3]):
        pp = probes.probe_params(names, exponents=exps)
        sp = sampling.sample_params(grid, names, exponents=exps)
        for order in (ranks, ranks[::-1], ranks[:1]):
            a = ffi.probe_fold_words(product_lib, order, pp)
            b = ffi.sample_fold_words(product_lib, order, sp)
            got = [a.channels[k].exponent for k in range(3)]
            assert got == [b.channels[k].exponent for k in range(3)]
            if exps is None and len(order) == 3:
                assert got == [10, 2, 0]                                   # 1020.5 < 2^10, 3.75 < 2^2, a field of zeros
            if exps == [11, 2, -3]:
                assert got == exps                                           # explicit exponents are left alone
        assert [pp.channels[k].exponent for k in range(3)] == [ffi.SAMPLE_AUTO_EXPONENT if e is None else e for e in (exps or [None] * 3)]   # a copy
    # a maximum above the range: "needs the exponent"
    for fold, q in ((ffi.probe_fold_words, probes.probe_params(names)), (ffi.sample_fold_words, sampling.sample_params(grid, names))):
        with pytest.raises(ffi.SphError, match=r"channel 1 \(velocity\) needs the exponent 65 \(at most 64\)") as e:
            fold(product_lib, [_words(none, [_bits(1.0), _bits(2.0 ** 64), 0])], q)
        assert e.value.status == 1


def test_fold_words_refuses_with_the_lattice_sentence(product_lib):
    names = ["pressure", "velocity_x"]
    grid = sampling.GridSpec(4, 3, (0.0, 0.0), 0.1)
    none = ffi.SAMPLE_NO_OFFENDER
    for exps in ([None, 1], [None, None]):
        pp = probes.probe_params(names, exponents=exps)
        sp = sampling.sample_params(grid, names, exponents=exps)
        for reason in (sr.BAD_H, sr.BAD_V, sr.BAD_VNORM, sr.BAD_CHANNEL, sr.BAD_CHANNEL + 1):
            ranks = [_words(none, [1, 2]), _words(907 << 8 | reason, [3, 4]), _words(41 << 8 | reason, [5, 6]), _words(5000 << 8 | sr.BAD_H, [0, 0])]
            said = []
            for fold, q in ((ffi.probe_fold_words, pp), (ffi.sample_fold_words, sp)):
                with pytest.raises(ffi.SphError) as e:
                    fold(product_lib, ranks, q)
                assert e.value.status == 1
                said.append(e.value.args[1] if len(e.value.args) > 1 else str(e.value))
            assert said[0] == said[1] and "(particle i=41" in said[0], said     # the smallest offending global id
    # a short msg truncates, terminates and does not fail otherwise; msg may be NULL
    arr = (ffi.SphSlabSampleWords * 2)(_words(none, [1, 2]), _words(41 << 8 | sr.BAD_H, [3, 4]))
    full = C.create_string_buffer(512)
    pp = probes.probe_params(names)
    assert product_lib.probe_fold_words(2, arr, C.byref(pp), full, 512) == 1 and full.value.startswith(b"sample: the smoothing length")
    for size in (1, 8, 33):
        buf = C.create_string_buffer(b"\xff" * 64, 64)
        assert product_lib.probe_fold_words(2, arr, C.byref(pp), buf, size) == 1
        assert buf.raw[:size] == full.value[:size - 1] + b"\0" and buf.raw[size:] == b"\xff" * (64 - size)
    assert product_lib.probe_fold_words(2, arr, C.byref(pp), None, 0) == 1
    assert [pp.channels[k].exponent for k in range(2)] == [ffi.SAMPLE_AUTO_EXPONENT] * 2          # a refusal leaves pp_io alone
    # n < 1, null words, null parameters
    buf = C.create_string_buffer(128)
    for n, w, q in ((0, arr, C.byref(pp)), (2, None, C.byref(pp)), (2, arr, None)):
        assert product_lib.probe_fold_words(n, w, q, buf, 128) == 1 and b"sph_probe_fold_words: n < 1" in buf.value
