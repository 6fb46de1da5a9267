"""include/sph_slab_sample.h against the built product library and its ctypes mirror (no GPU needed: symbols, signatures and sizes only)."""
import ctypes as C
import re
from pathlib import Path

from adaptive_sph_amd import ffi

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "sph_slab_sample.h"
NAMES = ["sph_slab_sample_range", "sph_sample_fold_words", "sph_slab_sample_layer", "sph_slab_sample_layer_download", "sph_sample_compose",
         "sph_group_sample_grid"]


def _code():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _declarations():
    """name -> the parameter types of its declaration, spaces removed"""
    out = {}
    for name, args in re.findall(r"\bint\s+(sph_\w+)\s*\(([^)]*)\)\s*;", _code()):
        out[name] = [re.sub(r"\s*\b\w+$", "", a.strip()).replace(" ", "") for a in args.split(",")]
    return out


def test_library_exports_the_six_declared_functions():
    decl = _declarations()
    assert sorted(decl) == sorted(NAMES)
    lib = C.CDLL(str(ffi.PRODUCT_LIB))
    for n in NAMES:
        assert hasattr(lib, n), n
    assert sorted("sph_" + s for s in ffi.SLAB_SAMPLE_SYMBOLS) == sorted(NAMES)
    assert not set(ffi.SLAB_SAMPLE_SYMBOLS) & set(ffi.ABI_SYMBOLS) and not set(ffi.SLAB_SAMPLE_SYMBOLS) & set(ffi.SAMPLE_SYMBOLS)


def test_signatures_are_the_stated_ones():
    decl = _declarations()
    ctx, par, sp = "sph_ctx*", "constsph_params*", "constsph_sample_params*"
    assert decl["sph_slab_sample_range"] == [ctx, par, sp, "sph_slab_sample_words*"]
    assert decl["sph_sample_fold_words"] == ["int", "constsph_slab_sample_words*", "sph_sample_params*", "char*", "uint64_t"]
    assert decl["sph_slab_sample_layer"] == [ctx, par, sp, "sph_sample_band*", "sph_sample_info*"]
    assert decl["sph_slab_sample_layer_download"] == [ctx, "int64_t*", "uint64_t"]
    assert decl["sph_sample_compose"] == [ctx, sp, "int", "constsph_sample_band*", "constint64_t*const*", "float*", "uint64_t", "int64_t*", "uint64_t"]
    assert decl["sph_group_sample_grid"] == ["sph_ctx**", "int", par, sp, "float*", "uint64_t", "int64_t*", "uint64_t", "sph_sample_info*"]


def test_ffi_signatures_agree_with_the_header(product_lib):
    """The argument count and the 64-bit / pointer positions of every ctypes signature."""
    decl = _declarations()
    for name in NAMES:
        fn = getattr(product_lib, name[4:])
        assert fn is not None and fn.restype is C.c_int32, name
        assert len(fn.argtypes) == len(decl[name]), name
        for t, d in zip(fn.argtypes, decl[name]):
            if d == "int":
                assert t is C.c_int32, (name, d)
            elif d == "uint64_t":
                assert t is C.c_uint64, (name, d)
            else:
                assert d.endswith("*") and C.sizeof(t) == C.sizeof(C.c_void_p), (name, d)


def test_struct_sizes_and_mirrors():
    code = _code()
    assert C.sizeof(ffi.SphSampleBand) == 16 and C.sizeof(ffi.SphSlabSampleWords) == 32
    band = re.search(r"typedef struct sph_sample_band \{(.*?)\}", code, re.S).group(1)
    assert re.search(r"int32_t\s+sx0, sx1;\s*uint32_t\s+n_boxes;\s*uint32_t\s+reserved;", band)
    assert [f[0] for f in ffi.SphSampleBand._fields_] == ["sx0", "sx1", "n_boxes", "reserved"]
    assert ffi.SphSampleBand.sx1.offset == 4 and ffi.SphSampleBand.n_boxes.offset == 8 and ffi.SphSampleBand.reserved.offset == 12
    words = re.search(r"typedef struct sph_slab_sample_words \{(.*?)\}", code, re.S).group(1)
    assert re.search(r"uint64_t\s+first_bad;\s*uint32_t\s+max_bits\[SPH_SAMPLE_MAX_CHANNELS\];", words)
    assert [f[0] for f in ffi.SphSlabSampleWords._fields_] == ["first_bad", "max_bits"]
    assert ffi.SphSlabSampleWords.max_bits.offset == 8 and ffi.SphSlabSampleWords.max_bits.size == 24
    assert ffi.SAMPLE_NO_OFFENDER == 2 ** 64 - 1
    w = ffi.SphSlabSampleWords.from_tuple((5 << 8 | 4, (1, 2, 3, 4, 5, 6)))
    assert w.as_tuple() == (5 << 8 | 4, (1, 2, 3, 4, 5, 6))


def test_sph_sample_h_points_to_the_new_header():
    text = (REPO / "include" / "sph_sample.h").read_text()
    assert "sph_slab_sample.h" in text and "not built yet" not in text
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        body = (REPO / doc).read_text()
        assert "sph_slab_sample.h" in body, doc
        assert not re.search(r"raw planes[^.]*not built yet", body), doc
