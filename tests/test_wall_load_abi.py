"""include/sph_wall_load.h against the built product library, its ctypes mirror and the twin (no GPU needed: symbols, signatures, sizes and
offsets only)."""
import ctypes as C
import re
from pathlib import Path

from adaptive_sph_amd import ffi, wall_loads
from tests import wall_load_reference as wr

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "sph_wall_load.h"


def _code():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def _declarations():
    """name -> the parameter types of its declaration, spaces removed"""
    out = {}
    for name, args in re.findall(r"\bint\s+(sph_\w+)\s*\(([^)]*)\)\s*;", _code()):
        out[name] = [re.sub(r"\s*\b\w+$", "", a.strip()).replace(" ", "") for a in args.split(",")]
    return out


def test_library_exports_the_declared_function(product_lib):
    decl = _declarations()
    assert sorted(decl) == ["sph_wall_load_compute"] == sorted("sph_" + s for s in ffi.WALL_LOAD_SYMBOLS)
    assert decl["sph_wall_load_compute"] == ["sph_ctx*", "constsph_params*", "constsph_wall_load_spec*", "sph_wall_load_result*", "int64_t*"]
    assert hasattr(C.CDLL(str(ffi.PRODUCT_LIB)), "sph_wall_load_compute")
    fn = product_lib.wall_load_compute
    assert fn is not None and fn.restype is C.c_int32 and len(fn.argtypes) == 5
    assert all(C.sizeof(t) == C.sizeof(C.c_void_p) for t in fn.argtypes)
    for other in (k for k in dir(ffi) if k.endswith("_SYMBOLS") and k != "WALL_LOAD_SYMBOLS"):
        assert not set(ffi.WALL_LOAD_SYMBOLS) & set(getattr(ffi, other)), other
    # sph_ffi.h stays what it was
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sph_ffi.h").read_text(), flags=re.S)
    assert "wall_load" not in text


def test_struct_sizes_and_offsets():
    text = HEADER.read_text()
    sizes = {"spec": (ffi.SphWallLoadSpec, 232), "element_words": (ffi.SphWallLoadElementWords, 64), "words": (ffi.SphWallLoadWords, 528),
             "element": (ffi.SphWallLoadElement, 152), "result": (ffi.SphWallLoadResult, 1232)}
    for name, (cls, size) in sizes.items():
        assert C.sizeof(cls) == size, name
        assert re.search(r"\} sph_wall_load_%s;\s*/\* %d bytes" % (name, size), text), name
    S, W, E, R = ffi.SphWallLoadSpec, ffi.SphWallLoadWords, ffi.SphWallLoadElement, ffi.SphWallLoadResult
    assert (S.flags.offset, S.bins.offset, S.exponent.offset, S.n_bins.offset, S.s_lo.offset, S.s_hi.offset) == (0, 4, 8, 136, 168, 200)
    assert (W.first_bad.offset, W.n.offset, W.element.offset) == (0, 8, 16)
    EW = ffi.SphWallLoadElementWords
    assert (EW.n_entries.offset, EW.n_wet.offset, EW.n_unbinned.offset, EW.max_bits.offset, EW.max_pressure.offset) == (0, 8, 16, 24, 56)
    assert (E.exponent.offset, E.raw.offset, E.sum.offset, E.n_entries.offset, E.n_wet.offset, E.n_unbinned.offset, E.max_pressure.offset, E.inv_ds.offset,
            E.n_bins.offset) == (0, 16, 80, 112, 120, 128, 136, 144, 148)
    assert (R.n_elements.offset, R.bins.offset, R.n.offset, R.element.offset) == (0, 4, 8, 16)
    # the field names and their order are the header's
    code = _code()
    for name, (cls, _) in sizes.items():
        body = re.search(r"typedef struct sph_wall_load_%s \{(.*?)\}" % name, code, re.S).group(1)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\w+\])*\s*(?:,|$)", decl.strip())]
        assert names == [f[0] for f in cls._fields_], name


def test_constants_and_names_agree():
    code = _code()

    def macro(name):
        return int(re.search(r"#define\s+%s\s+\(?(-?\w+)\)?" % name, code).group(1))

    assert macro("SPH_WALL_LOAD_MAX_ELEMENTS") == ffi.WALL_LOAD_MAX_ELEMENTS == wr.MAX_ELEMENTS == 8
    assert macro("SPH_WALL_LOAD_N_SUMS") == ffi.WALL_LOAD_N_SUMS == wr.N_SUMS == 4
    assert macro("SPH_WALL_LOAD_MAX_BINS") == ffi.WALL_LOAD_MAX_BINS == wr.MAX_BINS == 4096
    assert macro("SPH_WALL_LOAD_MAX_BINNED_ENTRIES") == ffi.WALL_LOAD_MAX_BINNED_ENTRIES == wr.MAX_BINNED == 2 ** 23
    assert macro("SPH_WALL_LOAD_BIN_SHIFT") == ffi.WALL_LOAD_BIN_SHIFT == wr.BIN_SHIFT == 40
    enum = re.search(r"enum \{(.*?)\};", code, re.S).group(1)
    assert [n.lower() for n in re.findall(r"SPH_WALL_LOAD_(\w+)", enum)] == ffi.WALL_LOAD_SUMS == wr.SUMS
    assert wall_loads.csv_columns(2) == ["step", "time", "dt"] + [f"{c}_{k}" for k in (0, 1) for c in ("fx", "fy", "torque", "normal", "n_wet", "peak_p", "peak_id")]


def test_spec_builder_and_ranges():
    spec = wall_loads.wall_load_spec(16, [None, (-1.0, 1.0), (-2.0, 2.0, 4)], [None, [3, None, -7, None]])
    assert spec.flags == 0 and spec.bins == 16 and list(spec.n_bins) == [0, 16, 4, 0, 0, 0, 0, 0]
    assert (spec.s_lo[1], spec.s_hi[1], spec.s_lo[2], spec.s_hi[2]) == (-1.0, 1.0, -2.0, 2.0)
    assert list(spec.exponent[0]) == [ffi.LEDGER_AUTO_EXPONENT] * 4 and list(spec.exponent[1]) == [3, ffi.LEDGER_AUTO_EXPONENT, -7, ffi.LEDGER_AUTO_EXPONENT]
    from adaptive_sph_amd import scene as sc
    box = sc.SceneBoundary("box", 4.0, 2.0)
    assert wall_loads.plane_ranges(sc.boundary_planes(box), box) == [(-1.0, 1.0), (-1.0, 1.0), (-2.0, 2.0), (-2.0, 2.0)]


def test_the_documents_describe_the_wall_loads():
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "sph_wall_load.h" in (REPO / doc).read_text(), doc
    assert "9.7" in (REPO / "DESIGN.md").read_text()
    assert "--wall-loads" in (REPO / "README.md").read_text()
