"""include/sph_ledger.h against the built product library and its ctypes mirror (no GPU needed: symbols, signatures and sizes only)."""
import ctypes as C
import re
from pathlib import Path

from adaptive_sph_amd import ffi, ledger
from tests import ledger_reference as lr

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "sph_ledger.h"
NAMES = ["sph_ledger_compute", "sph_slab_ledger_range", "sph_slab_ledger_sums", "sph_ledger_fold_words", "sph_ledger_compose", "sph_group_ledger"]
OTHERS = ("ABI_SYMBOLS", "RENDER_SYMBOLS", "CANDIDATE_SYMBOLS", "PROBLEM_SYMBOLS", "SEARCH_SYMBOLS", "SLAB_CANDIDATE_SYMBOLS", "SLAB_PROBLEM_SYMBOLS",
          "SLAB_SEARCH_SYMBOLS", "RANK_SEARCH_SYMBOLS", "SLAB_RENDER_SYMBOLS", "SAMPLE_SYMBOLS", "SLAB_SAMPLE_SYMBOLS")


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
    assert sorted("sph_" + s for s in ffi.LEDGER_SYMBOLS) == sorted(NAMES)
    for other in OTHERS:
        assert not set(ffi.LEDGER_SYMBOLS) & set(getattr(ffi, other)), other
    # sph_ffi.h stays what it was
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sph_ffi.h").read_text(), flags=re.S)
    assert {"sph_" + s for s in ffi.ABI_SYMBOLS} == set(re.findall(r"\b(sph_\w+)\s*\(", text))
    assert "ledger" not in text


def test_signatures_are_the_stated_ones():
    decl = _declarations()
    ctx, par, spec = "sph_ctx*", "constsph_params*", "constsph_ledger_spec*"
    assert decl["sph_ledger_compute"] == [ctx, par, spec, "sph_ledger_result*"]
    assert decl["sph_slab_ledger_range"] == [ctx, par, spec, "sph_ledger_words*"]
    assert decl["sph_slab_ledger_sums"] == [ctx, par, spec, "sph_ledger_sum*"]
    assert decl["sph_ledger_fold_words"] == ["int", "constsph_ledger_words*", "sph_ledger_spec*", "sph_ledger_words*", "char*", "uint64_t"]
    assert decl["sph_ledger_compose"] == ["int", "constsph_ledger_words*", "constsph_ledger_sum*", spec, "sph_ledger_result*"]
    assert decl["sph_group_ledger"] == ["sph_ctx**", "int", par, spec, "sph_ledger_result*"]


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
    assert (C.sizeof(ffi.SphLedgerSpec), C.sizeof(ffi.SphLedgerSum), C.sizeof(ffi.SphLedgerExtreme), C.sizeof(ffi.SphLedgerWords),
            C.sizeof(ffi.SphLedgerResult)) == (40, 16, 8, 200, 376)
    for name, size in (("spec", 40), ("sum", 16), ("extreme", 8), ("words", 200), ("result", 376)):
        assert re.search(r"\} sph_ledger_%s;\s*/\* %d bytes" % (name, size), HEADER.read_text()), name
    words = re.search(r"typedef struct sph_ledger_words \{(.*?)\}", code, re.S).group(1)
    assert re.search(r"uint64_t\s+first_bad;\s*uint64_t\s+n, n_outside;\s*uint64_t\s+max_bits\[SPH_LEDGER_N_SUMS\];\s*uint64_t\s+extreme\[SPH_LEDGER_N_EXTREMES\];",
                     words)
    assert [f[0] for f in ffi.SphLedgerWords._fields_] == ["first_bad", "n", "n_outside", "max_bits", "extreme"]
    assert (ffi.SphLedgerWords.max_bits.offset, ffi.SphLedgerWords.extreme.offset) == (24, 96)
    result = re.search(r"typedef struct sph_ledger_result \{(.*?)\}", code, re.S).group(1)
    assert [m for m in re.findall(r"\b(\w+)(?:\[\w+\])?;", result)] == ["what", "exponent", "n_outside", "raw", "sum", "extreme"]
    assert [f[0] for f in ffi.SphLedgerResult._fields_] == ["what", "exponent", "n", "n_outside", "raw", "sum", "extreme"]
    R = ffi.SphLedgerResult
    assert (R.exponent.offset, R.n.offset, R.n_outside.offset, R.raw.offset, R.sum.offset, R.extreme.offset) == (4, 40, 48, 56, 200, 272)
    w = ffi.SphLedgerWords.from_tuple((5 << 8 | 16, 7, 2, tuple(range(9)), tuple(range(100, 113))))
    assert w.as_tuple() == (5 << 8 | 16, 7, 2, tuple(range(9)), tuple(range(100, 113)))
    for q in (0, 1, -1, 2 ** 64, -2 ** 64 - 1, 2 ** 100 + 12345, -(2 ** 126)):
        assert ffi.SphLedgerSum.from_int(q).as_int() == q


def test_constants_and_names_agree():
    code = _code()

    def macro(name):
        return re.search(r"#define\s+%s\s+\(?(-?\w+)\)?" % name, code).group(1)

    assert (int(macro("SPH_LEDGER_N_SUMS")), int(macro("SPH_LEDGER_N_EXTREMES"))) == (ffi.LEDGER_N_SUMS, ffi.LEDGER_N_EXTREMES) == (lr.N_SUMS, lr.N_EXT) == (9, 13)
    assert (int(macro("SPH_LEDGER_MIN_EXPONENT")), int(macro("SPH_LEDGER_MAX_EXPONENT"))) == (ffi.LEDGER_MIN_EXPONENT, ffi.LEDGER_MAX_EXPONENT) == (-200, 200)
    assert int(macro("SPH_LEDGER_AUTO_EXPONENT"), 16) == ffi.LEDGER_AUTO_EXPONENT
    assert ffi.LEDGER_NO_OFFENDER == lr.NONE == 2 ** 64 - 1 and ffi.LEDGER_NO_ID == lr.NO_ID == 2 ** 32 - 1
    enums = re.findall(r"enum \{(.*?)\};", code, re.S)
    groups = dict(re.findall(r"SPH_LEDGER_(\w+) = (\d+)", enums[0]))
    assert {k.lower(): int(v) for k, v in groups.items()} == ffi.LEDGER_GROUPS == {"carried": lr.CARRIED, "step_outputs": lr.STEP, "outside": lr.OUTSIDE}
    assert [n.lower() for n in re.findall(r"SPH_LEDGER_(\w+)", enums[1])] == ffi.LEDGER_SUMS == lr.SUMS
    assert [n.lower() for n in re.findall(r"SPH_LEDGER_(\w+)", enums[2])] == ffi.LEDGER_EXTREMES == lr.EXTREMES
    assert all(lr.is_max(k) == name.startswith("max") for k, name in enumerate(lr.EXTREMES))
    assert ledger.CSV_COLUMNS[:4] == ["step", "time", "dt", "n"] and ledger.CSV_COLUMNS[4:13] == ffi.LEDGER_SUMS


def test_the_documents_describe_the_ledger():
    for doc in ("README.md", "DESIGN.md"):
        assert "sph_ledger.h" in (REPO / doc).read_text(), doc
    assert "9.4" in (REPO / "DESIGN.md").read_text()
    assert "--ledger" in (REPO / "README.md").read_text()
