"""include/sph_slab_partner_search.h against the built libraries and its ctypes mirror (no GPU needed: symbols and tables only)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from adaptive_sph_amd import distributed as D, ffi
from adaptive_sph_amd.workloads import default_params

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "sph_slab_partner_search.h"


def _declared(header: Path):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return re.findall(r"\bint\s+(sph_\w+)\s*\(", text)


def test_the_header_declares_the_optional_table():
    names = _declared(HEADER)
    assert len(names) == len(set(names)) == 4
    assert sorted(names) == sorted("sph_" + s for s in ffi.SLAB_SEARCH_SYMBOLS)


def test_product_exports_them_and_the_oracle_does_not(product_lib, oracle_lib):
    for n in _declared(HEADER):
        assert hasattr(product_lib.lib, n), n
    for s in ffi.SLAB_SEARCH_SYMBOLS:
        assert getattr(product_lib, s) is not None, s                      # the optional table is bound
        assert getattr(oracle_lib, s) is None, s
        assert not any(hasattr(oracle_lib.lib, prefix + s) for prefix in ("sph_", "oracle_")), s


def test_the_table_is_disjoint_from_every_other_one():
    others = {"ABI_SYMBOLS": ffi.ABI_SYMBOLS, "RENDER_SYMBOLS": ffi.RENDER_SYMBOLS, "CANDIDATE_SYMBOLS": ffi.CANDIDATE_SYMBOLS, "PROBLEM_SYMBOLS": ffi.PROBLEM_SYMBOLS,
              "SEARCH_SYMBOLS": ffi.SEARCH_SYMBOLS, "SLAB_CANDIDATE_SYMBOLS": ffi.SLAB_CANDIDATE_SYMBOLS, "SLAB_PROBLEM_SYMBOLS": ffi.SLAB_PROBLEM_SYMBOLS,
              "SLAB_RENDER_SYMBOLS": ffi.SLAB_RENDER_SYMBOLS}
    for name, table in others.items():
        assert not set(ffi.SLAB_SEARCH_SYMBOLS) & set(table), name
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sph_ffi.h").read_text(), flags=re.S)
    assert {"sph_" + s for s in ffi.ABI_SYMBOLS} == set(re.findall(r"\b(sph_\w+)\s*\(", text))   # sph_ffi.h stays what it was


def test_the_group_form_alone_takes_the_device_mode():
    assert D.SLAB_EXPORTS == ("lists", "candidates", "compact")
    assert D.GROUP_SLAB_EXPORTS == D.SLAB_EXPORTS + ("device",)
    assert "device" in D.GROUP_SLAB_EXPORTS and "device" not in D.SLAB_EXPORTS


def test_the_info_struct_is_the_plain_search_s():
    assert C.sizeof(ffi.SphPartnerSearchInfo) == D.C_INFO_BYTES == 48


def test_the_rank_driver_refuses_the_mode_and_names_the_group_form():
    with pytest.raises(ValueError, match="group_single_step_adaptivity_on_slabs"):
        D.rank_single_step_adaptivity_on_slabs(None, default_params(), 1e-3, 1, export="device")
    with pytest.raises(ValueError, match="export must be one of"):
        D.group_single_step_adaptivity_on_slabs(None, [], default_params(), 1e-3, 1, export="nothing")
