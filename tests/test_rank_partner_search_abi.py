"""include/sph_rank_partner_search.h against the built libraries and its ctypes mirror (no GPU needed: symbols, tables, structs and the
refusals that come before a context is looked at)."""
import ctypes as C
import re
from pathlib import Path

import pytest

from adaptive_sph_amd import distributed as D, ffi
from adaptive_sph_amd.workloads import default_params

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "sph_rank_partner_search.h"
OTHERS = ("ABI_SYMBOLS", "RENDER_SYMBOLS", "CANDIDATE_SYMBOLS", "PROBLEM_SYMBOLS", "SEARCH_SYMBOLS", "SLAB_CANDIDATE_SYMBOLS", "SLAB_PROBLEM_SYMBOLS",
          "SLAB_SEARCH_SYMBOLS", "SLAB_RENDER_SYMBOLS")


def _declared(header: Path):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return re.findall(r"\bint\s+(sph_\w+)\s*\(", text)


def test_the_header_declares_the_optional_table():
    names = _declared(HEADER)
    assert len(names) == len(set(names)) == len(ffi.RANK_SEARCH_SYMBOLS)
    assert sorted(names) == sorted("sph_" + s for s in ffi.RANK_SEARCH_SYMBOLS)
    for s in ("slab_find_partners_device", "slab_adapt_device", "slab_download_partner_decisions", "slab_download_merged_partner_problem", "relay_plan"):
        assert s in ffi.RANK_SEARCH_SYMBOLS, s


def test_product_exports_them_and_the_oracle_does_not(product_lib, oracle_lib):
    for n in _declared(HEADER):
        assert hasattr(product_lib.lib, n), n
    for s in ffi.RANK_SEARCH_SYMBOLS:
        assert getattr(product_lib, s) is not None, s                      # the optional table is bound
        assert getattr(oracle_lib, s) is None, s
        assert not any(hasattr(oracle_lib.lib, prefix + s) for prefix in ("sph_", "oracle_")), s
    with pytest.raises(ffi.SphError) as e:
        ffi.relay_plan(oracle_lib, 2, 0, 0, [16, 16], 4096)
    assert e.value.status == 30


def test_the_table_is_disjoint_from_every_other_one():
    for name in OTHERS:
        assert not set(ffi.RANK_SEARCH_SYMBOLS) & set(getattr(ffi, name)), name


def test_the_other_headers_stay_what_they_were():
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sph_ffi.h").read_text(), flags=re.S)
    assert {"sph_" + s for s in ffi.ABI_SYMBOLS} == set(re.findall(r"\b(sph_\w+)\s*\(", text))
    assert sorted(_declared(REPO / "include" / "sph_slab_partner_search.h")) == sorted("sph_" + s for s in ffi.SLAB_SEARCH_SYMBOLS)
    assert len(ffi.SLAB_SEARCH_SYMBOLS) == 4
    for other in ("sph_ffi.h", "sph_slab_partner_search.h", "sph_slab_partner_problem.h", "sph_partner_search.h"):
        assert not set(_declared(REPO / "include" / other)) & set(_declared(HEADER)), other


def test_the_structs_mirror_the_header():
    assert C.sizeof(ffi.SphRelayLeg) == 24 and C.sizeof(ffi.SphRelayStep) == 8 + 4 * 24
    assert ffi.SphRelayStep.send.offset == 8 and ffi.SphRelayStep.recv.offset == 8 + 48
    assert C.sizeof(ffi.SphPartnerSearchInfo) == D.C_INFO_BYTES == 48 < ffi.RANK_HEADER_BYTES


def test_the_plan_refuses_bad_arguments_without_a_device(product_lib):
    n = C.c_uint64(7)
    sizes = (C.c_uint64 * 2)(32, 32)
    plan = product_lib.relay_plan
    assert plan(2, 0, 0, 0, sizes, 4096, None, 0, C.byref(n)) == 0 and n.value == 1
    for args in ((0, 0, 0), (2, 2, 0), (2, -1, 0), (2, 0, 2), (2, 0, -1)):
        assert plan(*args, 0, sizes, 4096, None, 0, C.byref(n)) == 1, args
        assert n.value == 0
    assert plan(2, 0, 0, 0, None, 4096, None, 0, C.byref(n)) == 1
    assert plan(2, 0, 0, 0, sizes, 0, None, 0, C.byref(n)) == 1
    assert plan(2, 0, 0, 0, sizes, 4096, None, 0, None) == 1
    steps = (ffi.SphRelayStep * 1)()
    sizes[1] = 3 * 4096 + 1
    assert plan(2, 0, 0, 0, sizes, 4096, steps, 1, C.byref(n)) == 1 and n.value == 4            # the count is set when the capacity is refused


def test_the_null_context_is_refused(product_lib):
    p = default_params().to_ffi()
    info = ffi.SphPartnerSearchInfo()
    assert product_lib.slab_find_partners_device(None, 0, C.byref(p), None, 0, 0, 0, C.byref(info), None, None, None) == 1
    assert product_lib.slab_adapt_device(None, 0, C.byref(p), None) == 1
    assert product_lib.slab_download_partner_decisions(None, 0, None, None, None) == 1
    assert product_lib.slab_download_merged_partner_problem(None, None, None, None, None, None, None, None, 0, None, 0, None, None) == 1
    assert product_lib.slab_relay_sizes(None, None, 0, None, None, None, None, None, None) == 1


def test_the_rank_driver_still_refuses_the_mode_and_names_both_forms():
    assert D.SLAB_EXPORTS == ("lists", "candidates", "compact") and D.GROUP_SLAB_EXPORTS == D.SLAB_EXPORTS + ("device",)
    with pytest.raises(ValueError, match="group_single_step_adaptivity_on_slabs") as e:
        D.rank_single_step_adaptivity_on_slabs(None, default_params(), 1e-3, 1, export="device")
    assert "rank_single_step_adaptivity_on_slabs_device" in str(e.value)
    with pytest.raises(ValueError, match="FromMass"):
        D.rank_single_step_adaptivity_on_slabs_device(None, default_params(support_length_estimation="FromDistribution"), 1e-3, 1)
