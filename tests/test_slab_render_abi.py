"""include/sph_slab_render.h against the built product library and its ctypes mirror (no GPU needed: symbols and sizes only)."""
import ctypes as C
import re
from pathlib import Path

from adaptive_sph_amd import ffi

REPO = Path(__file__).resolve().parent.parent


def _declared(header: Path):
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    return re.findall(r"\bint\s+(sph_\w+)\s*\(", text)


def test_library_exports_every_declared_function():
    names = _declared(REPO / "include" / "sph_slab_render.h")
    assert sorted(names) == sorted("sph_" + s if not s.startswith("sph_") else s for s in
                                   ("slab_render_pressure_max", "slab_render_layer", "slab_render_layer_download", "render_compose", "group_render"))
    lib = C.CDLL(str(ffi.PRODUCT_LIB))
    for n in names:
        assert hasattr(lib, n), n
    assert sorted("sph_" + s for s in ffi.SLAB_RENDER_SYMBOLS) == sorted(names)


def test_band_is_16_bytes():
    assert C.sizeof(ffi.SphRenderBand) == 16
    assert [f[0] for f in ffi.SphRenderBand._fields_] == ["sx0", "sx1", "n_drawn", "reserved"]
    assert ffi.SphRenderBand.sx1.offset == 4 and ffi.SphRenderBand.n_drawn.offset == 8


def test_abi_symbols_are_those_of_sph_ffi_h():
    """The slab renderer lives in the optional, product-only table: ABI_SYMBOLS stays what sph_ffi.h declares."""
    text = re.sub(r"/\*.*?\*/", "", (REPO / "include" / "sph_ffi.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(sph_\w+)\s*\(", text))
    assert {"sph_" + s for s in ffi.ABI_SYMBOLS} == declared
    assert not set(ffi.SLAB_RENDER_SYMBOLS) & set(ffi.ABI_SYMBOLS)
