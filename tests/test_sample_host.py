"""The host side of the field sampling (include/sph_sample.h) without a device: that the numpy twin (tests/sample_reference.py) has the
two properties the 64-bit integer sums are there for, that sampling.resolve states the resolved output, that the interpolant is a
partition of unity inside a lattice, and the bytes write_vtk_grid writes."""
import ctypes as C
import re
from pathlib import Path

import numpy as np

from adaptive_sph_amd import ffi, sampling
from adaptive_sph_amd.vtk_exporter import VtkGridExporter, write_vtk_grid
from tests import sample_reference as sr

REPO = Path(__file__).resolve().parent.parent
CH = ["density", "pressure", "velocity_x", "velocity_y", "level_estimation"]


def _cloud(n=1280, seed=5):
    """Particles of two sizes scattered over a 1.1 x 0.8 box, with fields of both signs and a few FluidInterior levels."""
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 2)) * (1.1, 0.8) + (-0.05, -0.02)).astype(np.float32)
    h = np.where(rng.random(n) < 0.3, 0.06, 0.025).astype(np.float32)
    mass = (h * h * 0.27).astype(np.float32)
    lvl = (rng.random(n) * -0.2).astype(np.float32)
    lvl[rng.random(n) < 0.2] = np.nan
    return {"position": pos, "h2": h, "mass": mass, "density": (0.9 + 0.2 * rng.random(n)).astype(np.float32),
            "pressure": (rng.random(n) * 300).astype(np.float32), "velocity": ((rng.random((n, 2)) - 0.5) * 7).astype(np.float32),
            "level_estimation": lvl}


def _take(fields, idx):
    return {k: v[idx] for k, v in fields.items()}


GRID = dict(nx=64, ny=48, origin=(-0.08, -0.03), spacing=0.018)


def test_twin_is_permutation_invariant():
    f = _cloud()
    raw, exps, touching, foot = sr.sample(f, CH, 1.0, 0.2, **GRID)
    assert touching > 1000 and foot[0] > 30 and foot[1] > 10 * touching and np.count_nonzero(raw[0]) > 2000
    assert (raw[3] < 0).any() and (raw[3] > 0).any()            # velocity of both signs
    perm = np.random.default_rng(1).permutation(len(f["mass"]))
    raw2, exps2, touching2, foot2 = sr.sample(_take(f, perm), CH, 1.0, 0.2, **GRID)
    assert exps == exps2 and (touching, foot) == (touching2, foot2)
    assert np.array_equal(raw, raw2)


def test_twin_raw_planes_of_disjoint_sets_add_exactly():
    f = _cloud()
    n = len(f["mass"])
    _, exps, _, _ = sr.sample(f, CH, 1.0, 0.2, **GRID)
    whole = sr.sample(f, CH, 1.0, 0.2, exps=exps, **GRID)[0]
    part_a = np.flatnonzero(f["position"][:, 0] < 0.4)
    part_b = np.setdiff1d(np.arange(n), part_a)
    a = sr.sample(_take(f, part_a), CH, 1.0, 0.2, exps=exps, **GRID)[0]
    b = sr.sample(_take(f, part_b), CH, 1.0, 0.2, exps=exps, **GRID)[0]
    assert np.count_nonzero(a[0]) and np.count_nonzero(b[0]) and np.count_nonzero((a[0] != 0) & (b[0] != 0))   # the parts overlap
    assert np.array_equal(a + b, whole)


def test_twin_window_equals_the_whole_grid_there():
    f = _cloud()
    p = sr.Particles(f, CH, 1.0, 0.2)
    exps = sr.exponents(p)
    whole = sr.sample(f, CH, 1.0, 0.2, **GRID)[0]
    for win in [(0, 16, 0, 16), (24, 40, 16, 32), (48, 64, 20, 36)]:
        got = sr.window_planes(p, exps, GRID["nx"], GRID["ny"], GRID["origin"], GRID["spacing"], win)
        assert np.array_equal(got, whole[:, win[2]:win[3], win[0]:win[1]]), win


def test_twin_exponents_and_preconditions():
    assert [sr.exponent_of(m) for m in (0.0, 0.5, 0.75, 1.0, 7.9, 8.0, 2.0 ** -70)] == [0, 0, 0, 1, 3, 4, -69]
    f = _cloud(64)
    p = sr.Particles(f, ["pressure", "velocity_x"], 1.0)
    assert sr.first_offender(p) is None
    e = sr.exponents(p)
    assert all(np.abs(p.a[c]).max() < 2.0 ** e[c] and np.abs(p.a[c]).max() >= 2.0 ** (e[c] - 1) for c in range(2))
    too_small = [e[0] - 1, None]
    i, why = sr.first_offender(p, too_small)
    assert why == sr.BAD_CHANNEL and i == int(np.flatnonzero(np.abs(p.a[0]) >= 2.0 ** (e[0] - 1))[0])
    f["velocity"][40, 0] = np.inf
    f["h2"][50] = 0.0
    assert sr.first_offender(sr.Particles(f, ["pressure", "velocity_x"], 1.0)) == (40, sr.BAD_CHANNEL + 1)
    f["h2"][7] = 0.0
    assert sr.first_offender(sr.Particles(f, ["pressure", "velocity_x"], 1.0)) == (7, sr.BAD_H)


def test_resolve_on_hand_made_planes():
    one = 1 << 32
    raw = np.zeros((3, 2, 3), np.int64)
    raw[0] = [[one, one // 2, one // 2 - 256], [0, 3 * one, one // 4]]          # weights 1, 0.5, 0.5 - 2^-24 | 0, 3, 0.25
    raw[1] = [[5 * one, -one, one], [7, -9 * one, one]]                       # exponent 3: x 2^-29
    raw[2] = [[-one, one, one], [0, 6 * one, -one]]                           # exponent -2: x 2^-34
    plain = sampling.resolve(raw, [3, -2])
    assert plain.dtype == np.float32 and plain.shape == raw.shape
    assert np.array_equal(plain[0], np.array([[1, 0.5, (one // 2 - 256) / one], [0, 3, 0.25]], np.float32))
    assert np.array_equal(plain[1], np.array([[40, -8, 8], [7 * 2.0 ** -29, -72, 8]], np.float32))
    assert np.array_equal(plain[2], np.array([[-0.25, 0.25, 0.25], [0, 1.5, -0.25]], np.float32))
    norm = sampling.resolve(raw, [3, -2], normalize=True, min_weight=0.5, fill=float("nan"))
    assert np.array_equal(norm[0], plain[0])                                   # the weight plane is never normalised
    keep = np.array([[True, True, False], [False, True, False]])
    assert np.array_equal(np.isnan(norm[1]), ~keep) and np.array_equal(np.isnan(norm[2]), ~keep)
    assert np.array_equal(norm[1][keep], np.array([40, -16, -24], np.float32))
    assert np.array_equal(norm[2][keep], np.array([-0.25, 0.5, 0.5], np.float32))
    filled = sampling.resolve(raw, [3, -2], normalize=True, min_weight=0.2, fill=-1.0)
    assert np.array_equal(filled[1], np.array([[40, -16, np.float32(8) / plain[0, 0, 2]], [-1, -24, 32]], np.float32))
    # one rounding from the f64 product to f32, as the device does it: 2^32 + 1 sums resolve to 1, not to 1 + 2^-32
    assert sampling.resolve(np.full((1, 1, 1), one + 1, np.int64), [])[0, 0, 0] == np.float32(1.0)


def test_partition_of_unity_inside_a_lattice():
    """A 40 x 32 square lattice of spacing 1/40 at fill 0.93 with h from the mass, V = m / rest_density: every sample farther than 2h
    inside the lattice sees the weight 0.93 within 0.01.  (Measured on this twin: 0.9269 .. 0.9343; the bar is about twice that spread.)"""
    s, fill = np.float32(1.0 / 40), np.float32(0.93)
    ix, iy = np.meshgrid(np.arange(40), np.arange(32), indexing="ij")
    pos = np.stack([ix.ravel() * s, iy.ravel() * s], 1).astype(np.float32)
    mass = np.full(len(pos), s * s * fill, np.float32)
    h = (np.float32(1.9) * np.sqrt(mass * np.float32(0.318309873342514038086))).astype(np.float32)   # local_smoothing_length_from_mass
    f = {"position": pos, "mass": mass, "h2": h, "density": np.ones(len(pos), np.float32)}
    nx, ny, origin, spacing = 64, 48, (-0.05, -0.03), 0.018
    raw, _, touching, _ = sr.sample(f, [], 1.0, 0.0, nx, ny, origin, spacing, volume="rest")
    weight = sampling.resolve(raw, [])[0]
    X, Y = sr.centers(nx, ny, origin, spacing)
    R = 2 * float(h[0])
    inside = ((X > R) & (X < 39 * float(s) - R))[None, :] & ((Y > R) & (Y < 31 * float(s) - R))[:, None]
    assert inside.sum() > 1000 and touching == len(pos)
    assert np.abs(weight[inside] - 0.93).max() < 0.01, (weight[inside].min(), weight[inside].max())
    assert weight[~inside].min() == 0.0                                        # (the grid overhangs the lattice)


def test_grid_spec():
    from adaptive_sph_amd.scene import SceneBoundary
    g = sampling.GridSpec.covering(SceneBoundary("box", 2.0, 1.0), 0.25)
    assert (g.nx, g.ny, g.origin, g.spacing) == (8, 4, (-1.0, -0.5), 0.25)
    g = sampling.GridSpec.covering(SceneBoundary("box", 2.0, 1.0), 0.3, margin=0.1)
    assert (g.nx, g.ny) == (8, 4) and np.allclose(g.origin, (-1.1, -0.6))
    X, Y = g.centers()
    Xr, Yr = sr.centers(g.nx, g.ny, g.origin, g.spacing)
    assert X.dtype == np.float32 and np.array_equal(X, Xr) and np.array_equal(Y, Yr)
    assert sampling.expand_channels(["density", "velocity", "level"]) == ["density", "velocity_x", "velocity_y", "level_estimation"]


def test_symbols_and_structs_match_the_header():
    header = (REPO / "include" / "sph_sample.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(sph_sample_[a-z_]+)\s*\(", code))) == sorted("sph_" + s for s in ffi.SAMPLE_SYMBOLS)
    assert ffi.SAMPLE_SYMBOLS == ["sample_grid", "sample_field_range"]
    assert not set(ffi.SAMPLE_SYMBOLS) & set(ffi.ABI_SYMBOLS)
    ffi_header = (REPO / "include" / "sph_ffi.h").read_text()
    assert "sph_sample" not in ffi_header and "sph_sample" not in (REPO / "rust_shim" / "src" / "lib.rs").read_text()
    for name, value in [("SPH_SAMPLE_MAX_CHANNELS", ffi.SAMPLE_MAX_CHANNELS), ("SPH_SAMPLE_MAX_SIDE", ffi.SAMPLE_MAX_SIDE),
                        ("SPH_SAMPLE_MAX_EXPONENT", ffi.SAMPLE_MAX_EXPONENT)]:
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert "#define SPH_SAMPLE_MIN_EXPONENT (-64)" in header and ffi.SAMPLE_MIN_EXPONENT == -64
    assert "#define SPH_SAMPLE_AUTO_EXPONENT 0x7fffffff" in header and ffi.SAMPLE_AUTO_EXPONENT == 0x7FFFFFFF
    assert re.search(r"SPH_SAMPLE_VOLUME_DENSITY = 0, SPH_SAMPLE_VOLUME_REST = 1", header) and ffi.SAMPLE_VOLUMES == {"density": 0, "rest": 1}
    assert C.sizeof(ffi.SphSampleChannel) == 12
    assert C.sizeof(ffi.SphSampleParams) == 10 * 4 + 6 * 12
    assert C.sizeof(ffi.SphSampleInfo) == 6 * 4 + 3 * 8
    for field, _ in ffi.SAMPLE_CHANNELS.values():
        assert field in ffi.FIELDS


def test_product_library_exports_the_sampling_symbols(product_lib):
    for s in ffi.SAMPLE_SYMBOLS:
        assert hasattr(product_lib.lib, "sph_" + s) and getattr(product_lib, s) is not None


def test_write_vtk_grid_bytes(tmp_path):
    grid = sampling.GridSpec(5, 3, (-1.0, 2.0), 0.5)
    rng = np.random.default_rng(3)
    planes = {k: rng.standard_normal((3, 5)).astype(np.float32) for k in ("weight", "density", "velocity_x", "velocity_y", "level_estimation")}
    path = tmp_path / "g.vtk"
    write_vtk_grid(path, grid, planes)
    blob = path.read_bytes()
    pos = 0

    def line():
        nonlocal pos
        end = blob.index(b"\n", pos)
        out = blob[pos:end].decode()
        pos = end + 1
        return out

    def payload(count):
        nonlocal pos
        a = np.frombuffer(blob, ">f4", count, pos)
        pos += 4 * count
        assert blob[pos:pos + 1] == b"\n"
        pos += 1
        return a

    assert [line() for _ in range(4)] == ["# vtk DataFile Version 4.2", "SPH grid 1.0", "BINARY", "DATASET STRUCTURED_POINTS"]
    assert line() == "DIMENSIONS 5 3 1"
    assert [float(v) for v in line().split()[1:]] == [-0.75, 2.25, 0.0]        # ORIGIN: the centre of sample (0, 0)
    assert line() == "SPACING 0.5 0.5 1.0"
    assert line() == "POINT_DATA 15"
    for name in ("weight", "density"):
        assert line() == f"SCALARS {name} float 1" and line() == "LOOKUP_TABLE default"
        assert np.array_equal(payload(15), planes[name].ravel())               # x fastest, row 0 (the lowest y) first, big-endian
    assert line() == "VECTORS velocity float"
    v = payload(45).reshape(15, 3)
    assert np.array_equal(v[:, 0], planes["velocity_x"].ravel()) and np.array_equal(v[:, 1], planes["velocity_y"].ravel()) and not v[:, 2].any()
    assert line() == "SCALARS level_estimation float 1" and line() == "LOOKUP_TABLE default"
    assert np.array_equal(payload(15), planes["level_estimation"].ravel())
    assert pos == len(blob)


def test_vtk_grid_exporter_series(tmp_path):
    import json
    grid = sampling.GridSpec(2, 2, (0.0, 0.0), 1.0)
    with VtkGridExporter(tmp_path / "out", "my-sph-grid") as ex:
        ex.add_snapshot(0.5, grid, {"weight": np.ones((2, 2), np.float32)})
        ex.add_snapshot(1.0, grid, {"weight": np.zeros((2, 2), np.float32)})
    series = json.loads((tmp_path / "out" / "my-sph-grid.vtk.series").read_text())
    assert series["files"] == [{"name": "my-sph-grid-00001.vtk", "time": 0.5}, {"name": "my-sph-grid-00002.vtk", "time": 1.0}]
    assert (tmp_path / "out" / "my-sph-grid-00002.vtk").exists()


def test_series_names_only_files_that_exist(tmp_path):
    """The index entry of a snapshot is written behind its file: a writer that raises leaves no entry."""
    import json
    import pytest
    grid = sampling.GridSpec(2, 2, (0.0, 0.0), 1.0)
    with VtkGridExporter(tmp_path, "g") as ex:
        ex.add_snapshot(0.5, grid, {"weight": np.ones((2, 2), np.float32)})
        with pytest.raises(ValueError):
            ex.add_snapshot(1.0, grid, {"weight": np.ones((3, 2), np.float32)})      # not the grid's shape
        ex.add_snapshot(1.5, grid, {"weight": np.zeros((2, 2), np.float32)})
    files = json.loads((tmp_path / "g.vtk.series").read_text())["files"]
    assert files == [{"name": "g-00001.vtk", "time": 0.5}, {"name": "g-00002.vtk", "time": 1.5}]
    assert all((tmp_path / f["name"]).exists() for f in files)


def test_grid_options_are_checked_when_parsed():
    import pytest
    from adaptive_sph_amd.__main__ import build_parser
    a = build_parser().parse_args(["run", "c.yaml", "s.yaml", "--grid-vtk", "out", "--grid-spacing", "0.01", "--grid-fields", "density,level"])
    assert (a.grid_vtk, a.grid_spacing, a.grid_fields) == ("out", 0.01, "density,level")
    a = build_parser().parse_args(["run", "c.yaml", "s.yaml"])
    assert (a.grid_vtk, a.grid_spacing, a.grid_fields) == (None, None, "density,pressure,velocity")
    for bad in ("0", "-0.1", "nan", "inf"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["run", "c.yaml", "s.yaml", "--grid-vtk", "out", "--grid-spacing", bad])
