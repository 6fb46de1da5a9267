"""include/sph_probe.h against the built product library and its ctypes mirror, the numpy twin of the probe sums against the lattice
twin, and the host helpers of adaptive_sph_amd/probes.py (no GPU needed)."""
import ctypes as C
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import ffi, probes
from adaptive_sph_amd.vtk_exporter import VtkPointsExporter, write_vtk_points
from tests import probe_reference as pr
from tests import sample_reference as sr

REPO = Path(__file__).resolve().parent.parent
HEADER = REPO / "include" / "sph_probe.h"
NAMES = ["sph_probe_set_create", "sph_probe_set_upload", "sph_probe_set_download", "sph_probe_set_size", "sph_probe_set_bins", "sph_probe_set_destroy",
         "sph_probe_sample", "sph_probe_advect"]


def _code():
    return re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)


def test_library_exports_the_eight_declared_functions():
    declared = re.findall(r"\bint\s+(sph_\w+)\s*\(", _code())
    assert sorted(declared) == sorted(NAMES)
    lib = C.CDLL(str(ffi.PRODUCT_LIB))
    for n in NAMES:
        assert hasattr(lib, n), n
    assert sorted("sph_" + s for s in ffi.PROBE_SYMBOLS) == sorted(NAMES)
    for other in ("ABI_SYMBOLS", "SAMPLE_SYMBOLS", "SLAB_SAMPLE_SYMBOLS", "LEDGER_SYMBOLS", "RENDER_SYMBOLS"):
        assert not set(ffi.PROBE_SYMBOLS) & set(getattr(ffi, other)), other
    # sph_ffi.h and sph_sample.h stay what they were
    for name in ("sph_ffi.h", "sph_sample.h"):
        assert "probe" not in (REPO / "include" / name).read_text()


def test_struct_sizes_equal_the_headers():
    pinned = dict(re.findall(r"SPH_PROBE_STATIC_ASSERT\(sizeof\((\w+)\) == (\d+)", _code()))
    assert pinned == {"sph_probe_params": "92", "sph_probe_advect_params": "20", "sph_probe_info": "80"}
    assert (C.sizeof(ffi.SphProbeParams), C.sizeof(ffi.SphProbeAdvectParams), C.sizeof(ffi.SphProbeInfo)) == (92, 20, 80)
    assert ffi.SphProbeInfo.cell_size.offset == 64 and ffi.SphProbeInfo.n_moved.offset == 48 and ffi.SphProbeParams.channels.offset == 20
    assert (ffi.PROBE_MAX_POINTS, ffi.PROBE_MAX_CELLS) == (1 << 24, 1 << 22)
    code = _code()
    assert "#define SPH_PROBE_MAX_POINTS (1ull << 24)" in code and "#define SPH_PROBE_MAX_CELLS (1u << 22)" in code
    gcc = shutil.which("gcc")
    if gcc:   # the header's own assertions, by a C compiler
        r = subprocess.run([gcc, "-std=c11", "-fsyntax-only", "-I", str(REPO / "include"), "-x", "c", str(HEADER)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def _synthetic(n=300, seed=5):
    rng = np.random.default_rng(seed)
    fine = np.arange(n) < 2 * n // 3
    pos = np.where(fine[:, None], rng.uniform([-0.5, -0.4], [0.1, 0.2], (n, 2)), rng.uniform([0.0, -0.4], [0.9, 0.5], (n, 2))).astype(np.float32)
    h = np.where(fine, 0.03, 0.075).astype(np.float32) * rng.uniform(0.9, 1.1, n).astype(np.float32)
    lvl = rng.uniform(-0.2, 0.05, n).astype(np.float32)
    lvl[::7] = np.nan
    fields = {"position": pos, "h2": h, "mass": (1000.0 * (h / 1.2) ** 2).astype(np.float32),
              "density": rng.uniform(950, 1050, n).astype(np.float32), "pressure": rng.uniform(0, 4000, n).astype(np.float32),
              "velocity": rng.normal(0, 1.5, (n, 2)).astype(np.float32), "constant_field": rng.uniform(0.7, 1.1, n).astype(np.float32),
              "level_estimation": lvl}
    order = rng.permutation(n)
    return {k: v[order] for k, v in fields.items()}


def test_the_point_twin_equals_the_lattice_twin():
    f = _synthetic()
    channels = list(sr.CHANNELS)
    assert len(channels) == 6
    for volume in ("density", "rest"):
        p = sr.Particles(f, channels, 1000.0, 0.25, volume)
        assert p.n == 300 and p.h.max() > 2 * p.h.min()
        exps = sr.exponents(p)
        nx, ny = 45, 38
        X, Y = sr.centers(nx, ny, (-0.7, -0.6), 0.041)
        want, foot = sr.raw_planes(p, exps, X, Y)
        PX, PY = np.tile(X, ny), np.repeat(Y, nx)
        got, foot_p, touched = pr.raw_at_points(p, exps, PX, PY)
        assert got.shape == (7, nx * ny) and np.array_equal(got.reshape(7, ny, nx), want)
        assert np.array_equal(foot, foot_p)
        assert np.count_nonzero(want[0]) > 300 and (want[6] < 0).any() and np.count_nonzero(~touched) > 100
        assert not got[:, ~touched].any()
        # any order of the points gives the same words
        perm = np.random.default_rng(1).permutation(nx * ny)
        again, _, _ = pr.raw_at_points(p, exps, PX[perm], PY[perm])
        assert np.array_equal(again, got[:, perm])


def test_the_twins_advect():
    raw = np.array([[1 << 32, 1 << 31, 1 << 30, 0], [1 << 33, -(1 << 30), 1 << 32, 5], [0, 1 << 31, 1 << 20, 7]], np.int64)
    PX, PY = np.array([0.0, 1.0, 2.0, 3.0], np.float32), np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    X, Y, moved = pr.advect(raw, [1, 0], PX, PY, 0.25, 0.5)
    assert moved.tolist() == [True, True, False, False]          # weights 1, 0.5, 0.25, 0
    assert X.tolist() == [0.0 + 0.25 * 4.0, 1.0 + 0.25 * -1.0, 2.0, 3.0]
    assert Y.tolist() == [0.5, 0.5 + 0.25 * 1.0, 0.5, 0.5]
    X, Y, moved = pr.advect(raw, [1, 0], PX, PY, -3e38, 0.5)      # a step that overflows (u_x = 4) stalls the point in both coordinates
    assert moved.tolist() == [False, True, False, False] and X[0] == PX[0] and Y[0] == PY[0] and X[1] == np.float32(1.0) + np.float32(3e38)


def test_line():
    a = probes.line((0.25, -1.0), (0.25, 2.0), 7)
    assert a.dtype == np.float32 and a.shape == (7, 2)
    f = np.float32
    for k in range(7):
        t = f(k) / f(6)
        assert a[k, 0] == f(0.25) + t * (f(0.25) - f(0.25)) and a[k, 1] == f(-1.0) + t * (f(2.0) - f(-1.0))
    assert a[0].tolist() == [0.25, -1.0] and a[-1].tolist() == [0.25, 2.0]
    assert probes.line((0.1, 0.2), (5.0, 6.0), 1).tolist() == [[np.float32(0.1), np.float32(0.2)]]
    with pytest.raises(ValueError):
        probes.line((0, 0), (1, 1), 0)


def test_surface_height():
    ys = np.linspace(0.0, 1.0, 11)
    assert math.isnan(probes.surface_height(np.full(11, 0.1), ys))                          # dry
    assert probes.surface_height(np.full(11, 0.9), ys) == 1.0                                 # submerged to the top
    w = np.array([1, 1, 1, 1, 0.8, 0.2, 0, 0, 0, 0, 0], float)                                # one crossing, between 0.4 and 0.5
    assert probes.surface_height(w, ys) == pytest.approx(0.4 + 0.5 * 0.1)
    assert probes.surface_height(w, ys, threshold=0.8) == pytest.approx(0.4)
    w2 = np.array([1, 1, 0.1, 0, 0, 0.9, 1, 0.7, 0.3, 0, 0], float)                           # a splash above the pool: the highest
    assert probes.surface_height(w2, ys) == pytest.approx(0.7 + 0.5 * 0.1)
    assert probes.surface_height(np.array([0.7]), np.array([0.3])) == 0.3
    with pytest.raises(ValueError):
        probes.surface_height(np.ones(3), np.ones(4))


def test_load_spec_round_trip(tmp_path):
    import yaml
    doc = {"points": [[0.5, -0.25], [1.5, 0.75]], "lines": [{"from": [0.9, -0.7], "to": [0.9, 0.3], "count": 5, "name": "wall"},
                                                           {"from": [0.0, 0.0], "to": [1.0, 0.0], "count": 3}],
           "fields": ["pressure", "velocity"], "volume": "rest"}
    path = tmp_path / "spec.yaml"
    path.write_text(yaml.safe_dump(doc))
    spec = probes.load_spec(path)
    want = np.concatenate([np.array(doc["points"], np.float32), probes.line((0.9, -0.7), (0.9, 0.3), 5), probes.line((0, 0), (1, 0), 3)])
    assert spec.points.dtype == np.float32 and np.array_equal(spec.points, want)
    assert spec.labels == ["0", "1"] + [f"wall[{k}]" for k in range(5)] + ["7", "8", "9"]
    assert spec.fields == ["pressure", "velocity"] and spec.volume == "rest"
    cols = probes.csv_columns(spec)
    assert cols[:3] == ["step", "time", "dt"] and cols[3:7] == ["0:weight", "0:pressure", "0:velocity_x", "0:velocity_y"]
    assert cols[11] == "wall[0]:weight" and len(cols) == 3 + 10 * 4
    # the defaults, and what is refused
    path.write_text("points: [[1, 2]]\n")
    spec = probes.load_spec(path)
    assert spec.fields == ["pressure", "density", "velocity"] and spec.volume == "density" and spec.points.tolist() == [[1.0, 2.0]]
    for text in ("points: [[1, 2]]\nfields: [vorticity]\n", "points: [[1, 2]]\nvolume: cube\n", "point: [[1, 2]]\n"):
        path.write_text(text)
        with pytest.raises(ValueError):
            probes.load_spec(path)


def test_write_vtk_points_is_read_back(tmp_path):
    rng = np.random.default_rng(2)
    pts = rng.uniform(-2, 2, (37, 2)).astype(np.float32)
    data = {"weight": rng.uniform(0, 1, 37).astype(np.float32), "pressure": rng.uniform(0, 5000, 37).astype(np.float32)}
    write_vtk_points(tmp_path / "p.vtk", pts, data)
    got, arrays = pr.read_vtk_points(tmp_path / "p.vtk")
    assert np.array_equal(got, pts) and list(arrays) == ["id", "weight", "pressure"]
    assert np.array_equal(arrays["id"], np.arange(37)) and all(np.array_equal(arrays[k], data[k]) for k in data)
    write_vtk_points(tmp_path / "empty.vtk", np.zeros((0, 2), np.float32))
    got, arrays = pr.read_vtk_points(tmp_path / "empty.vtk")
    assert got.shape == (0, 2) and list(arrays) == ["id"]
    with pytest.raises(ValueError):
        write_vtk_points(tmp_path / "bad.vtk", pts, {"weight": np.zeros(5, np.float32)})
    with VtkPointsExporter(tmp_path / "series", "my-sph-tracers") as ex:
        ex.add_snapshot(0.0, pts)
        ex.add_snapshot(0.5, pts + np.float32(0.25))
    names = sorted(f.name for f in (tmp_path / "series").iterdir())
    assert names == ["my-sph-tracers-00001.vtk", "my-sph-tracers-00002.vtk", "my-sph-tracers.vtk.series"]
    assert np.array_equal(pr.read_vtk_points(tmp_path / "series" / "my-sph-tracers-00002.vtk")[0], pts + np.float32(0.25))
    assert '"time": 0.5' in (tmp_path / "series" / "my-sph-tracers.vtk.series").read_text()
