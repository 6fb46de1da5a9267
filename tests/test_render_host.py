"""The renderer's host half (no GPU): recipe parsing of the media fixtures, ColorMap::get, the PNG writer, the numpy restatement of
the rasteriser on hand-built cases, and the SipHash the RandomColor attribute hashes with."""
import os
import subprocess
import sys
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest

from adaptive_sph_amd import ffi, render
from adaptive_sph_amd import image_export as ie
from tests import render_reference as rr

MEDIA = Path(__file__).parent / "golden" / "media"


# ---- recipes ----------------------------------------------------------------------------------------------------------------
def test_neighbor_numbers_recipe_parses():
    cfgs = ie.parse_recipe(MEDIA / "neighbor-numbers.yaml")
    assert [c.png_file for c in cfgs] == ["neighbor-number-from-distribution.png", "neighbor-number-from-mass.png"]
    ests = []
    for c in cfgs:
        assert c.visualization_params.visualized_attribute == "NeighborCount"
        assert c.time == pytest.approx(0.9) and c.scene_file == "scene-ratio2to1.yaml" and c.scene is None
        assert c.image_width is None and c.zoom_out is None and c.video_start_time is None
        params, scene = ie.resolve_entry(c, MEDIA)   # ../default-config.yaml -> tests/golden/default-config.yaml
        assert not (params.merging or params.sharing or params.splitting)
        assert len(scene.blocks) == 2
        ests.append(params.support_length_estimation)
    assert ests == ["FromDistributionClamped1", "FromMass"]


def test_surface_detection_recipe_parses():
    cfgs = ie.parse_recipe(MEDIA / "surface-detection.yaml")
    assert len(cfgs) == 2
    for c, method in zip(cfgs, ("CenterDiff", "EmptyAngle")):
        v = c.visualization_params
        assert v.visualized_attribute == "SingleColor" and v.show_flag_is_fluid_surface and not v.take_data_from_stash
        assert c.no_legend
        params, _ = ie.resolve_entry(c, MEDIA)
        assert params.level_estimation_method == method and params.boundary_is_fluid_surface
        rp = render.render_params(v, params, 8, 4)
        assert rp.flags == ffi.RENDER_SHOW_SURFACE and rp.attribute == render.VISUALIZED_ATTRIBUTES.index("SingleColor")


def test_video_recipe_parses():
    (c,) = ie.parse_recipe(MEDIA / "video-default.yaml")
    assert c.video_start_time == 0 and c.video_fps == 60 and c.video_speed == pytest.approx(0.25) and c.time == 3
    assert c.png_file == "video-default.mp4" and c.video_img_dir is None and c.no_legend
    params, scene = ie.resolve_entry(c, MEDIA)     # scene_file "../default-scene.yaml"
    assert params.viscosity_type == "ApproxLaplace" and params.init_boundary_handler == "AnalyticOverestimate"
    assert scene.boundary.width == 2


def test_density_recipe_is_refused_like_the_reference():
    # visualized_attribute at top level: serde finds no visualization_params
    with pytest.raises(ie.RecipeError, match="failed parsing export config file"):
        ie.parse_recipe(MEDIA / "density.yaml")


def test_surface_distance_recipe_is_refused_like_the_reference():
    cfgs = ie.parse_recipe(MEDIA / "surface-distance.yaml")
    with pytest.raises(ie.RecipeError, match="not able to find attribute fill_stash_with"):
        ie.resolve_entry(cfgs[0], MEDIA)


def test_scene_and_scene_file_rules(tmp_path):
    base = dict(time=0.1, config_path=str(Path(__file__).parent / "golden" / "default-config.yaml"),
                visualization_params={"visualized_attribute": "Velocity"}, png_file="x.png")
    c = ie.ImageExportConfig.from_mapping(base)
    with pytest.raises(ie.RecipeError, match=r"^expected either 'scene' or 'scene_file'$"):
        ie.resolve_entry(c, tmp_path)
    c = ie.ImageExportConfig.from_mapping(dict(base, scene={"boundary": {"type": "box", "width": 2, "height": 2}, "blocks": []},
                                               scene_file="a.yaml"))
    with pytest.raises(ie.RecipeError, match="Not both!"):
        ie.resolve_entry(c, tmp_path)


def test_unknown_attribute_variant_is_a_parse_error(tmp_path):
    p = tmp_path / "r.yaml"
    p.write_text("- time: 1\n  config_path: c.yaml\n  visualization_params:\n    visualized_attribute: Colour\n  png_file: a.png\n")
    with pytest.raises(ie.RecipeError, match="failed parsing export config file"):
        ie.parse_recipe(p)


# ---- colour maps ------------------------------------------------------------------------------------------------------------
def test_color_map_get_clamps_and_interpolates():
    cm = render.ColorMap([(1.0, (1, 1, 1)), (0.0, (0, 0, 0)), (2.0, (1, 0, 0))])   # sorted at construction
    assert [float(v) for v, _ in cm.color_stops()] == [0.0, 1.0, 2.0]
    assert cm.get(-5) == (0, 0, 0) and cm.get(9) == (1, 0, 0)
    assert cm.get(0.5) == (np.float32(0.5),) * 3
    assert cm.get(1.5) == (1, np.float32(0.5), np.float32(0.5))
    assert cm.get(float("nan")) == (0, 0, 0)
    stops = [(float(v), *map(float, c)) for v, c in cm.color_stops()]
    x = np.array([-5, 0, 0.25, 0.5, 1, 1.5, 2, 9, np.nan], np.float32)
    want = np.array([rr._u8(cm.get(v)) for v in x])
    assert np.array_equal(rr.cmap_get(stops, x), want)


def test_fixed_maps_fit_the_stop_limit():
    P = type("P", (), {"maximum_surface_distance": 0.45})()
    for attr in render.VISUALIZED_ATTRIBUTES:
        cm = render.get_color_map(attr, P)
        if cm is not None:
            assert 1 <= len(cm.color_stops()) <= ffi.RENDER_MAX_STOPS
            vs = [float(v) for v, _ in cm.color_stops()]
            assert vs == sorted(vs)
    inf = render.get_color_map("Distance", P).color_stops()
    assert float(inf[0][0]) == pytest.approx(-0.45) and float(inf[-1][0]) == 0.0


# ---- PNG --------------------------------------------------------------------------------------------------------------------
def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (13, 21, 3), dtype=np.uint8)
    p = tmp_path / "a.png"
    render.write_png(p, img)
    data = p.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, tags = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        tags.append(tag)
        pos += 12 + n
    assert tags == [b"IHDR", b"IDAT", b"IEND"]
    assert np.array_equal(render.decode_png(data), img)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(p) as im:
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)


def test_legend_draws_gradient_frame_and_ticks():
    img = np.full((100, 200, 3), 255, np.uint8)
    cm = render.ColorMap([(0.0, (0, 0, 1)), (1.0, (1, 0, 0))])
    render.draw_legend(img, cm)
    x = int(200 * 0.865)
    assert tuple(img[45, x]) != (255, 255, 255) and img[45, x, 2] > img[45, x, 0]   # bottom: the minimum's blue
    assert img[25, x, 0] > img[25, x, 2]                                              # top: the maximum's red
    assert tuple(img[35, int(200 * 0.83)]) == (0, 0, 0)                               # the frame
    assert tuple(img[50, int(200 * 0.83) - 1]) == (0, 0, 0)                           # tick of the minimum (text on the left)
    assert tuple(img[5, 5]) == (255, 255, 255)


# ---- the rasteriser's predicates on hand-built scenes ------------------------------------------------------------------------
def _frame(w, h, s=1, zoom=1.0, segments=()):
    return rr.Frame(w, h, s, zoom, segments)


def test_overlapping_discs_the_larger_index_wins_whatever_the_order():
    f = _frame(40, 40)
    pos = np.array([[0.0, 0.0], [0.2, 0.0]], np.float32)
    r = np.array([0.3, 0.3], np.float32)
    rgb = np.array([[255, 0, 0], [0, 0, 255]], np.uint8)
    img = f.render(pos, r, rgb)
    # scale = 40 / 2 = 20 px per unit; the overlap around x = 0.1 -> column 22 belongs to particle 1 (blue)
    assert tuple(img[20, 22]) == (0, 0, 255)
    assert tuple(img[20, 16]) == (255, 0, 0)
    img2 = f.render(pos[::-1], r[::-1], rgb[::-1])   # swapped: now the red one has the larger index
    assert tuple(img2[20, 22]) == (255, 0, 0)


def test_stroke_band_is_black():
    f = _frame(100, 100)
    pos = np.array([[0.0, 0.0]], np.float32)
    r = np.array([0.5], np.float32)   # 25 px; band [23.75, 26.25)
    img = f.render(pos, r, np.array([[10, 200, 30]], np.uint8))
    assert tuple(img[50, 50]) == (10, 200, 30)
    assert tuple(img[50, 50 + 24]) == (0, 0, 0)       # u = 74.5 -> 24.5 px from the centre
    assert tuple(img[50, 50 + 27]) == (255, 255, 255)


def test_boundary_segment_is_black_outside_particles():
    seg = [(-0.5, -1.0, -0.5, 1.0)]
    f = _frame(100, 50, segments=seg)   # W != H: scale = 50 / 2 = 25
    img = f.render(np.zeros((0, 2), np.float32), np.zeros(0, np.float32), np.zeros((0, 3), np.uint8))
    col = int(50 - 0.5 * 25)   # x = -0.5 -> u = 37.5
    assert tuple(img[25, col]) == (0, 0, 0)
    assert tuple(img[25, col + 2]) == (255, 255, 255)
    assert tuple(img[0, col]) == (0, 0, 0) and img.shape == (50, 100, 3)


def test_supersampling_averages_in_integers():
    f = _frame(4, 4, s=2)
    keys = np.zeros((8, 8), np.uint32)
    keys[0, 0] = 1
    # one of the four samples of pixel (0, 0) shows particle 0 filled red
    pos = np.array([[-1.0 + 0.125, 1.0 - 0.125]], np.float32)   # centre of sample (0, 0): scale = 4 samples per unit
    r = np.array([0.1], np.float32)
    img = f.resolve(keys, pos, r, np.array([[255, 0, 0]], np.uint8))
    assert tuple(img[0, 0]) == (255, (3 * 255 + 2) // 4, (3 * 255 + 2) // 4)
    assert tuple(img[1, 1]) == (255, 255, 255)


def test_rust_default_hasher_is_siphash13_and_python_agrees_on_siphash24():
    msgs = [i.to_bytes(8, "little") for i in (0, 1, 2, 12345, 2 ** 40 + 7)]
    code = "import sys\nfor m in sys.argv[1:]: print(sys.hash_info.algorithm, hash(bytes.fromhex(m)))"
    out = subprocess.run([sys.executable, "-c", code] + [m.hex() for m in msgs], env=dict(os.environ, PYTHONHASHSEED="0"),
                         capture_output=True, text=True, check=True).stdout.split("\n")
    algo = out[0].split()[0]
    c, d = {"siphash24": (2, 4), "siphash13": (1, 3)}.get(algo, (None, None))
    if c is None:
        pytest.skip(f"this interpreter hashes bytes with {algo}")
    for m, line in zip(msgs, out):
        h = rr.siphash(m, 0, 0, c, d)
        signed = h - (1 << 64) if h >= 1 << 63 else h
        if signed == -1:
            signed = -2
        assert int(line.split()[1]) == signed
    # the (1, 3) variant is Rust's DefaultHasher of a usize: the published SipHash-1-3 of the 8 bytes (keys 0) for i = 0
    assert rr.rust_default_hash_usize(0) == rr.siphash(bytes(8), 0, 0, 1, 3)


def test_render_entry_points_are_exported_by_the_product_library():
    from adaptive_sph_amd import build
    lib = ffi.SphLibrary(build.build_hip(), "sph_")
    for s in ffi.RENDER_SYMBOLS:
        assert getattr(lib.lib, "sph_" + s) is not None
    header = (Path(__file__).resolve().parent.parent / "include" / "sph_render.h").read_text()
    for s in ffi.RENDER_SYMBOLS:
        assert f"int sph_{s}(" in header


def test_image_subcommand_is_wired():
    from adaptive_sph_amd.__main__ import build_parser
    a = build_parser().parse_args(["image", "a.yaml", "b.yaml", "--supersample", "2"])
    assert a.command == "image" and a.RECIPE == ["a.yaml", "b.yaml"] and a.supersample == 2
