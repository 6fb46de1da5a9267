"""The host-side predictor of the neighbour-list forms (tests/oracle_harness.py) against the CPU oracle alone -- no device.  What
tests/test_gpu_list_forms.py asserts about its scenes (a form's share, the threshold pairs 32 / 33 candidates in a row, 24 / 25 offset
slots, 128 / 129 list entries, waves that hold two forms, the 16-bit crossing of the strip, the 20 000 / 20 001 cluster) is a property of the
scene and of the predictor, so it is checked here where no GPU is needed."""
import numpy as np
import pytest

from adaptive_sph_amd import ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params
from tests import oracle_harness as oh


def forced(**kw):
    return dam_break_params(hybrid_dfsph_max_avg_density_error=0.0, hybrid_dfsph_max_avg_divergence_error=0.0, iisph_max_avg_density_error=0.0,
                            max_dt=2e-5, max_iters=4, **kw)


def oracle_step(oracle_lib, scn, pos, mass, vel, **kw):
    o = ffi.Context(oracle_lib, len(mass), sc.boundary_planes(scn.boundary))
    o.upload(mass, pos, vel)
    o.step(forced(**kw).to_ffi())
    return o


@pytest.mark.parametrize("name", sorted(oh.LIST_FORM_SCENES))
def test_scenes_exercise_what_they_are_for(oracle_lib, name):
    scn, pos, mass, vel = oh.LIST_FORM_SCENES[name]()
    assert 1500 <= len(mass) <= 10000
    o = oracle_step(oracle_lib, scn, pos, mass, vel)
    for policy in ("fast", "exact"):
        f = oh.list_form_facts(o, pos, policy)
        c = f["counts"]
        # the wall flag of the list word (a boundary term: lambda or its gradient non-zero) is lambda_sum != 0 in these scenes
        assert np.array_equal(o.download("lambda_sum") != 0, (o.download("lambda_grad_sum") != 0).any(axis=1))
        assert c["n_mask"] + c["n_index"] + c["n_walk"] == c["n_lists"] == len(mass)
        # the neighbour counts per form add up to the oracle's
        assert sum(int(f["neighbor_count"][f["form"] == k].sum()) for k in (oh.FORM_MASK, oh.FORM_INDEX, oh.FORM_WALK)) == int(o.download("neighbor_count").sum())
        assert oh.LIST_FORM_REQUIREMENTS[name][policy](f), (policy, {k: v for k, v in f.items() if not isinstance(v, np.ndarray)})
        if policy == "fast":   # an offset list only beside a mask word, never beyond 24 others
            assert not (f["has_list"] & (f["form"] != oh.FORM_MASK)).any() and (f["neighbor_count"][f["has_list"]] - 1 <= oh.OFFSET_SLOTS).all()
    o.close()


def test_candidate_rows_against_a_brute_force_count(oracle_lib):
    """candidate_rows through the cell-start table == counting, per particle, the particles of the three cells of each row"""
    scn, pos, mass, vel = oh.LIST_FORM_SCENES["half_squeezed"]()
    o = oracle_step(oracle_lib, scn, pos, mass, vel)
    g, ci = o.grid(), o.download("cell_index").astype(np.int64)
    rows = oh.candidate_rows(g, ci)
    cx, cy = ci % g.size_x, ci // g.size_x
    for i in np.random.default_rng(0).integers(0, len(ci), 200):
        for dr in range(3):
            assert rows[i, dr] == int(((cy == cy[i] + dr - 1) & (np.abs(cx - cx[i]) <= 1)).sum())
    # every neighbour is a candidate: a list never holds more than the three rows do
    assert (o.download("neighbor_count") <= rows.sum(axis=1)).all()
    # the device's slots are a permutation that keeps the upload order inside a cell
    slot = oh.device_slots(ci)
    order = np.argsort(slot)
    assert (np.diff(ci[order]) >= 0).all() and (np.diff(order)[np.diff(ci[order]) == 0] > 0).all()
    o.close()


def test_the_strip_crosses_the_16_bit_range_in_both_directions(oracle_lib):
    scn = oh.strip_scene()
    pos, mass, vel = sc.init_particles(scn)
    o = oracle_step(oracle_lib, scn, pos, mass, vel)
    f = oh.list_form_facts(o, pos)
    assert f["counts"]["n_mask"] == len(mass) == 6 * 15800 and (f["neighbor_count"] - 1).max() <= oh.OFFSET_SLOTS
    oh.assert_strip_crossings(f, pos, o.grid(), o.download("cell_index"))
    o.close()


@pytest.mark.parametrize("others", [19999, 20000])
def test_the_cluster_sits_on_the_neighbour_count_guard(oracle_lib, others):
    pos, mass, vel = oh.cluster_scene(others)
    o = ffi.Context(oracle_lib, len(mass), sc.boundary_planes(sc.SceneBoundary("box", 4.0, 2.0)))
    o.upload(mass, pos, vel)
    if others + 1 <= oh.MAX_NEIGHBOR_COUNT:
        o.step(forced().to_ffi())
        nc = o.download("neighbor_count")
        assert nc.max() == nc[0] == oh.MAX_NEIGHBOR_COUNT and nc[1:].max() < oh.MAX_NEIGHBOR_COUNT // 2
    else:
        with pytest.raises(ffi.SphError) as e:
            o.step(forced().to_ffi())
        assert e.value.status == 16
    o.close()


@pytest.mark.parametrize("name,policy,constant,key", [("rows_32_33", "fast", "ROW_CAP", "n_walk"), ("index_128_129", "exact", "INDEX_CAP", "n_index")])
def test_an_off_by_one_threshold_changes_the_predicted_counts(oracle_lib, monkeypatch, name, policy, constant, key):
    """the threshold scenes discriminate: a decision taken at 33 candidates / 129 entries instead of 32 / 128 (or at 31 / 127) gives other
    counts, so a kernel whose comparison is off by one cannot equal the prediction there"""
    scn, pos, mass, vel = oh.LIST_FORM_SCENES[name]()
    o = oracle_step(oracle_lib, scn, pos, mass, vel)
    want = oh.list_form_facts(o, pos, policy)["counts"][key]
    for delta in (-1, 1):
        monkeypatch.setattr(oh, constant, getattr(oh, constant) + delta)
        assert oh.list_form_facts(o, pos, policy)["counts"][key] != want, delta
        monkeypatch.undo()
    o.close()


def test_extended_lists_of_squeeze_045_pass_128_entries(oracle_lib):
    """The premise of test_gpu_list_forms.py::test_level_estimation_on_crowded_extended_lists: at the level estimation's range
    (level_estimation_range / 1.9 of h instead of 2) the lists of squeeze_0.45 hold <= 128 entries (index list) for one part of the block
    and more (candidate walk) for the other -- counted by brute force with the kernels' predicate, r^2 < (h k)^2 in f32."""
    scn, pos, mass, vel = oh.LIST_FORM_SCENES["squeeze_0.45"]()
    o = oracle_step(oracle_lib, scn, pos, mass, vel)
    h = np.float32(1.9) * np.sqrt(mass[0] * np.float32(0.318309873342514038086), dtype=np.float32)
    k = np.float32(dam_break_params().level_estimation_range) / np.float32(1.9)
    s = np.float32(h * k)
    dx = pos[:, None, 0] - pos[None, :, 0]
    dy = pos[:, None, 1] - pos[None, :, 1]
    count = ((dx * dx + dy * dy) < s * s).sum(axis=1)
    assert (count > o.download("neighbor_count")).all()
    form, c = oh.predict_list_forms(o.grid(), o.download("cell_index"), count, o.download("lambda_sum"), extended=True)
    assert c["n_mask"] == 0 and c["n_index"] >= 500 and c["n_walk"] >= 500, c
    o.close()
