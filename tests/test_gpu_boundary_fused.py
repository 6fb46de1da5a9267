"""The step boundary of a plain context in three launches -- integrating tail, count, place (sph_sort.hip: k_inc_count<true> carries the
reduction of the tail's header partials in a workgroup of its own and leaves the cell-range table in its two-level form;
k_inc_place_reorder<false, true> takes the prefix of the block sums per wave and finishes the table for the next step's BUILD) -- against
the five it replaces (SPH_BOUNDARY_FUSED=0: tail, k_header_ahead, count, k_inc_scan, place).  Two contexts of one process step side by
side; after every step: dt, both iteration counts, the grid, the cell indices, the neighbour lists, the fields and what the host made of
the mover count (the form of every build: merge or radix sort) are equal bit for bit."""
import numpy as np
import pytest

from adaptive_sph_amd import ffi, scene as sc
from adaptive_sph_amd.workloads import dam_break_params
from tests.test_gpu_incremental_sort import scene_of

pytestmark = pytest.mark.gpu

STEPS = 12
FIELDS = ("position", "velocity", "density", "pressure", "cell_index")
ONLY_IN_ONE_FORM = ("inc_scan", "header_ahead")


def scene(kind):
    """small: at most 1024 cells -- one count block, which is also the last one.  col180: a cell count that is no multiple of 1024 over
    several count blocks.  column: at rest when the run starts -- steps without a mover.  thrown / collide: many movers, a travelling
    bounding box (tests/test_gpu_incremental_sort.py)."""
    if kind == "small":
        return sc.dam_break_small(24, 16, 1 / 64), {}
    if kind == "col180":
        return sc.dam_break_small(180, 180, 1 / 128), {}
    return scene_of(kind)


def grid_tuple(c):
    g = c.grid()
    return (g.cell_size, g.cells_min_x, g.cells_min_y, g.size_x, g.size_y)


def make_pair(lab_lib, monkeypatch, kind, solver, env=None):
    scn, over = scene(kind)
    pos, mass, vel = sc.init_particles(scn)
    P = dam_break_params(pressure_solver_method=solver, **over)
    planes = sc.boundary_planes(scn.boundary, P.init_boundary_handler)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    out = []
    for form in ("fused", "split"):   # (the switches are read at sph_create)
        if form == "split":
            monkeypatch.setenv("SPH_BOUNDARY_FUSED", "0")
        g = ffi.Context(lab_lib, len(mass), planes)
        if form == "split":
            monkeypatch.delenv("SPH_BOUNDARY_FUSED")
        g.upload(mass, pos, vel)
        g.profile_enable(1)
        out.append(g)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return out[0], out[1], P.to_ffi()


def build_launches(c):
    return {k: v[0] for k, v in c.profile_get().items()
            if (k.startswith(("inc_", "sort_", "rs_")) or k in ("reorder", "cell_start", "header")) and k not in ONLY_IN_ONE_FORM}


def step_and_compare(a, b, p, s):
    sa, sb = a.step(p), b.step(p)
    ka = (np.float32(sa.dt).view(np.uint32).item(), int(sa.div_solver.iters), int(sa.density_solver.iters), int(sa.density_solver.normal_count))
    kb = (np.float32(sb.dt).view(np.uint32).item(), int(sb.div_solver.iters), int(sb.density_solver.iters), int(sb.density_solver.normal_count))
    assert ka == kb, s
    assert grid_tuple(a) == grid_tuple(b), s
    for f in FIELDS:
        assert np.array_equal(a.download(f), b.download(f)), (s, f)
    (oa, ia), (ob, ib) = a.download_neighbors(), b.download_neighbors()
    assert np.array_equal(oa, ob) and np.array_equal(ia, ib), s
    # what the host read in the mapped mover-count word decides the form of the build it queues: the launches of every scope of a
    # build agree, but for the two the fused form does not have (the sweeps' do not: a paced solve queues iterations in vain as the
    # host's timing has it)
    pa, pb = (build_launches(c) for c in (a, b))
    assert pa == pb, (s, pa, pb)


def forms_differ(a, b, merges_at_least):
    pa, pb = a.profile_get(), b.profile_get()
    assert pa.get("inc_reorder", (0, 0))[0] >= merges_at_least, pa
    assert all(k not in pa for k in ONLY_IN_ONE_FORM), pa                       # three launches ...
    assert pb["inc_scan"][0] == pb["inc_reorder"][0] and pb["header_ahead"][0] >= pb["inc_reorder"][0], pb   # ... against five


CASES = [("small", "HybridDFSPH"), ("small", "IISPH"), ("col180", "HybridDFSPH"), ("col180", "OnlyDivergence"), ("column", "HybridDFSPH"),
         ("thrown", "HybridDFSPH"), ("thrown", "OnlyDivergence"), ("collide", "IISPH")]


@pytest.mark.parametrize("kind,solver", CASES)
def test_three_launch_boundary_is_the_five_launch_boundary(lab_lib, monkeypatch, kind, solver):
    a, b, p = make_pair(lab_lib, monkeypatch, kind, solver)
    sizes = set()
    for s in range(STEPS):
        step_and_compare(a, b, p, s)
        sizes.add(grid_tuple(a)[1:])
    g = a.grid()
    ncells = g.size_x * g.size_y
    print(kind, solver, "cells", ncells, "grids", len(sizes), {k: v[0] for k, v in a.profile_get().items() if k.startswith("inc_") or k == "sort_scatter"})
    if kind == "small":
        assert ncells <= 1024
    if kind == "col180":
        assert ncells % 1024 != 0 and ncells > 2 * 1024
    if kind in ("thrown", "collide"):
        assert len(sizes) > 1, sizes   # the predicted grid did change size between steps
    forms_differ(a, b, STEPS - 2)   # (every build but the first of the run was queued ahead as a merge)
    a.close()
    b.close()


def test_mover_count_that_crosses_the_merge_limit_selects_the_same_builds(lab_lib, monkeypatch):
    """SPH_INC_SORT=k: the merge up to n / k movers.  A thrown block with a low limit: whether a build is a merge or a radix sort hangs on
    the count the device handed over -- from the first finishing workgroup of the place launch here, from k_inc_scan there."""
    a, b, p = make_pair(lab_lib, monkeypatch, "thrown", "HybridDFSPH", env=dict(SPH_INC_SORT="40"))
    for s in range(STEPS):
        step_and_compare(a, b, p, s)
    print({k: v[0] for k, v in a.profile_get().items() if k.startswith("inc_") or k == "sort_scatter"})
    a.close()
    b.close()


def test_header_dropped_by_the_host_is_rebuilt_by_the_header_kernel(lab_lib, monkeypatch):
    """sph_download and sph_upload_field between steps: the upload drops the header the count launch published and the build queued with
    it -- the next step launches k_header and sorts at its start, in both forms alike."""
    a, b, p = make_pair(lab_lib, monkeypatch, "column", "HybridDFSPH")
    for s in range(STEPS):
        step_and_compare(a, b, p, s)
        if s % 3 == 1:
            for c in (a, b):
                v = c.download("velocity")
                c.upload_field("velocity", v * np.float32(0.5))
    pa = a.profile_get()
    assert pa["header"][0] >= 1 + STEPS // 3, pa   # the first step's, and one after every upload
    forms_differ(a, b, STEPS - 2 - STEPS // 3)
    a.close()
    b.close()
