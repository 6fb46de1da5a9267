"""The state ledger of slab contexts (include/sph_ledger.h: range, fold, sums, compose, the group call) against its restatement
(tests/ledger_reference.py), byte for byte: every rank's words and sums over the ids it owns, the composition against the group call
and against the twin over the whole vector assembled by global id, that every rank folds to the same exponents and the same refusal,
that a ghost slot is no offender, and the refusals."""
import math

import numpy as np
import pytest

from adaptive_sph_amd import distributed as D, ffi, ledger, scene as sc
from adaptive_sph_amd.workloads import dam_break_params, default_params
from tests import ledger_reference as lr
from tests.test_gpu_slab_render import Group, _scene_a, _scene_b, close_all

pytestmark = pytest.mark.gpu

FIXTURES = ["A2", "A3", "B2", "B3"]


@pytest.fixture(scope="module")
def groups(product_lib):
    """which -> the loopback group of tests/test_gpu_slab_render.py's fixture (scene A: the 40 x 32 dam break, 4 steps; scene B: the 2:1
    media scene, 3 steps; k = 2 or 3 slabs), built on first use, gathered once and left unchanged."""
    made = {}

    def get(which):
        if which not in made:
            g = (_scene_a if which[0] == "A" else _scene_b)(product_lib, int(which[1]))
            made[which] = g
            assert all(len(i) > 0 for i in g.ids)
            assert any(np.any(np.diff(i.astype(np.int64)) < 0) for i in g.ids), "slot order equals id order: the test would not see a mix-up"
            g.own = [np.sort(i).astype(np.int64) for i in g.ids]
            g.whole = lr.Particles(g.f, None, g.P.rest_density)           # gathered by global id: the id is the index
        return made[which]

    yield get
    for g in made.values():
        g.close()


def _rank_path(g, what=lr.ALL, exps=None, order=None):
    """range on every member, the fold, the sums, compose -> (Ledger, words, folded spec, sums)"""
    words = [ledger.ledger_rank_words(c, g.P, what, exps) for c in g.ctxs]
    spec, _ = ledger.fold(words, what, exps, lib=g.ctxs[0].lib)
    sums = [ledger.ledger_rank_sums(c, g.P, spec) for c in g.ctxs]
    order = list(range(len(words))) if order is None else order
    return ledger.compose([words[i] for i in order], [sums[i] for i in order], spec, lib=g.ctxs[0].lib), words, spec, sums


@pytest.mark.parametrize("which", FIXTURES)
def test_rank_words_and_sums_equal_the_twin_over_the_owned_ids(groups, which):
    g = groups(which)
    tw = [lr.words(g.whole.subset(own), lr.ALL, None, g.planes) for own in g.own]
    kind, used, folded = lr.fold(tw, lr.ALL)
    assert kind == "ok"
    _, words, spec, sums = _rank_path(g)
    for r, c in enumerate(g.ctxs):
        assert words[r].as_tuple() == tw[r], (which, r)
        assert words[r].n == len(g.own[r]) and sum(c.dist_get_stats()["n_ghost"]) > 0            # it holds ghosts and counts none
        assert sums[r] == lr.sums(g.whole.subset(g.own[r]), lr.ALL, used), (which, r)
    assert list(spec.exponent) == used
    # some rank's own maxima give another exponent than the whole vector's: a rank that took its own would sum at another scale
    own_exps = [lr.fold([w], lr.ALL)[1] for w in tw]
    print(which, "whole", used, "ranks", own_exps)
    assert sum(w[1] for w in tw) == g.n and [sum(col) for col in zip(*sums)] == lr.sums(g.whole, lr.ALL, used)


def test_some_rank_alone_would_take_other_exponents(groups):
    differ = []
    for which in FIXTURES:
        g = groups(which)
        tw = [lr.words(g.whole.subset(own), lr.ALL, None, g.planes) for own in g.own]
        used = lr.fold(tw, lr.ALL)[1]
        differ += [(which, r) for r, w in enumerate(tw) if lr.fold([w], lr.ALL)[1] != used]
    assert differ, "every rank's own maxima give the whole vector's exponents on every fixture: the test shows nothing"


@pytest.mark.parametrize("which", FIXTURES)
def test_compose_equals_the_group_call_and_the_twin(groups, which):
    g = groups(which)
    kind, want = lr.ledger(g.whole, lr.ALL, None, g.planes)
    assert kind == "ok" and want["n"] == g.n
    want_bytes = lr.result_bytes(want)
    assert lr.result_bytes(lr.ledger(g.whole, lr.ALL, None, g.planes, g.own)[1]) == want_bytes      # the twin composes over these cuts
    grp = ledger.ledger_group(g.ctxs, g.P)
    assert bytes(grp) == want_bytes, (which, grp.raw, want["raw"], grp.extremes, want["extreme"])
    per_rank, words, spec, sums = _rank_path(g)
    assert bytes(per_rank) == want_bytes
    back = list(range(len(g.ctxs)))[::-1]
    assert bytes(_rank_path(g, order=back)[0]) == want_bytes                                        # the ranks in any order
    # the extremes sit on different ranks, and the ids are global
    owners = {name: next(r for r, own in enumerate(g.own) if grp.extreme(name)[1] in own) for name in ("min_x", "max_x")}
    assert owners["min_x"] == 0 and owners["max_x"] == len(g.ctxs) - 1
    assert grp.extreme("max_density") == (float(g.f["density"].max()), int(np.argmax(g.f["density"])))
    # every group alone; explicit exponents
    for what in (lr.CARRIED, lr.STEP, lr.OUTSIDE, lr.CARRIED | lr.OUTSIDE):
        w = lr.result_bytes(lr.ledger(g.whole, what, None, g.planes)[1])
        assert bytes(ledger.ledger_group(g.ctxs, g.P, what)) == w and bytes(_rank_path(g, what)[0]) == w, (which, what)
    wider = [e + 2 for e in want["exponent"]]
    w = lr.result_bytes(lr.ledger(g.whole, lr.ALL, wider, g.planes)[1])
    assert bytes(ledger.ledger_group(g.ctxs, g.P, lr.ALL, wider)) == w and bytes(_rank_path(g, lr.ALL, wider)[0]) == w


@pytest.mark.parametrize("which", ["A3", "B2"])
def test_every_rank_folds_to_the_same_exponents_and_the_same_refusal(groups, which):
    g = groups(which)
    words = [ledger.ledger_rank_words(c, g.P) for c in g.ctxs]
    k = len(words)
    folds = [ledger.fold(words[r:] + words[:r], lib=g.ctxs[0].lib) for r in range(k)]              # every rank starts with its own words
    assert len({bytes(spec) for spec, _ in folds}) == 1 and len({bytes(f) for _, f in folds}) == 1
    # an exponent one too small for the kinetic energy: reached on at least two ranks, every rank names the same particle
    used = list(folds[0][0].exponent)
    t = lr.terms(g.whole, lr.ALL)[5]
    tops = sorted(float(t[own].max()) for own in g.own)
    e = math.frexp(tops[-2])[1] - 1                                                                # 2^e <= the second largest of the ranks' maxima
    exps = [None] * 5 + [e] + [None] * 3
    tw = [lr.words(g.whole.subset(own), lr.ALL, exps, g.planes) for own in g.own]
    assert sum(w[0] != lr.NONE for w in tw) >= 2 and len({w[0] for w in tw if w[0] != lr.NONE}) >= 2
    kind, sentence, _ = lr.fold(tw, lr.ALL, exps)
    first = int(np.flatnonzero(t >= 2.0 ** e).min())
    assert kind == "refused" and f"(particle i={first})" in sentence and "sum 5 (kinetic)" in sentence
    words = [ledger.ledger_rank_words(c, g.P, lr.ALL, exps) for c in g.ctxs]                        # SPH_OK whatever the data says
    assert [w.first_bad for w in words] == [w[0] for w in tw]
    for r in range(k):
        with pytest.raises(ffi.SphError) as err:
            ledger.fold(words[r:] + words[:r], lr.ALL, exps, lib=g.ctxs[0].lib)
        assert err.value.status == 1 and str(err.value).endswith(sentence)
    with pytest.raises(ffi.SphError) as err:
        ledger.ledger_group(g.ctxs, g.P, lr.ALL, exps)
    assert err.value.status == 1 and sentence in str(err.value)
    # nothing changed: the next ledger is the twin's
    assert bytes(ledger.ledger_group(g.ctxs, g.P)) == lr.result_bytes(lr.ledger(g.whole, lr.ALL, None, g.planes)[1])


def test_a_ghost_slot_is_no_offender(product_lib):
    """Two slabs cut where m |x| passes a power of two: the particles stand at x in [-2, -0.9], so m |x| spans one octave and 2^e lies
    inside it; the cut is put at x = -2^e / m.  Under the explicit exponent e for the x moment every particle of the LEFT rank offends
    and none of the right rank.  After one step the right rank holds ghosts of the left rank's particles: they would offend, but a
    ghost is not owned -- the right rank's words name nobody, the fold names the left rank's smallest id."""
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.002)
    scn = sc.dam_break_small(40, 24, 1.0 / 37)
    pos, mass, vel = sc.init_particles(scn)
    assert float(mass.min()) == float(mass.max())
    m = float(mass[0])
    e = math.frexp(m)[1]                                              # m < 2^e <= 2 m
    cut = -(2.0 ** e) / m
    assert (pos[:, 0] < cut).sum() > 300 and (pos[:, 0] >= cut).sum() > 300
    g = Group.__new__(Group)
    g.P, g.p, g.n, g.planes = P, P.to_ffi(), len(mass), sc.boundary_planes(scn.boundary)
    g.ctxs = D.make_loopback_group(product_lib, pos, mass, vel, g.planes, 2, cuts=[-D.INF, cut, D.INF])
    try:
        ffi.group_step(g.ctxs, g.p)
        g.gather()
        own = [np.sort(i).astype(np.int64) for i in g.ids]
        whole = lr.Particles(g.f, None, P.rest_density)
        exps = [None] * 3 + [e] + [None] * 5
        tw = [lr.words(whole.subset(o), lr.CARRIED, exps) for o in own]
        assert tw[0][0] == (int(own[0][0]) << 8 | lr.BAD_TERM + 3) and tw[1][0] == lr.NONE              # what the construction is for
        t = np.abs(lr.terms(whole, lr.CARRIED)[3])
        assert (t[own[0]] >= 2.0 ** e).all() and (t[own[1]] < 2.0 ** e).all()
        assert sum(g.ctxs[1].dist_get_stats()["n_ghost"]) > 0                                          # the right rank holds ghosts: all of them offenders
        words = [ledger.ledger_rank_words(c, P, lr.CARRIED, exps) for c in g.ctxs]
        assert [w.as_tuple() for w in words] == tw
        assert words[1].first_bad == ffi.LEDGER_NO_OFFENDER and words[1].n == len(own[1])
        with pytest.raises(ffi.SphError) as err:
            ledger.fold(words, lr.CARRIED, exps, lib=product_lib)
        assert f"sum 3 (moment_x) is not finite or not below 2^exponent = 2^{e} (particle i={own[0][0]})" in str(err.value)
        # with automatic exponents the group's ledger is the twin's
        assert bytes(ledger.ledger_group(g.ctxs, P)) == lr.result_bytes(lr.ledger(whole, lr.ALL, None, g.planes)[1])
    finally:
        g.close()


def test_before_the_first_step_every_slot_is_owned(product_lib):
    scn = sc.dam_break_small(24, 20, 1.0 / 24)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004)
    whole = lr.Particles({"mass": mass, "position": pos, "velocity": vel}, None, P.rest_density)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 3)
    try:
        want = lr.ledger(whole, lr.CARRIED | lr.OUTSIDE, None, planes)[1]
        assert bytes(ledger.ledger_group(grp, P, lr.CARRIED | lr.OUTSIDE)) == lr.result_bytes(want) and want["n"] == len(mass)
        with pytest.raises(ffi.SphError, match=r"particle i=0; before the first step") as err:          # the smallest GLOBAL id
            ledger.ledger_group(grp, P)
        assert err.value.status == 1
        words = [ledger.ledger_rank_words(c, P) for c in grp]
        assert len({w.first_bad for w in words}) == 3 and all(w.first_bad & 0xFF == lr.BAD_RHO_SIGN for w in words)
        ffi.group_step(grp, P.to_ffi())                                                                # not poisoned: the group steps on
        assert ledger.ledger_group(grp, P).n == len(mass)
    finally:
        close_all(grp)


def _refused(status, word, f, *a, **kw):
    with pytest.raises(ffi.SphError) as e:
        f(*a, **kw)
    assert e.value.status == status and word in str(e.value), (status, word, e.value)


def test_refusals(product_lib):
    P = default_params(merging=False, sharing=False, splitting=False, max_dt=0.004)
    scn = sc.dam_break_small(24, 20, 1.0 / 24)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    p = P.to_ffi()
    plain = ffi.Context(product_lib, len(mass) + 64, planes)
    grp = D.make_loopback_group(product_lib, pos, mass, vel, planes, 2)
    C = ffi.C
    try:
        plain.upload(mass, pos, vel)
        explicit = ledger.ledger_spec(lr.CARRIED, [0] * 9)
        # a plain context given to a slab call or as a member; a slab context given to sph_ledger_compute
        _refused(30, "not a slab context", ledger.ledger_rank_words, plain, P, lr.CARRIED)
        _refused(30, "not a slab context", ledger.ledger_rank_sums, plain, P, explicit)
        _refused(30, "no slab context", ledger.ledger_group, [grp[0], plain], P, lr.CARRIED)
        _refused(30, "no slab context", ledger.ledger_group, [plain, grp[0]], P, lr.CARRIED)
        _refused(30, "one rank holds a slab", ledger.ledger, grp[1], P, lr.CARRIED)
        # an automatic exponent given to the sums; no or unknown groups; exponents outside the range; null pointers; n < 1
        _refused(1, "sph_ledger_fold_words", ledger.ledger_rank_sums, grp[0], P, ledger.ledger_spec(lr.CARRIED))
        for what in (0, 8):
            _refused(1, "group", ledger.ledger_rank_words, grp[0], P, what)
            _refused(1, "group", ledger.ledger_rank_sums, grp[0], P, ledger.ledger_spec(what, [0] * 9))
            _refused(1, "group", ledger.ledger_group, grp, P, what)
        _refused(1, "exponent -201", ledger.ledger_rank_words, grp[0], P, lr.CARRIED, [-201] + [None] * 8)
        _refused(1, "exponent 300", ledger.ledger_group, grp, P, lr.CARRIED, [0] * 6 + [300, 0, 0])
        _refused(1, "null", ledger.ledger_rank_words, grp[0], None, lr.CARRIED)
        _refused(1, "null", ledger.ledger_rank_sums, grp[0], P, None)
        _refused(1, "n < 1", ledger.ledger_group, [], P)
        spec, words, sums, out = ledger.ledger_spec(lr.CARRIED), ffi.SphLedgerWords(), (ffi.SphLedgerSum * 9)(), ffi.SphLedgerResult()
        handles = (C.c_void_p * 2)(*[c.handle for c in grp])
        assert product_lib.slab_ledger_range(grp[0].handle, C.byref(p), C.byref(spec), None) == 1
        assert product_lib.slab_ledger_range(grp[0].handle, C.byref(p), None, C.byref(words)) == 1
        assert product_lib.slab_ledger_sums(grp[0].handle, C.byref(p), C.byref(explicit), None) == 1
        assert product_lib.group_ledger(handles, 0, C.byref(p), C.byref(spec), C.byref(out)) == 1
        assert product_lib.group_ledger(None, 2, C.byref(p), C.byref(spec), C.byref(out)) == 1
        assert product_lib.group_ledger(handles, 2, None, C.byref(spec), C.byref(out)) == 1
        assert product_lib.group_ledger(handles, 2, C.byref(p), None, C.byref(out)) == 1
        assert product_lib.group_ledger(handles, 2, C.byref(p), C.byref(spec), None) == 1
        assert product_lib.group_ledger(handles, 2, C.byref(p), C.byref(spec), C.byref(out)) == 0 and out.n == len(mass)
        ffi.group_step(grp, p)                                           # the refusals left the group able to step and to answer
        assert ledger.ledger_group(grp, P).n == len(mass)
    finally:
        plain.close()
        close_all(grp)


def test_a_poisoned_slab_group_keeps_no_ledger(product_lib):
    """Contexts with room for their owned particles but not for a ghost layer: the step ends in SPH_ERR_CAPACITY and leaves them
    poisoned (tests/test_gpu_slab_render.py); the range, the sums and the group call answer SPH_ERR_POISONED."""
    scn = sc.dam_break_small(96, 48, 1 / 48)
    pos, mass, vel = sc.init_particles(scn)
    planes = sc.boundary_planes(scn.boundary)
    P = dam_break_params(max_iters=3, level_estimation_method="EmptyAngle", maximum_surface_distance=0.2, particle_radius_fine=0.004,
                         particle_radius_base=0.02)
    p = P.to_ffi()
    cuts = D.slab_cuts(pos[:, 0], 2)
    parts = D.partition(pos[:, 0], cuts)
    grp = []
    try:
        for r in range(2):
            c = ffi.Context(product_lib, len(parts[r]) + 8, planes)
            c.dist_configure(r, 2, cuts[r], cuts[r + 1])
            c.upload(mass[parts[r]], pos[parts[r]], vel[parts[r]])
            c.upload_field("particle_id", parts[r].astype(np.uint32))
            grp.append(c)
        with pytest.raises(ffi.SphError) as e:
            for _ in range(3):
                ffi.group_step(grp, p)
        assert e.value.status == 3
        _refused(31, "undefined", ledger.ledger_group, grp, P, lr.CARRIED)
        for c in grp:
            _refused(31, "undefined", ledger.ledger_rank_words, c, P, lr.CARRIED)
            _refused(31, "undefined", ledger.ledger_rank_sums, c, P, ledger.ledger_spec(lr.CARRIED, [0] * 9))
    finally:
        close_all(grp)
