"""sph_ledger_fold_words and sph_ledger_compose (include/sph_ledger.h: host arithmetic, no context, no device) through ctypes with
hand-made words and sums, against tests/ledger_reference.py: carries across 2^64, negative sums, the order of the ranks, an empty rank,
ties and signed zeros among the extremes, the smallest offender and its sentence, the automatic exponents, correct rounding."""
import ctypes as C
import math
import random
import struct

import numpy as np
import pytest

from adaptive_sph_amd import ffi, ledger
from tests import ledger_reference as lr

f32 = np.float32


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", abs(float(x))))[0]


def _key(k, value, i):
    o = int(lr.ord_f32(np.array([value], f32))[0])
    return (o << 32) | (lr.NO_ID - i if lr.is_max(k) else i)


def _words(first_bad=lr.NONE, n=0, n_outside=0, bits=None, keys=None):
    e = lr.empty_words()
    b, k = list(e[3]), list(e[4])
    for s, v in (bits or {}).items():
        b[s] = v
    for j, v in (keys or {}).items():
        k[j] = v
    return first_bad, n, n_outside, tuple(b), tuple(k)


def _compose(product_lib, words, sums, what, used):
    spec = ledger.ledger_spec(what, used)
    got = ledger.compose(words, sums, spec, lib=product_lib)
    want = lr.compose(words, sums, what, used)
    assert bytes(got) == lr.result_bytes(want), (got.raw, want["raw"], got.sums, want["sum"], got.extremes, want["extreme"])
    return got, want


def test_sums_carry_across_2_64_and_go_negative_in_any_order(product_lib):
    what = lr.CARRIED
    used = [3, -7, 0, 12, 1, 5, -2, 0, 0]
    big = (1 << 60) - 1
    ranks = [[big, -big, 5, 2 ** 59, -1, 0, 1, 0, 0] for _ in range(40)]                   # 40 * (2^60 - 1) > 2^64: lo wraps twice
    ranks += [[(1 << 64) - 1, -(1 << 64), -(1 << 70) - 3, 1, -1, 1 << 90, -(1 << 90), 0, 0],   # a rank whose own sums span both words
              [1, -1, (1 << 70) + 2, -(1 << 64), 1 << 64, 1, 1, 0, 0]]
    words = [_words(n=3, bits={0: _bits(1.0)}) for _ in ranks]
    got, want = _compose(product_lib, words, ranks, what, used)
    assert want["raw"][0] == 40 * big + (1 << 64) and want["raw"][0] >> 64 >= 3            # carried out of lo
    assert want["raw"][1] < -(1 << 65) and want["raw"][2] == 40 * 5 - 1 and want["raw"][4] == (1 << 64) - 41
    assert got.raw == dict(zip(lr.SUMS, want["raw"])) and got.n == 3 * len(ranks)
    assert got.exact("momentum_x") == want["raw"][1] * ledger.Fraction(2) ** (-7 - 60)
    rng = random.Random(5)
    for _ in range(4):                                                                    # ranks in any order
        order = list(range(len(ranks)))
        rng.shuffle(order)
        again = ledger.compose([words[i] for i in order], [ranks[i] for i in order], ledger.ledger_spec(what, used), lib=product_lib)
        assert bytes(again) == bytes(got)
    # sums of a group that is not asked for are ignored and come back as 0 with exponent 0
    assert got.raw["volume"] == 0 and got.exponents["volume"] == 0
    junk = [r[:7] + [99, -99] for r in ranks]
    assert bytes(ledger.compose(words, junk, ledger.ledger_spec(what, used), lib=product_lib)) == bytes(got)


def test_an_empty_rank_changes_nothing(product_lib):
    what = lr.ALL
    used = [0] * 9
    full = _words(n=5, n_outside=2, bits={0: _bits(0.75)}, keys={0: _key(0, 2.5, 3), 3: _key(3, -0.25, 4), 7: _key(7, 990.0, 1)})
    sums = [11, -12, 13, -14, 15, 16, -17, 18, 19]
    a, _ = _compose(product_lib, [full], [sums], what, used)
    b, _ = _compose(product_lib, [lr.empty_words(), full, lr.empty_words()], [[0] * 9, sums, [0] * 9], what, used)
    assert bytes(a) == bytes(b) and a.n == 5 and a.n_outside == 2
    assert a.extreme("max_speed2") == (2.5, 3) and a.extreme("min_y") == (-0.25, 4) and a.extreme("min_density") == (990.0, 1)
    assert a.extreme("max_x") == (0.0, ffi.LEDGER_NO_ID) and a.extreme("max_h") == (0.0, ffi.LEDGER_NO_ID)
    # nothing but empty ranks: zeros, no ids; the automatic exponent of nothing is 0
    spec, folded = ledger.fold([lr.empty_words()] * 3, what, lib=product_lib)
    assert list(spec.exponent) == [0] * 9 and folded.as_tuple() == lr.empty_words()
    none, _ = _compose(product_lib, [lr.empty_words()] * 3, [[0] * 9] * 3, what, [0] * 9)
    assert none.n == 0 and all(v == (0.0, ffi.LEDGER_NO_ID) for v in none.extremes.values()) and not any(none.raw.values())
    assert math.isnan(none.centre_of_mass[0])


def test_equal_extremes_go_to_the_smaller_id_and_minus_zero_lies_below_zero(product_lib):
    what = lr.CARRIED
    used = [0] * 9
    zero = [0] * 9
    r0 = _words(n=2, keys={0: _key(0, 4.0, 70), 1: _key(1, -1.5, 70), 2: _key(2, 0.0, 9), 3: _key(3, 0.0, 9), 5: _key(5, 1.0, 70), 6: _key(6, 1.0, 70)})
    r1 = _words(n=2, keys={0: _key(0, 4.0, 12), 1: _key(1, -1.5, 12), 2: _key(2, -0.0, 3), 3: _key(3, -0.0, 30), 5: _key(5, 1.0, 71), 6: _key(6, 1.0, 69)})
    for order in ([r0, r1], [r1, r0]):
        got, _ = _compose(product_lib, order, [zero, zero], what, used)
        assert got.extreme("max_speed2") == (4.0, 12) and got.extreme("min_x") == (-1.5, 12)          # the smaller id on the other rank
        assert got.extreme("min_mass") == (1.0, 70) and got.extreme("max_mass") == (1.0, 69)
        v, i = got.extreme("max_x")
        assert (v, i) == (0.0, 9) and math.copysign(1.0, v) == 1.0                                 # +0 is the maximum though its id is larger
        v, i = got.extreme("min_y")
        assert (v, i) == (0.0, 30) and math.copysign(1.0, v) == -1.0                               # -0 the minimum
    # ord orders like the values
    vals = np.array([-np.inf, -3.0e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3.0e38, np.inf], f32)
    o = lr.ord_f32(vals)
    assert np.all(np.diff(o) > 0)
    assert all(lr.unord(int(a)) == float(v) for a, v in zip(o, vals))


def test_the_smallest_offender_across_ranks_and_its_sentence(product_lib):
    what = lr.CARRIED | lr.STEP
    exps = [None] * 9
    ranks = [_words(first_bad=(900 << 8) | lr.BAD_VX, n=4), _words(n=2), _words(first_bad=(17 << 8) | lr.BAD_RHO_SIGN, n=4),
             _words(first_bad=(17 << 8) | lr.BAD_TERM + 5, n=1)]
    kind, sentence, _ = lr.fold(ranks, what, exps)
    assert kind == "refused" and "(particle i=17;" in sentence and "before the first step" in sentence
    for order in (ranks, ranks[::-1]):
        with pytest.raises(ffi.SphError) as e:
            ledger.fold(order, what, lib=product_lib)
        assert e.value.status == 1 and str(e.value).endswith(sentence)
    with pytest.raises(ffi.SphError):                                  # compose refuses words that name an offender
        ledger.compose(ranks, [[0] * 9] * 4, ledger.ledger_spec(what, [0] * 9), lib=product_lib)
    # every reason has its sentence; an explicit exponent is named
    for why, word in ((lr.BAD_M, "the mass is not finite"), (lr.BAD_Y, "the y is not finite"), (lr.BAD_P, "the pressure is not finite"),
                      (lr.BAD_H, "the smoothing length is not finite"), (lr.BAD_SPEED2, "squared speed")):
        w = [_words(first_bad=(2 ** 32 - 2 << 8) | why, n=1)]
        with pytest.raises(ffi.SphError) as e:
            ledger.fold(w, what, lib=product_lib)
        assert str(e.value).endswith(lr.fold(w, what, exps)[1]) and word in str(e.value) and "i=4294967294)" in str(e.value)
    w = [_words(first_bad=(3 << 8) | lr.BAD_TERM + 6, n=1)]
    for ex in (None, -4):
        exps6 = [None] * 6 + [ex, None, None]
        with pytest.raises(ffi.SphError) as e:
            ledger.fold(w, what, exps6, lib=product_lib)
        assert str(e.value).endswith(lr.fold(w, what, exps6)[1]) and "sum 6 (angular)" in str(e.value)
        assert ("2^-4" in str(e.value)) == (ex is not None)
    # a short msg truncates and terminates; no msg at all is allowed
    spec = ledger.ledger_spec(what)
    arr = (ffi.SphLedgerWords * 4)(*[ffi.SphLedgerWords.from_tuple(r) for r in ranks])
    msg = C.create_string_buffer(b"\xff" * 32, 32)
    assert product_lib.ledger_fold_words(4, arr, C.byref(spec), None, msg, 12) == 1
    assert msg.raw[:12] == sentence.encode()[:11] + b"\0" and msg.raw[12:] == b"\xff" * 20
    assert product_lib.ledger_fold_words(4, arr, C.byref(spec), None, None, 0) == 1
    assert product_lib.ledger_fold_words(4, arr, C.byref(spec), None, msg, 0) == 1


def test_automatic_exponents(product_lib):
    what = lr.CARRIED | lr.STEP
    cases = [(0.0, 0), (1.0, 1), (0.999, 0), (0.5, 0), (0.49999, -1), (3.0, 2), (4.0, 3), (2.0 ** -200, -199), (2.0 ** -201, -200), (2.0 ** -202, -200),
             (5e-324, -200), (2.0 ** 199, 200), (math.nextafter(2.0 ** 200, 0.0), 200)]
    for m, want in cases:
        ranks = [_words(n=1, bits={4: _bits(m / 3)}), _words(n=1, bits={4: _bits(m), 8: _bits(m)}), _words(n=0)]
        spec, folded = ledger.fold(ranks, what, [7, None, None, None, None, None, None, None, None], lib=product_lib)
        kind, used, f = lr.fold(ranks, what, [7] + [None] * 8)
        assert kind == "ok" and list(spec.exponent) == used and folded.as_tuple() == f
        assert spec.exponent[4] == spec.exponent[8] == want, (m, want)
        assert spec.exponent[0] == 7 and spec.exponent[1] == 0                        # explicit: left alone; nothing seen: 0
        if m > 0:
            assert m < 2.0 ** want and (want == -200 or m >= 2.0 ** (want - 1))
    # a sum that is not asked for gets 0, whatever the caller wrote there
    spec, _ = ledger.fold([_words(n=1, bits={7: _bits(8.0)})], lr.CARRIED, [1] * 7 + [55, 1000], lib=product_lib)
    assert list(spec.exponent) == [1] * 7 + [0, 0]
    # above the range: refused, on every rank the same
    for m, need in ((2.0 ** 200, 201), (1e300, 997)):
        ranks = [_words(n=1), _words(n=1, bits={5: _bits(m)})]
        kind, sentence, _ = lr.fold(ranks, what)
        assert kind == "refused" and f"sum 5 (kinetic) needs the exponent {need} (at most 200)" in sentence
        for order in (ranks, ranks[::-1]):
            with pytest.raises(ffi.SphError) as e:
                ledger.fold(order, what, lib=product_lib)
            assert e.value.status == 1 and str(e.value).endswith(sentence)


def test_resolved_doubles_round_to_nearest_even(product_lib):
    what = lr.CARRIED
    ints = [0, 1, -1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, -(2 ** 53 + 1), -(2 ** 53 + 3), 2 ** 54 + 2, 2 ** 54 + 6, 2 ** 64 - 1, 2 ** 64, 2 ** 64 + 2 ** 11,
            2 ** 64 + 2 ** 11 + 1, 3 * 2 ** 64 + 3 * 2 ** 11, 2 ** 100 + 2 ** 47, 2 ** 100 + 2 ** 47 + 1, 2 ** 100 + 3 * 2 ** 47, -(2 ** 100 + 3 * 2 ** 47), 2 ** 91 - 1,
            -(2 ** 91 - 1), 2 ** 120 - 2 ** 66, (2 ** 53 - 1) * 2 ** 40 + 2 ** 39, (2 ** 53 - 1) * 2 ** 40 + 2 ** 39 - 1, -(2 ** 126) + 1]
    rng = random.Random(11)
    ints += [rng.randrange(-2 ** 91, 2 ** 91) for _ in range(40)] + [rng.randrange(-2 ** 70, 2 ** 70) for _ in range(20)]
    halfway = [q for q in ints if q.bit_length() > 54 and abs(q) % (1 << (abs(q).bit_length() - 53)) == 1 << (abs(q).bit_length() - 54)]
    assert len(halfway) >= 6                                                               # ties are among the cases
    for e in (0, -200, 200, 13):
        for at in range(0, len(ints), 7):
            chunk = (ints[at:at + 7] + [0] * 7)[:7]
            got, want = _compose(product_lib, [_words(n=1)], [chunk + [0, 0]], what, [e] * 7 + [0, 0])
            for s in range(7):
                assert got.sums[lr.SUMS[s]] == math.ldexp(float(chunk[s]), e - 60)
    # a tie above 2^53 goes to even, in both directions
    assert float(2 ** 53 + 1) == 2.0 ** 53 and float(2 ** 53 + 3) == 2.0 ** 53 + 4


def test_refusals_of_the_host_calls(product_lib):
    ok = ffi.SphLedgerWords.from_tuple(_words(n=1))
    sums = (ffi.SphLedgerSum * 9)()
    out = ffi.SphLedgerResult()
    msg = C.create_string_buffer(256)
    spec = ledger.ledger_spec(lr.CARRIED, [0] * 9)
    assert product_lib.ledger_compose(1, C.byref(ok), sums, C.byref(spec), C.byref(out)) == 0
    assert product_lib.ledger_compose(0, C.byref(ok), sums, C.byref(spec), C.byref(out)) == 1
    assert product_lib.ledger_compose(1, None, sums, C.byref(spec), C.byref(out)) == 1
    assert product_lib.ledger_compose(1, C.byref(ok), None, C.byref(spec), C.byref(out)) == 1
    assert product_lib.ledger_compose(1, C.byref(ok), sums, None, C.byref(out)) == 1
    assert product_lib.ledger_compose(1, C.byref(ok), sums, C.byref(spec), None) == 1
    assert product_lib.ledger_fold_words(0, C.byref(ok), C.byref(spec), None, msg, 256) == 1 and b"n < 1" in msg.value
    assert product_lib.ledger_fold_words(1, None, C.byref(spec), None, msg, 256) == 1
    assert product_lib.ledger_fold_words(1, C.byref(ok), None, None, msg, 256) == 1
    for what, word in ((0, "asks for nothing"), (8, "unknown group"), (1 | 16, "unknown group")):
        bad = ledger.ledger_spec(what, [0] * 9)
        assert product_lib.ledger_fold_words(1, C.byref(ok), C.byref(bad), None, msg, 256) == 1 and word.encode() in msg.value
        assert product_lib.ledger_compose(1, C.byref(ok), sums, C.byref(bad), C.byref(out)) == 1
    auto = ledger.ledger_spec(lr.CARRIED)                               # compose wants the fold's exponents
    assert product_lib.ledger_compose(1, C.byref(ok), sums, C.byref(auto), C.byref(out)) == 1
    assert product_lib.ledger_fold_words(1, C.byref(ok), C.byref(auto), None, msg, 256) == 0 and list(auto.exponent) == [0] * 9
    for e in (201, -201):
        bad = ledger.ledger_spec(lr.CARRIED, [0, 0, e, 0, 0, 0, 0, 0, 0])
        assert product_lib.ledger_fold_words(1, C.byref(ok), C.byref(bad), None, msg, 256) == 1 and f"exponent {e}".encode() in msg.value
        assert product_lib.ledger_compose(1, C.byref(ok), sums, C.byref(bad), C.byref(out)) == 1
    step_only = ledger.ledger_spec(lr.STEP, [999] * 7 + [0, 0])         # exponents of sums that are not asked for are not looked at
    assert product_lib.ledger_compose(1, C.byref(ok), sums, C.byref(step_only), C.byref(out)) == 0 and list(out.exponent) == [0] * 9


def test_the_twin_agrees_with_itself_over_partitions():
    """The restatement's own composition: any partition of the same particles gives the same bytes."""
    rng = np.random.default_rng(3)
    n = 300
    fields = {"mass": (rng.choice([1.0, 4096.0], n) * 1e-3).astype(f32), "position": rng.uniform(-2, 2, (n, 2)).astype(f32),
              "velocity": rng.normal(0, 3, (n, 2)).astype(f32), "density": rng.uniform(900, 1100, n).astype(f32),
              "pressure": rng.uniform(0, 5000, n).astype(f32), "h2": rng.uniform(0.01, 0.05, n).astype(f32)}
    P = lr.Particles(fields, rng.permutation(n), 1000.0)
    planes = [(1.0, 0.0, 1.5), (-1.0, 0.0, 1.5), (0.0, 1.0, 1.0)]
    kind, whole = lr.ledger(P, lr.ALL, None, planes)
    assert kind == "ok" and 0 < whole["n_outside"] < n and whole["n"] == n
    perm = rng.permutation(n)
    for parts in ([perm[:100], perm[100:]], [perm[:1], perm[1:150], perm[150:150], perm[150:]]):
        kind, split = lr.ledger(P, lr.ALL, None, planes, parts)
        assert kind == "ok" and lr.result_bytes(split) == lr.result_bytes(whole)
    assert len(lr.result_bytes(whole)) == 376
    assert whole["extreme"][0][0] == float(lr.speed2(P).max()) and whole["extreme"][3][0] == float(P.y.min())
    m = sum(int(v) for v in np.trunc(P.m.astype(np.float64) * 2.0 ** (60 - whole["exponent"][0])).astype(np.int64))
    assert whole["raw"][0] == m and abs(whole["sum"][0] - float(P.m.astype(np.float64).sum())) < 1e-9
