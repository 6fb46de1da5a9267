"""sph_relay_plan (include/sph_rank_partner_search.h) simulated in numpy over byte arrays: the schedule that drives the relay of the
per-rank device search, without a device.  Every rank's plan is fetched on its own -- as every rank derives its own at run time -- and the
simulation executes them side by side: a message is what the sender's plan names, copied to where the receiver's plan puts it.

Checked in every sub-round: (a) the two ends of every pair name the same message (origin, offset, byte count: exchange's pairing rule),
(b) no message exceeds chunk_bytes, (d) a rank sends only bytes it holds.  At the end: (c) the root holds every blob / every rank holds
the root's blob; (e) all ranks have the same number of sub-rounds."""
import numpy as np
import pytest

from adaptive_sph_amd import ffi

CHUNKS = (4096, 1 << 20)


def size_sets(n, chunk):
    """blob sizes per rank: the edge sizes rotated over the ranks, so that each of them sits at every distance from every root"""
    edge = [0, 1, chunk, chunk + 1, 3 * chunk + 17]
    sets = [[edge[(r + shift) % len(edge)] for r in range(n)] for shift in range(len(edge))]
    sets.append([0] * n)
    sets.append([chunk] * n)
    return sets


def blobs_of(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=s, dtype=np.uint8) for s in sizes]


def simulate(lib, n, root, sizes, chunk, outwards):
    """-> (what every rank holds of every blob, as (data, have-mask) per origin; the number of sub-rounds; the messages sent)"""
    blobs = blobs_of(sizes, 1000 * n + root)
    plans = [ffi.relay_plan(lib, n, root, r, sizes, chunk, outwards=outwards) for r in range(n)]
    assert len({len(q) for q in plans}) == 1, [len(q) for q in plans]                                 # (e)
    origins = [root] if outwards else list(range(n))
    data = [{o: np.zeros(sizes[o], np.uint8) for o in origins} for _ in range(n)]
    have = [{o: np.zeros(sizes[o], bool) for o in origins} for _ in range(n)]
    for o in origins:
        data[o][o][:] = blobs[o]
        have[o][o][:] = True
    messages = 0
    for k in range(len(plans[0])):
        steps = [q[k] for q in plans]
        assert len({(s["round"], s["sub_round"]) for s in steps}) == 1
        for r in range(n):                                            # nothing crosses the outer edge of the row
            assert steps[r]["send"][0][2] == 0 or r > 0
            assert steps[r]["recv"][0][2] == 0 or r > 0
            assert steps[r]["send"][1][2] == 0 or r + 1 < n
            assert steps[r]["recv"][1][2] == 0 or r + 1 < n
        arriving = []
        for r in range(n - 1):                                        # the pair (r, r + 1): r's right side, r + 1's left side
            for src, s_side, dst, d_side in ((r, 1, r + 1, 0), (r + 1, 0, r, 1)):
                sent, taken = steps[src]["send"][s_side], steps[dst]["recv"][d_side]
                assert sent[2] == taken[2], (n, root, k, src, dst, sent, taken)                      # (a)
                if sent[2] == 0:
                    continue
                assert sent == taken, (n, root, k, src, dst, sent, taken)
                o, off, ln = sent
                assert ln <= chunk                                                                      # (b)
                assert off + ln <= sizes[o]
                assert have[src][o][off:off + ln].all(), (n, root, k, src, o, off, ln)               # (d)
                arriving.append((dst, o, off, data[src][o][off:off + ln].copy()))
                messages += 1
        for dst, o, off, payload in arriving:                         # (all exchanges of a sub-round read before any of them writes)
            assert not have[dst][o][off:off + len(payload)].any()     # nothing is received twice
            data[dst][o][off:off + len(payload)] = payload
            have[dst][o][off:off + len(payload)] = True
    return blobs, data, have, plans, messages


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_the_gather_brings_every_blob_to_the_root(product_lib, n, chunk):
    for root in range(n):
        for sizes in size_sets(n, chunk):
            blobs, data, have, plans, messages = simulate(product_lib, n, root, sizes, chunk, outwards=False)
            gathered = np.concatenate([data[root][o] for o in range(n)] + [np.zeros(0, np.uint8)])
            assert all(have[root][o].all() for o in range(n))
            assert np.array_equal(gathered, np.concatenate(blobs + [np.zeros(0, np.uint8)])), (n, root, sizes)   # (c) rank order
            rounds = max(root, n - 1 - root)
            want = 0
            for t in range(1, rounds + 1):
                moving = [sizes[o] for o in range(n) if abs(root - o) >= t]
                want += max(-(-s // chunk) for s in moving)
            assert len(plans[0]) == want, (n, root, sizes)
            assert messages == sum(-(-sizes[o] // chunk) * abs(root - o) for o in range(n))               # every chunk, once per hop


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_the_broadcast_brings_the_roots_blob_to_every_rank(product_lib, n, chunk):
    for root in range(n):
        for size in (0, 1, chunk, chunk + 1, 3 * chunk + 17):
            sizes = [7] * n                                          # (only the root's entry is read)
            sizes[root] = size
            blobs, data, have, plans, messages = simulate(product_lib, n, root, sizes, chunk, outwards=True)
            for r in range(n):
                assert have[r][root].all() and np.array_equal(data[r][root], blobs[root]), (n, root, size, r)    # (c)
            assert len(plans[0]) == max(root, n - 1 - root) * -(-size // chunk)
            assert messages == (n - 1) * -(-size // chunk)


def test_a_blob_of_several_chunks_takes_several_sub_rounds(product_lib):
    """three ranks, root 0: rank 2's blob of 2.5 chunks crosses rank 1; rank 1 forwards in round 2 what it took in round 1, chunk by chunk"""
    chunk = 4096
    sizes = [32, 48, 2 * chunk + 2048]
    plan1 = ffi.relay_plan(product_lib, 3, 0, 1, sizes, chunk)
    assert [(s["round"], s["sub_round"]) for s in plan1] == [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
    assert plan1[0]["send"][0] == (1, 0, 48) and plan1[0]["recv"][1] == (2, 0, chunk)
    assert plan1[1]["send"][0] == (0, 0, 0) and plan1[1]["recv"][1] == (2, chunk, chunk)
    assert plan1[2]["recv"][1] == (2, 2 * chunk, 2048)
    assert [s["send"][0] for s in plan1[3:]] == [(2, 0, chunk), (2, chunk, chunk), (2, 2 * chunk, 2048)]
    assert all(s["recv"][0][2] == 0 and s["recv"][1][2] == 0 for s in plan1[3:])
    plan0 = ffi.relay_plan(product_lib, 3, 0, 0, sizes, chunk)
    assert [s["recv"][1] for s in plan0] == [(1, 0, 48), (0, 0, 0), (0, 0, 0), (2, 0, chunk), (2, chunk, chunk), (2, 2 * chunk, 2048)]
