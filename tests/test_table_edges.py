"""The host builder (talc_table_host.h: findSlotBounded, findSlot, find, the deferred serial pass of insertAll) and
lookup_host on tables whose probe chains cross the end of the table, and on the count edges — against the oracle table.

The generator's dump here has more than 100 000 lines, so insertAll takes its parallel phase whenever more than one
thread is to be had: the last thread's range ends at the capacity, every key of the zone (PU.end_loaded_table) that
finds the last slots taken is deferred, and the serial pass puts it at the start of the table.  That keys ARE stored
below their home follows from the homes alone: more stored keys have their home in the last W slots than W."""
import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
from talc_amd import lib as T
from talc_amd.synth import Synth

W, F = 4, 48
PARALLEL_FROM = 100_000     # insertAll: n < 100000 lines run on one thread


@pytest.fixture(scope="module", params=[(k, x10) for k in (18, 21, 31) for x10 in (20, 40)], ids=lambda p: "k%d-x%d" % p)
def host_zone(request):
    k, x10 = request.param
    synth = Synth(target_kmers=110_000, k=k, seed=800 + k)
    E = PU.end_loaded_table(synth, k, x10, W, F, np.random.default_rng(1000 * k + x10))
    assert len(E.keys) > PARALLEL_FROM, len(E.keys)
    assert T.lib().omp_get_max_threads() > 1          # (the OpenMP runtime the library itself runs on: insertAll's thread count)
    return E


def test_home_mirrors_are_in_range():
    rng = np.random.default_rng(2)
    keys = rng.integers(0, 1 << 60, 100_000, dtype=np.uint64)
    for cap in (64, 132_852, (1 << 32) - 1):
        h = PU.table_home(keys, cap)
        assert h.min() >= 0 and h.max() < cap and len(np.unique(h)) > min(cap, 60_000) * 0.6
    assert PU.table_home(np.array([0], np.uint64), 1000)[0] == 0
    h = PU.count_home(keys, (1 << 16) - 1)
    assert h.min() >= 0 and h.max() < (1 << 16) and PU.count_home(np.array([0], np.uint64), 255)[0] == 0
    assert int(PU.mix64(np.array([1], np.uint64))[0]) == 0xB456BCFC34C2CB2C      # (MurmurHash3's fmix64 of 1)


def test_zone_holds_more_keys_than_slots(host_zone):
    """The reach condition, from the homes alone: per table more than W stored keys have their home in the last W slots
    (each of the W slots is some key's home), so at least F / 2 - W of them are stored after the wrap, from slot 0 on."""
    E = host_zone
    k = E.k
    m1 = np.uint64((1 << (2 * (k - 1))) - 1)
    stored = np.unique(E.keys[E.counts >= E.p.min_count])
    for name, key in (("RIGHT", stored >> np.uint64(2)), ("LEFT", stored & m1)):
        home = PU.table_home(np.unique(key), E.capacity)
        zone = home[home >= E.capacity - W]
        print("K=%d x10=%d capacity %d %s: %d keys with their home in the last %d slots, at least %d stored below it"
              % (k, E.x10, E.capacity, name, len(zone), W, len(zone) - W))
        assert len(zone) - W >= 20 and len(set(zone.tolist())) == W
        assert home.min() > 0        # ... and slot 0 is no key's home: what is stored there came over the end


def test_point_lookups_on_the_host(host_zone):
    E = host_zone
    assert len(E.ttab) == len(E.otab) > 100_000
    n = PU.check_zone_lookups(E, [("lookup_host", E.ttab.lookup_host)])
    print("queries", n)


def test_builder_semantics_through_the_dump_files(host_zone, tmp_path):
    """The same table through the text parser: size, (count, colour) of every query and build_stats equal the oracle's."""
    E = host_zone
    dump, junc = PU.junction_dump_files(E, tmp_path)
    ot = O.OracleTable(E.q, O.OracleTable.FLAT)
    ost = ot.build_from_files(dump, junc)
    with PU.table_slots_x10(E.x10):
        th = T.Table.from_files(dump, junc, E.p)
    assert th.capacity == E.capacity and len(th) == len(ot) == len(E.otab)
    assert int(th.build_stats[0]) == int(ost[0]) and int(th.build_stats[1]) == int(ost[1])
    for q in PU.zone_queries(E).values():
        oc, oj = ot.lookup_packed(q)
        ec, ej = E.otab.lookup_packed(q)
        assert (oc == ec).all() and (oj == ej).all()
        c, j = th.lookup_host(q)
        assert (c == oc).all() and (j == oj).all()


@pytest.mark.parametrize("k", [18, 21, 31])
@pytest.mark.parametrize("name", PU.COUNT_EDGES)
def test_count_edges_on_the_host(name, k):
    PU.check_count_edge(name, k, None)


def test_refill_end_cluster_keeps_the_table_and_places_the_first_keys_first():
    """PU.refill_end_cluster on a linear-probing table made here (random keys, 40 more with their home in the last 8 of
    600 slots, random insertion order): the same buckets in the same occupied slots, every key still reached from its home
    (PU.image_homes), and with the 40 first, every other key whose home is in those 8 slots is stored below it."""
    rng = np.random.default_rng(9)
    cap, w = 600, 8
    keys = np.unique(rng.integers(0, 1 << 40, 100_000, dtype=np.uint64))
    home = PU.table_home(keys, cap)
    zone = keys[home >= cap - w]
    first, others = zone[:40], zone[40:52]
    assert len(others) == 12 and len(set(PU.table_home(first, cap).tolist())) == w
    rest = keys[(home < cap - w) & (home > 0)][:200]
    tab = np.zeros(cap, PU.BUCKET)
    tab["key"] = PU.EMPTY
    every = np.concatenate([first, others, rest])
    for n, key in enumerate(rng.permutation(every).tolist()):
        j = int(PU.table_home(key, cap)[0])
        while tab["key"][j] != PU.EMPTY:
            j = (j + 1) % cap
        tab[j] = (key, [n + 1, 0, 0, 0], [0, 0, 0, 0])
    out = PU.refill_end_cluster(tab, set(first.tolist()))
    assert sorted(out.tobytes()[i:i + 32] for i in range(0, 32 * cap, 32)) == sorted(tab.tobytes()[i:i + 32] for i in range(0, 32 * cap, 32))
    slots, got, homes = PU.image_homes(out, "refilled")
    below = set(got[homes > slots].tolist())
    assert set(others.tolist()) <= below and out["key"][0] != PU.EMPTY
