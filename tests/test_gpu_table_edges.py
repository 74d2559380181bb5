"""-m gpu: every table prober where a probe chain crosses the end of the table.

Linear probing is written out in probe_bucket / probe_bucket_from (talc_kernels_probe.h), build_claim_bucket and
dev_find_slot (talc_kernels_build.h), fast_forward_dir and walk_record (talc_kernels_search.h), count_insert and
k_count_rehash (talc_kernels_count.h) and the host builder; each has its own wrap at the last slot, and on the
generator's tables no chain ever reaches it.  Here the tables are end-loaded (PU.end_loaded_table): filler k-mers whose
RIGHT key or LEFT key has its home in the last W slots, more of them than W, so most are stored at the start of the
table, and the generator's own keys with their home there are pushed over the end with them.

What shows that the wrapped paths are taken are the reach conditions, asserted from the exported image and the homes
alone (PU.zone_reach, never from a result under test) and printed per table: keys stored below their home per
direction, the generator's own among them, and the counter's last-slot keys per capacity stage.  Which keys go over the
end depends on the order the CASes land in, so every key of the zone is looked up; no placement is assumed.

K = 18, 21, 31; TALC_TABLE_SLOTS_X10 = 20, 40; tables built on the host and uploaded, and built on the device.  Counts and
colours are compared with tolerance 0.  The walk-record check runs at both densities for K = 21 and at x10 = 20 for K = 18
and 31."""
import numpy as np
import pytest

import kmer_ref as R
import oracle_lib as O
import parity_util as PU
import test_gpu_edge_lane as EL
import test_gpu_structure as TS
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

W, F = 4, 48                 # the zone of the lookup / builder / derived-table / coverage tables
WALK_W, WALK_F = 16, 192     # ... of the tables the search walks: the generator's own keys of the last 16 slots
COMBOS = [(k, x10, built) for k in (18, 21, 31) for x10 in (20, 40) for built in ("host", "device")]


def _id(c):
    return "k%d-x%d-%s" % c


class _Image:
    """The bucket tables a host-built table had before its upload, made from the image after it with the degree bits
    taken off (a host-built table has no image before).  So for the host-built tables the before / after assertions of
    check_indegree_bits_of_every_right_bucket hold by construction and carry no weight; its comparison of the degree
    bits with bucket_dicts does.  The device-built tables have a real image before the upload."""

    def __init__(self, after):
        self.right, self.left = after.right.copy(), after.left.copy()
        occ = self.right["key"] != PU.EMPTY
        self.right["key"][occ] &= PU.KEY_MASK

    def free(self):
        pass


def _upload_with_images(E, built, dicts=True):
    before = PU.DeviceImage(E.ttab) if built == "device" else None      # (a host-built table has no image yet)
    E.upload(0)
    E.after = PU.DeviceImage(E.ttab)
    E.before = before or _Image(E.after)
    if dicts:                                                            # (what the derived-table checkers compare with)
        E.right, E.left = PU.bucket_dicts(E.keys, E.counts, E.k, E.p.min_count)


def _reach(E, w, genuine=(None, None)):
    """The reach conditions of both tables of E (image and homes alone), printed."""
    out = {}
    for name, tab, gen in (("RIGHT", E.after.right, genuine[0]), ("LEFT", E.after.left, genuine[1])):
        r = PU.zone_reach(tab, w, gen, "%s %s" % (E.name, name))
        print("%s capacity %d %s: %d keys with their home in the last %d slots, %d keys stored below their home (the generator's own: %d), the last of them in slot %d"
              % (E.name, E.capacity, name, r["in_zone"], w, r["below"], r["genuine_below"], r["last_wrapped_slot"]))
        out[name] = r
    return out


@pytest.fixture(scope="module", params=COMBOS, ids=_id)
def zone(request):
    k, x10, built = request.param
    synth = Synth(target_kmers=60_000, k=k, seed=700 + k)
    E = PU.end_loaded_table(synth, k, x10, W, F, np.random.default_rng(100 * k + x10), device=0 if built == "device" else None)
    E.name, E.built = _id(request.param), built
    _upload_with_images(E, built)
    yield E
    E.before.free()
    E.after.free()
    E.ctx.close()
    E.ttab.close()


# ---------------------------------------------------------------- 2. reach
def test_chains_cross_the_end_of_both_tables(zone):
    """Also pins PU.table_home against the product: in the exported image every key is reached from its home over
    occupied slots, with the wrap (PU.image_homes)."""
    r = _reach(zone, W)
    for name in ("RIGHT", "LEFT"):
        assert r[name]["in_zone"] > W and r[name]["below"] >= 20, (zone.name, name, r[name])
    assert zone.ttab.capacity == zone.capacity == len(zone.after.right)


# ---------------------------------------------------------------- 3a. lookups
def test_point_lookups(zone):
    E = zone
    assert len(E.ttab) == len(E.otab)
    n = PU.check_zone_lookups(E, [("lookup", E.ttab.lookup), ("lookup_host", E.ttab.lookup_host)])
    print(E.name, "queries", n)


def test_successor_lookups(zone):
    E = zone
    n = 0
    for direction, kms in PU.zone_successor_queries(E):
        g4c, g4j = E.ttab.next_counts(kms, direction)
        some = 0
        for i, km in enumerate(kms.tolist()):
            e4c, e4j = E.otab.next_counts(PU.kmer_text(km, E.k), direction)
            assert e4c.tolist() == g4c[i].tolist() and e4j.tolist() == g4j[i].tolist(), (E.name, direction, i)
            some += int(e4c.any())
        assert some >= 4 * (F // 2) and some < len(kms)          # the fillers' buckets are there, the absent keys' are not
        n += len(kms)
    # ... and of every stored k-mer of the dump, a sample (both directions)
    sample = E.keys[E.counts >= E.p.min_count][:: 97]
    for direction in (0, 1):
        g4c, g4j = E.ttab.next_counts(sample, direction)
        for i, km in enumerate(sample.tolist()):
            e4c, e4j = E.otab.next_counts(PU.kmer_text(km, E.k), direction)
            assert e4c.tolist() == g4c[i].tolist() and e4j.tolist() == g4j[i].tolist(), (E.name, direction, i)
    print(E.name, "successor queries of the zone", n, "of the dump", 2 * len(sample))


# ---------------------------------------------------------------- 3b. builder semantics
def test_builder_semantics_through_the_dump_files(zone, tmp_path):
    """The end-loaded dump (fillers with a line below MIN_COUNT before and a duplicate after the kept one; junction
    lines over fillers and their reverse complements, colours at, above and below colouredCountThr and negative;
    homopolymers) through the text route of this table's builder: size, build_stats and every query equal the oracle's."""
    E = zone
    dump, junc = PU.junction_dump_files(E, tmp_path)
    ot = O.OracleTable(E.q, O.OracleTable.FLAT)
    ost = ot.build_from_files(dump, junc)
    with PU.table_slots_x10(E.x10):
        tf = T.Table.from_files(dump, junc, E.p, device=0 if E.built == "device" else None)
    assert tf.capacity == E.capacity and len(tf) == len(ot) == len(E.otab) == len(E.ttab)
    assert int(tf.build_stats[0]) == int(ost[0]) and int(tf.build_stats[1]) == int(ost[1])
    hom = np.array([int(d * E.k, 4) for d in "0123"], dtype=np.uint64)
    oc, oj = E.otab.lookup_packed(hom)
    assert oc.tolist() == [0, 50, 50, 50] and (oj == 0).all()     # stored but for poly-A, coloured by their junction lines, de-coloured
    parts = PU.zone_queries(E)
    tf.upload(0)
    for q in list(parts.values()) + [hom]:
        oc, oj = ot.lookup_packed(q)
        ec, ej = E.otab.lookup_packed(q)
        assert (oc == ec).all() and (oj == ej).all()
        for fn in (tf.lookup_host, tf.lookup, E.ttab.lookup):
            c, j = fn(q)
            assert (c == oc).all() and (j == oj).all(), (E.name, fn)
    tf.close()


# ---------------------------------------------------------------- 3c. derived tables: the checkers of test_gpu_derived_tables
def test_indegree_bits_on_an_end_loaded_table(zone):
    PU.check_indegree_bits_of_every_right_bucket(zone)


def test_walk_records_on_an_end_loaded_table(zone):
    """Every walk record against the plain walk: at both densities for K = 21, at x10 = 20 for K = 18 and 31 (the other four
    tables pass through: this check walks every stored key in Python, and the module has a time to keep)."""
    if zone.k == 21 or zone.x10 == 20:
        PU.check_every_walk_record_equals_the_plain_walk(zone)


def test_presence_filter_on_an_end_loaded_table(zone):
    PU.check_presence_filter_has_no_false_negative(zone)


def test_image_export_and_import_of_an_end_loaded_table(zone):
    PU.check_image_exported_after_an_upload_imports_to_the_same_table(zone)


# ---------------------------------------------------------------- 3d. coverage and structure
def _zone_reads(E, rng):
    """Reads of the zone's k-mers, flanked along the graph (PU.flank): every filler and absent k-mer alone (K bases: the
    right degree comes from the k-mer's own probe) and in the middle of 3 K - 2 bases; the chained pairs — a LEFT
    filler and the RIGHT filler that follows it at the next position, whose RIGHT bucket, stored after the wrap,
    publishes the right degree of the position before; and every filler beside an N."""
    k = E.k
    m1 = (1 << (2 * (k - 1))) - 1
    reads = []
    for x in np.concatenate([E.fill, E.absent_r, E.absent_l]).tolist():
        t = PU.kmer_text(x, k)
        reads.append(t)
        reads.append(PU.flank(E.left, x >> 2, 0, k, k - 1, rng) + t + PU.flank(E.right, x & m1, 1, k, k - 1, rng))
    n_chain = 0
    for g, f in E.chain:
        pair = PU.kmer_text(g, k) + "ACGT"[f & 3]
        assert pair[1:] == PU.kmer_text(f, k)
        reads += [pair, PU.flank(E.left, g >> 2, 0, k, 5, rng) + pair + PU.flank(E.right, f & m1, 1, k, 5, rng), "N" + pair + "N" + pair]
        n_chain += 3
    return reads, n_chain


def test_coverage_degrees_and_structure_of_zone_reads(zone):
    E = zone
    reads, n_chain = _zone_reads(E, np.random.default_rng(4))
    assert n_chain >= 6
    # from the image: of the chained pairs, those whose shared bucket (the RIGHT key of the pair's second k-mer) is stored
    # below its home, so that cov_count publishes the first position's right degree from a wrapped bucket
    slots, keys, home = PU.image_homes(E.after.right, E.name)
    below = set(keys[home > slots].tolist())
    wrapped = sum(1 for g, f in E.chain if (f >> 2) in below)
    print("%s: %d chained pairs, the shared RIGHT bucket of %d stored below its home" % (E.name, len(E.chain), wrapped))
    assert len(E.chain) > W and wrapped >= 1
    bases, offs = PU.pack_reads(reads)
    b = E.ctx.batch(bases, offs)
    b.coverage()
    c, j, ko, nin = b.fetch_coverage()
    b.close()
    hits = 0
    for i, s in enumerate(reads):
        wc, wj, wn = E.otab.coverage(s)
        got_c, got_j = c[int(ko[i]):int(ko[i + 1])], j[int(ko[i]):int(ko[i + 1])]
        assert (got_c == wc).all() and (got_j == wj).all() and wn == nin[i], (E.name, i, s)
        hits += int((wc > 0).sum())
    assert hits >= 2 * F + 2 * n_chain
    # degrees (fetch_coverage_degrees against getOutDegree) and everything fetch_structure returns
    facts = TS._compare_case(E, reads, "%s zone reads" % E.name)
    assert sum(int((f["cov"] > 0).sum() >= 2) for f in facts) >= n_chain


# ---------------------------------------------------------------- 3e. the search walks through wrapped keys
def _transcripts(synth):
    """The generator's transcripts: error-free short reads longer than any of them are whole transcripts."""
    bases, offs = synth.short_reads(0, 4000, length=1_000_000, sub_rate=0.0)
    return sorted(set(PU.seqs_of(bases, offs)))


def _noisy(synth, s, rng):
    """The generator's read model (makeRead: a deletion, an insertion before the base, or a substitution per base, at
    the generator's rates) on the stretch s.  Written out here, not the generator's own routine, which draws its
    positions itself and cannot be made to cover a chosen k-mer; the reads only have to bear errors around the zone's
    keys, and both sides correct the same reads."""
    ps, pi, pd = synth.spec.sub_rate, synth.spec.ins_rate, synth.spec.del_rate
    out = []
    for ch in s:
        r = rng.random()
        if r < pd:
            continue
        if r < pd + pi:
            out.append("ACGT"[int(rng.integers(0, 4))])
        if pd + pi <= r < pd + pi + ps:
            ch = "ACGT"[("ACGT".index(ch) + 1 + int(rng.integers(0, 3))) % 4]
        out.append(ch)
    return "".join(out)


class _Stretches:
    """What edge_reads asks of a generator: error-free stretches, here those chosen around the zone's keys."""

    def __init__(self, seqs):
        self.seqs = seqs

    def short_reads(self, first, n, length=0, sub_rate=0.0):
        return PU.pack_reads([self.seqs[(first + i) % len(self.seqs)] for i in range(n)])


@pytest.fixture(scope="module", params=COMBOS, ids=_id)
def walked(request):
    """An end-loaded table whose zone (the last 16 slots) is the home of generator keys as well — the first generator
    seed that gives at least 6 per direction, which the homes alone decide, before anything is built — with 96 fillers
    per direction piled onto the same slots; the reads are drawn from the transcripts that hold those keys.

    A host builder inserts in dump order, fillers first, so every generator key of the zone goes over the end.  The
    device builder gives every line a thread of one launch and the first CAS on a slot takes it: left to itself it keeps
    the generator's keys, one probe from their home, in the zone and sends fillers over the end.  So the device-built
    table's image is taken before the upload, the run of buckets that crosses the end is filled again with the fillers'
    buckets first (PU.refill_end_cluster: the placement the builder gives when the fillers' CASes land first; the
    buckets are the builder's own), and the table the tests use is that image imported.  Either way the placement is
    fixed, and test_generator_keys_are_pushed_over_the_end reads it from the image after the upload."""
    k, x10, built = request.param
    m1 = np.uint64((1 << (2 * (k - 1))) - 1)
    found = []

    def admit(base_keys, base_counts, capacity):
        stored = base_keys[base_counts >= T.default_params(k=k).min_count]
        stored = stored[~np.isin(stored, [int(d * k, 4) for d in "0123"])]       # (the generator's own: not the homopolymers added)
        found[:] = [set(key[PU.table_home(key, capacity) >= capacity - WALK_W].tolist())
                    for key in (np.unique(stored >> np.uint64(2)), np.unique(stored & m1))]
        return min(len(found[0]), len(found[1])) >= 6

    for seed in range(900 + k, 960 + k):
        synth = Synth(target_kmers=60_000, k=k, seed=seed)
        E = PU.end_loaded_table(synth, k, x10, WALK_W, WALK_F, np.random.default_rng(seed), device=0 if built == "device" else None, colour=False,
                                admit=admit)
        if E is not None:
            break
    else:
        raise AssertionError("no generator seed with 6 keys per direction in the zone")
    gen = list(found)
    if built == "device":
        img = PU.DeviceImage(E.ttab)
        img.right = PU.refill_end_cluster(img.right, set((E.fill >> np.uint64(2)).tolist()))
        img.left = PU.refill_end_cluster(img.left, set((E.fill & m1).tolist()))
        img.store()
        placed = T.Table.import_device(E.p, E.capacity, len(E.ttab), img.right_ptr.value, img.left_ptr.value, 0)
        img.free()
        E.ttab.close()
        E.ttab = placed
    E.name, E.built, E.genuine = _id(request.param) + "-seed%d" % seed, built, gen
    _upload_with_images(E, built, dicts=False)
    # stretches of the transcripts around every occurrence of a zone key: the key 30 bases from the start, 30 from the
    # end, and in the middle
    rng = np.random.default_rng(seed + 1)
    stretches, noisy = [], []
    tx = _transcripts(synth)
    for key in sorted(gen[0] | gen[1]):
        text = PU.kmer_text(key, k - 1)
        for t in tx:
            at = t.find(text)
            while at >= 0:
                for lo, hi in ((at - 30, at + 700), (at - 700, at + k + 29), (at - 350, at + 350)):
                    s = t[max(0, lo):max(0, hi)]
                    if len(s) >= 6 * k:
                        stretches.append(s)
                        noisy += [_noisy(synth, s, rng) for _ in range(2)]
                at = t.find(text, at + 1)
    E.stretches, E.noisy = stretches, noisy
    yield E
    E.before.free()
    E.after.free()
    E.ctx.close()
    E.ttab.close()


def test_generator_keys_are_pushed_over_the_end(walked):
    r = _reach(walked, WALK_W, walked.genuine)
    for name in ("RIGHT", "LEFT"):
        assert r[name]["genuine_below"] >= 3 and r[name]["below"] >= 20, (walked.name, name, r[name])
    assert len(walked.stretches) >= 12 and len(walked.noisy) == 2 * len(walked.stretches)


def _zone_read_set(E):
    eb, eo = EL.edge_reads(_Stretches(E.stretches), 2 * len(E.stretches), E.k, seed=3)
    reads = E.noisy + PU.seqs_of(eb, eo)
    return PU.pack_reads(reads)


@pytest.mark.parametrize("setting", ["TALC_WALK=1", "TALC_WALK=0", "TALC_TEST_EDGE_LANE=1", "TALC_TEST_EDGE_LANE=0", "TALC_TEST_TINY_CAPS=1"])
def test_correction_through_wrapped_keys(walked, setting, monkeypatch):
    """Error-bearing reads (the generator's read model) and edge reads (test_gpu_edge_lane.edge_reads) over the
    transcripts' stretches that hold the zone's keys, against the oracle, under the switches that choose the prober: walk
    records or the per-step form, the fused edge lane or the separate calls, and the retry pass."""
    E = walked
    bases, offs = _zone_read_set(E)
    name, value = setting.split("=")
    monkeypatch.setenv(name, value)
    ttab = E.ttab
    if name == "TALC_WALK":
        # read by the upload: the image of the fixture's table, imported and uploaded under the switch.  The bucket tables
        # it then has are that image byte for byte, so the reach conditions asserted on it hold for this table too.
        ttab = T.Table.import_device(E.p, E.capacity, len(E.ttab), E.after.right_ptr.value, E.after.left_ptr.value, 0)
        ttab.upload(0)
        again = PU.DeviceImage(ttab)
        assert again.right.tobytes() == E.after.right.tobytes() and again.left.tobytes() == E.after.left.tobytes()
        again.free()
        assert (ttab.device_bytes < E.ttab.device_bytes) == (value == "0")
    pair = PU.EndLoaded()
    pair.otab, pair.p, pair.ttab = E.otab, E.p, ttab
    pair.ctx = T.Context(ttab, E.p, 0)                              # (the other switches are read by the context)
    bad, (so, o_st), _ = PU.compare_correction(pair, bases, offs, nthreads=16)
    t = pair.ctx.timing()
    print("%s %s: %d reads, corrected %d, trail steps %d, retried %d" % (E.name, setting, len(so), int((np.asarray(o_st) == 0).sum()), t.n_trail_steps, t.n_retried))
    assert not bad, (E.name, setting, bad[:5])
    assert int((np.asarray(o_st) == 0).sum()) > len(so) // 2 and t.n_trail_steps > 0
    if name == "TALC_TEST_TINY_CAPS":
        assert t.n_retried > 0
    pair.ctx.close()
    if ttab is not E.ttab:
        ttab.close()


def test_trace_of_a_read_through_a_wrapped_key(walked):
    E = walked
    bases, offs = PU.pack_reads(E.noisy[:4])
    for idx in (0, 3):
        assert PU.first_trace_diff(E, bases, offs, idx) is None


# ---------------------------------------------------------------- 3f. the counter
STAGE_BITS = 20     # the keys' hash has its low 20 bits set (or all but the lowest): the last slot or the one before it
                    # of every capacity from 2^16 to 2^20


def _last_slot_kmers(k, n, rng):
    """Random k-mers by rejection with count_home(km, 2^20 - 1) the last slot, and as many with the slot before it."""
    full = (1 << STAGE_BITS) - 1
    got = {full: [], full - 1: []}
    while min(len(v) for v in got.values()) < n:
        km = np.unique(rng.integers(0, 1 << (2 * k), 8_000_000, dtype=np.uint64))
        h = PU.count_home(km, full)
        for want, v in got.items():
            v += km[h == want].tolist()
    return np.array(got[full][:n] + got[full - 1][:n], dtype=np.uint64)


def _capacity_stages(batches, k, expected_distinct=1):
    """The capacities the counter passes through for these batches, by its growth rule (talc_counter_add: before a batch
    whose windows could pass load 0.7 the exact number of distinct k-mers is read; the table doubles until that number
    plus the batch's windows fit).  A mirror that nothing pins against the product (the counter does not tell its
    capacity): the stage figures printed and asserted rest on it.  The coverage does not: the keys' hashes have their low
    20 bits set, so their home is the last slot of whichever power of two up to 2^20 the table has."""
    cap = 1 << 16
    while expected_distinct > 0.7 * cap:
        cap *= 2
    stages, known, since, seen = [cap], 0, 0, []
    for bases, offs in batches:
        wins = int(np.maximum(np.diff(offs.astype(np.int64)) - k + 1, 0).sum())
        if known + since + wins > 0.7 * cap:
            known = len(np.unique(np.concatenate(seen))) if seen else 0
            since = 0
            if known + wins > 0.7 * cap:
                while known + wins > 0.7 * cap:
                    cap *= 2
                stages.append(cap)
        since += wins
        seen.append(R.count(bases, offs, k)[0])
    return stages


def test_count_home_mirror_against_the_counters_compaction():
    """PU.count_home against the product: a nearly empty counter (400 k-mers in 65 536 slots: each in its home slot,
    but for a collision or two) is fetched in slot order within every block of 4 096 slots a wave compacts
    (k_count_compact), so within a block the fetched keys' homes ascend.  A wrong mirror gives random order: half the
    neighbours descend."""
    k = 21
    rng = np.random.default_rng(12)
    kms = np.unique(rng.integers(0, 1 << (2 * k), 400, dtype=np.uint64))
    bases, offs = PU.pack_reads([PU.kmer_text(x, k) for x in kms.tolist()])
    c = T.KmerCounter(T.default_params(k=k), 0, 1)
    c.add(bases, offs)
    got, cnt = c.fetch(1)
    c.close()
    assert sorted(got.tolist()) == kms.tolist() and (cnt == 1).all()
    home = PU.count_home(got, (1 << 16) - 1)
    same_block = (home[1:] >> 12) == (home[:-1] >> 12)
    descend = int(((home[1:] < home[:-1]) & same_block).sum())
    print("count_home mirror: %d neighbours in one block, %d descend" % (int(same_block.sum()), descend))
    assert int(same_block.sum()) > 300 and descend <= 4


@pytest.mark.parametrize("k", [21, 31])
def test_counter_with_keys_of_the_last_slot_at_every_capacity(k):
    """K-base reads whose k-mers have their home in the last slot (or the one before) of every capacity from 2^16 to
    2^20, 1 to 5 times each, mixed into short reads that make the table grow: count_insert's and k_count_rehash's
    `& mask` at the last slot, at every stage."""
    rng = np.random.default_rng(k)
    zone = _last_slot_kmers(k, 40, rng)
    synth = Synth(target_kmers=150_000, k=21, seed=77)
    sb, so = synth.short_reads(0, 4400, length=150, sub_rate=0.005, n_rate=0.001)
    short = PU.seqs_of(sb, so)
    texts = [PU.kmer_text(x, k) for x in zone.tolist()]
    reps = rng.integers(1, 6, len(zone))
    # batch 0: every zone k-mer once, into the 64 K-slot table; then the short reads in batches of 550 with the
    # remaining repeats spread over them
    later = [t for t, r in zip(texts, reps.tolist()) for _ in range(r - 1)]
    batches = [PU.pack_reads(texts)]
    for b in range(8):
        recs = short[550 * b:550 * (b + 1)] + later[b::8]
        order = rng.permutation(len(recs))
        batches.append(PU.pack_reads([recs[i] for i in order]))
    all_bases, all_offs = PU.pack_reads([PU.seqs_of(*b) for b in batches][0] + [s for b in batches[1:] for s in PU.seqs_of(*b)])
    want_k, want_c = R.count(all_bases, all_offs, k)
    stages = _capacity_stages(batches, k)
    for cap in stages:
        h = PU.count_home(zone, cap - 1)
        print("K=%d counter capacity 2^%d: %d keys with their home in the last slot, %d in the one before" % (k, cap.bit_length() - 1, int((h == cap - 1).sum()), int((h == cap - 2).sum())))
        assert int((h == cap - 1).sum()) >= 40 and int((h == cap - 2).sum()) >= 40
    assert stages[0] == 1 << 16 and len(stages) >= 4 and stages[-1] <= 1 << STAGE_BITS, stages
    p = T.default_params(k=k)
    c = T.KmerCounter(p, 0, 1)
    for bases, offs in batches:
        c.add(bases, offs)
    st = c.stats()
    k1, c1 = c.fetch(1)
    o = np.argsort(k1, kind="stable")
    assert np.array_equal(k1[o], want_k) and np.array_equal(c1[o], want_c)
    at = np.searchsorted(want_k, np.sort(zone))
    assert sorted(want_c[at].tolist()) == sorted(reps.tolist())       # (the reference holds the zone's k-mers with their repeats)
    k2, c2 = c.fetch(2)
    o = np.argsort(k2, kind="stable")
    keep = want_c >= 2
    assert np.array_equal(k2[o], want_k[keep]) and np.array_equal(c2[o], want_c[keep])
    assert st == (int(want_c.sum()), len(want_k), int(keep.sum()))
    mine = c.build_table()
    c.close()
    ref = T.Table.from_arrays(want_k, want_c, p, device=0)
    assert len(mine) == len(ref) == int(keep.sum()) and list(mine.build_stats) == [len(want_k), len(ref), 0]
    mine.upload(0)
    ref.upload(0)
    q = np.concatenate([want_k, zone ^ np.uint64(1), rng.integers(0, 1 << (2 * k), 50_000, dtype=np.uint64)])
    a, b = mine.lookup(q), ref.lookup(q)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[0][:len(want_k)], np.where(keep, want_c, 0))
    for direction in (0, 1):
        a, b = mine.next_counts(zone, direction), ref.next_counts(zone, direction)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    mine.close()
    ref.close()


# ---------------------------------------------------------------- 3g. count edges
@pytest.mark.parametrize("k", [18, 21, 31])
@pytest.mark.parametrize("built", ["host", "device"])
@pytest.mark.parametrize("name", PU.COUNT_EDGES)
def test_count_edges(name, built, k):
    """A count of exactly 0xFFFFFFFF (the oracle keeps such a k-mer; the device builder's count words are preset to that
    value, so its finalize pass runs before the counts are written), a dump without a kept line, one (K-1)-prefix."""
    tt, ot, keys, qs, oc, oj = PU.check_count_edge(name, k, 0 if built == "device" else None)
    tt.upload(0)
    c, j = tt.lookup(qs)
    assert (c == oc).all() and (j == oj).all(), (name, built, k)
    for direction in (0, 1):
        g4c, g4j = tt.next_counts(keys, direction)
        for i, km in enumerate(keys.tolist()):
            e4c, e4j = ot.next_counts(PU.kmer_text(km, k), direction)
            assert e4c.tolist() == g4c[i].tolist() and e4j.tolist() == g4j[i].tolist(), (name, built, direction, i)
    if name == "one-prefix":
        img = PU.DeviceImage(tt)
        assert int((img.right["key"] != PU.EMPTY).sum()) == 1 and int((img.left["key"] != PU.EMPTY).sum()) == 4
        img.free()
    ctx = T.Context(tt, tt.params, 0)
    reads = [PU.kmer_text(x, k) for x in keys.tolist()] + ["ACGT" * 20]
    bases, offs = PU.pack_reads(reads)
    b = ctx.batch(bases, offs)
    b.coverage()
    c, j, ko, nin = b.fetch_coverage()
    b.close()
    want = np.concatenate([ot.coverage(s)[0] for s in reads])
    assert (c == want).all(), (name, built, k)
    ctx.close()
    tt.close()
