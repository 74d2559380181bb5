"""-m gpu: the states a table object passes through — host-built or device-built (staged), coloured where it lives,
uploaded (a staged image is adopted where it is, a host image is copied), exported, imported, copied back to the host on
demand, uploaded to a second GPU — and what every call answers in each of them.  Point lookups are compared with the
oracle table, which gets the same colouring at the same moments.

Two small tables (60 000 k-mers, K = 21): one without junction colours, one with them.  Both dumps hold the four
homopolymers, and the coloured one has a junction line for each, so the de-colouring changes answers too."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import parity_util as PU
from talc_amd import lib as T
from talc_amd.synth import Synth

pytestmark = pytest.mark.gpu

K = 21
HOM = np.array([int(d * K, 4) for d in "0123"], dtype=np.uint64)


class Spec:
    """One dump, its junction lines, the queries, and the oracle's answers at every stage of the build (`raw`: inserted,
    `coloured`: junction lines applied, `final`: homopolymers de-coloured).  Computed once, never changed."""

    def __init__(self, junctions, seed):
        self.synth = Synth(target_kmers=60_000, k=K, seed=seed)
        self.p, self.q = PU.both_params(k=K, use_junctions=int(junctions))
        keys, counts = self.synth.dump_arrays(release=False)
        self.keys = np.concatenate([keys, HOM])
        self.counts = np.concatenate([counts, np.full(4, 50, np.uint32)])
        if junctions:
            jk, jc = self.synth.junction_arrays()
            self.jk, self.jc = np.concatenate([jk, HOM]), np.concatenate([jc, np.full(4, 77, np.int64)]).astype(np.int64)
        else:
            self.jk, self.jc = np.zeros(0, np.uint64), np.zeros(0, np.int64)
        rng = np.random.default_rng(seed)
        self.qs = np.concatenate([self.keys[:3000], rng.integers(0, 1 << (2 * K), 3000, dtype=np.uint64), self.jk[:2000],
                                  PU.revcomp_packed(self.jk[:500], K) if junctions else self.jk, HOM])
        otab = O.OracleTable(self.q, O.OracleTable.FLAT)
        otab.insert_packed(self.keys, self.counts)
        self.want = {"raw": otab.lookup_packed(self.qs)}
        otab.colour_packed(self.jk, self.jc)
        self.want["coloured"] = otab.lookup_packed(self.qs)
        otab.decolour()
        self.want["final"] = otab.lookup_packed(self.qs)
        self.size = len(otab)
        otab.close()
        minc = self.p.min_count
        assert int((self.want["raw"][0] >= minc).sum()) > 1000 and int((self.want["raw"][0] == 0).sum()) >= 3000
        assert (self.want["raw"][1] == 0).all() and (self.want["raw"][0][-4:] == 50).all()
        if junctions:   # the colouring and the de-colouring each change answers
            assert int((self.want["coloured"][1] > 0).sum()) > 500 and (self.want["coloured"][1][-4:] == 77).all()
            assert (self.want["final"][1][-4:] == 0).all() and int((self.want["final"][1] > 0).sum()) > 500
        else:
            assert (self.want["final"][1] == 0).all()

    def table(self, device=None, finish=True):
        """A product table from the dump: host-built (device None) or built on GPU `device` (staged there)."""
        t = T.Table.from_arrays(self.keys, self.counts, self.p, device=device)
        assert len(t) == self.size
        if finish:
            t.colour(self.jk, self.jc)
            t.decolour_repeats()
        return t

    def same(self, answer, stage, what=""):
        c, j = answer
        wc, wj = self.want[stage]
        assert (c == wc).all() and (j == wj).all(), (what, stage, int((c != wc).sum()), int((j != wj).sum()))


@pytest.fixture(scope="module")
def plain():
    return Spec(False, 71)


@pytest.fixture(scope="module")
def coloured():
    return Spec(True, 72)


@pytest.fixture(params=["plain", "coloured"])
def spec(request, plain, coloured):
    return plain if request.param == "plain" else coloured


@contextlib.contextmanager
def device_buffers(nbytes):
    """Two caller-owned buffers on GPU 0, as talc_table_export_device wants them."""
    hip = PU._hip()
    r, l = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(r), nbytes) == 0 and hip.hipMalloc(C.byref(l), nbytes) == 0
    try:
        yield r.value, l.value
    finally:
        hip.hipFree(r)
        hip.hipFree(l)


def assert_upload_wrote_degree_bits_only(before, after):
    """Two exported images of one table, before and after its upload: every word equal but the top three bits of the
    occupied RIGHT keys (the in-degrees, PU.check_indegree_bits_of_every_right_bucket)."""
    occ = before.right["key"] != PU.EMPTY
    assert (after.right["key"][~occ] == PU.EMPTY).all()
    assert (before.right["key"][occ] >> np.uint64(61) == 0).all()
    assert ((after.right["key"][occ] & PU.KEY_MASK) == before.right["key"][occ]).all()
    assert int((after.right["key"][occ] >> np.uint64(61) != 0).sum()) > 1000
    assert (after.right["cnt"] == before.right["cnt"]).all() and (after.right["jc"] == before.right["jc"]).all()
    assert after.left.tobytes() == before.left.tobytes()


def test_host_built_table_before_its_upload(spec):
    t = spec.table()
    with pytest.raises(T.TalcError, match="not uploaded to device 0"):
        t.lookup(spec.qs)
    with pytest.raises(T.TalcError, match="not uploaded to device 0"):
        T.Context(t, spec.p, 0)
    with device_buffers(t.image_bytes) as (r, l), pytest.raises(T.TalcError, match="no image on device 0"):
        t.export_device(0, r, l)
    for d in (0, 1):
        with pytest.raises(T.TalcError, match="not uploaded to device 0"):
            t.fetch_walk(d)
    spec.same(t.lookup_host(spec.qs), "final")
    assert t.device_bytes > 2 * t.image_bytes > 0
    t.close()


def test_host_built_table_after_its_upload(spec):
    t = spec.table()
    t.upload(0)
    spec.same(t.lookup(spec.qs), "final", "device")
    spec.same(t.lookup_host(spec.qs), "final", "host")
    nbytes = t.device_bytes
    assert nbytes > 2 * t.image_bytes
    t.upload(0)                                   # a second upload to the same GPU does nothing
    assert t.device_bytes == nbytes
    spec.same(t.lookup(spec.qs), "final", "device, uploaded twice")
    spec.same(t.lookup_host(spec.qs), "final", "host, uploaded twice")
    with pytest.raises(T.TalcError, match="already uploaded"):
        t.colour(HOM, np.full(4, 5, np.int64))
    with pytest.raises(T.TalcError, match="already uploaded"):
        t.decolour_repeats()
    spec.same(t.lookup(spec.qs), "final", "device, after the refused edits")
    t.close()


def test_staged_image_is_edited_in_place_and_the_host_image_follows(coloured):
    """A host lookup materialises the host image of a device-built table; colouring and de-colouring then run on the
    staged image, and the next host lookup must see them."""
    spec = coloured
    t = spec.table(device=0, finish=False)
    with pytest.raises(T.TalcError, match="not uploaded to device 0"):
        t.lookup(spec.qs)
    raw = PU.DeviceImage(t)                       # a staged image can be exported
    assert int((raw.right["key"] != PU.EMPTY).sum()) > 40_000 and (raw.right["jc"] == 0).all()
    spec.same(t.lookup_host(spec.qs), "raw")
    t.colour(spec.jk, spec.jc)
    spec.same(t.lookup_host(spec.qs), "coloured")
    t.decolour_repeats()
    spec.same(t.lookup_host(spec.qs), "final")
    done = PU.DeviceImage(t)
    assert (done.right["key"] == raw.right["key"]).all() and (done.right["cnt"] == raw.right["cnt"]).all()
    assert int((done.right["jc"] != 0).sum()) > 500 and int((done.left["jc"] != 0).sum()) > 500
    raw.free()
    done.free()
    t.close()


def test_upload_adopts_the_staged_image(coloured):
    spec = coloured
    t = spec.table(device=0)
    before = PU.DeviceImage(t)
    nbytes = t.device_bytes
    t.upload(0)
    after = PU.DeviceImage(t)
    assert_upload_wrote_degree_bits_only(before, after)
    assert t.device_bytes >= nbytes
    spec.same(t.lookup_host(spec.qs), "final", "host image copied back from the uploaded copy")
    spec.same(t.lookup(spec.qs), "final", "device")
    with pytest.raises(T.TalcError, match="already uploaded"):
        t.decolour_repeats()
    twin = spec.table()
    twin.upload(0)
    bases, offs = spec.synth.reads(0, 50)
    ctx, ctx2 = T.Context(t, spec.p, 0), T.Context(twin, spec.p, 0)
    a, b = ctx.correct(bases, offs), ctx2.correct(bases, offs)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len(a[2]) == 50 and not np.array_equal(a[0], bases)         # something was corrected
    ctx.close()
    ctx2.close()
    before.free()
    after.free()
    twin.close()
    t.close()


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("walk", ["0", "1"])
def test_walk_switch_decides_what_an_upload_holds(plain, monkeypatch, builder, walk):
    spec = plain
    monkeypatch.setenv("TALC_WALK", walk)
    t = spec.table(device=0 if builder == "device" else None)
    nbytes = t.device_bytes
    t.upload(0)
    if walk == "0":
        assert t.device_bytes == nbytes
        for d in (0, 1):
            with pytest.raises(T.TalcError, match="no walk tables"):
                t.fetch_walk(d)
    else:
        assert t.device_bytes == nbytes + 2 * t.capacity * 32
        for d in (0, 1):
            w = t.fetch_walk(d)
            assert len(w) == t.capacity and int((w["key"] != PU.EMPTY).sum()) > 40_000
    spec.same(t.lookup(spec.qs), "final")
    t.close()


def test_imported_image_is_staged_until_its_upload(coloured):
    spec = coloured
    src = spec.table(device=0)
    src.upload(0)
    image = PU.DeviceImage(src)                   # (its RIGHT keys carry degree bits)
    t = T.Table.import_device(spec.p, src.capacity, len(src), image.right_ptr.value, image.left_ptr.value, 0)
    assert len(t) == spec.size and t.capacity == src.capacity
    with pytest.raises(T.TalcError, match="not uploaded to device 0"):
        t.lookup(spec.qs)
    with pytest.raises(T.TalcError, match="not uploaded to device 0"):
        t.fetch_walk(1)
    staged = PU.DeviceImage(t)
    assert staged.right.tobytes() == image.right.tobytes() and staged.left.tobytes() == image.left.tobytes()
    spec.same(t.lookup_host(spec.qs), "final", "host image of the staged import")
    t.decolour_repeats()                          # not refused: nothing has been uploaded yet (and nothing is left to de-colour)
    spec.same(t.lookup_host(spec.qs), "final", "after an edit of the staged import")
    nbytes = t.device_bytes
    t.upload(0)
    assert t.device_bytes >= nbytes
    spec.same(t.lookup(spec.qs), "final", "device")
    with device_buffers(t.image_bytes) as (r, l), pytest.raises(T.TalcError, match="no image on device 1"):
        t.export_device(1, r, l)
    again = PU.DeviceImage(t)
    assert again.right.tobytes() == image.right.tobytes() and again.left.tobytes() == image.left.tobytes()
    for x in (image, staged, again):
        x.free()
    t.close()
    src.close()


def test_second_gpu_gets_a_copy_through_the_host_image(coloured):
    if T.device_count() < 2:
        pytest.skip("needs two GPUs")
    spec = coloured
    t = spec.table(device=0)
    t.upload(0)
    nbytes = t.device_bytes
    t.upload(1)
    assert t.device_bytes == nbytes
    spec.same(t.lookup(spec.qs, device=0), "final", "device 0")
    spec.same(t.lookup(spec.qs, device=1), "final", "device 1")
    spec.same(t.lookup_host(spec.qs), "final", "host")
    t.close()
