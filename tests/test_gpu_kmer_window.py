"""One base that is not a letter, at every fragile place of the k-mer window (talc_kmer_window.h: the N-mask words, the
passes, the K - 1 bases a pass stages beyond its positions, the read's two ends), through k_solidity, k_base_support and
k_strand_vote, in a plain, a -rev and an auto-strand context, against the contracts in numpy (tests/solidity_ref.py,
support_ref.py, strand_ref.py, from the host image of the table: never from a device result).  Integers and bytes,
tolerance 0.  What the reads are is asserted from the reference alone before any device call."""
import numpy as np
import pytest

import solidity_ref as S
import strand_ref as R
import support_ref as P
import test_gpu_solidity as G
import test_gpu_support as GS
from talc_amd import lib as T

pytestmark = pytest.mark.gpu

TILE = 256        # KWIN_TILE (talc_kmer_window.h): positions per pass of a wave
FORMS = [None, (2, 40)]
ACGT_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def places(k):
    """Where the base is replaced: both sides of every N-mask word and pass, the overlap of a pass, both ends."""
    L = 2 * TILE + 70 + k - 1
    return L, [0, k - 1, 63, 64, 64 + k - 2, 255, 256, 256 + k - 2, 256 + k - 1, 511, 512, L - k, L - 1]


def rc_raw(r):
    """The reverse complement of raw bytes: the letters complemented, every other byte where it was."""
    return r[::-1].translate(ACGT_COMP)


_made = {}


def made(k):
    """The table (every k-mer of one random sequence, counts above MIN_COUNT), the three contexts, the 13 clean reads and
    the weak positions each is to have: computed once per K, shared, left unchanged."""
    if k in _made:
        return _made[k]
    rng = np.random.default_rng(3000 + k)
    Gs = "".join("ACGT"[x] for x in rng.integers(0, 4, 1000).tolist())
    minc = T.default_params(k=k).min_count
    table = {}
    for i in range(len(Gs) - k + 1):
        table.setdefault(S.pack(Gs[i:i + k]), int(rng.choice([minc + 1, 50])))
    keys = np.fromiter(table.keys(), dtype=np.uint64, count=len(table))
    counts = np.fromiter(table.values(), dtype=np.uint32, count=len(table))
    c = G.Ctx(keys, counts, k=k)
    assert c.minc == minc and int(counts.min()) >= minc + 1
    rev = G.Ctx(share=c)
    rev.p = T.default_params(k=k, reverse=1)
    rev.ctx.close()
    rev.ctx, rev.rev = T.Context(c.ttab, rev.p, 0), True
    auto = G.Ctx(share=c)
    auto.ctx.auto_strand()
    L, js = places(k)
    n = L - k + 1
    assert n == 2 * TILE + 70 and len(js) == len(set(js)) == 13 and all(0 <= j < L for j in js)
    for b in (64, 256, 512):                               # both sides of every word and pass edge
        assert b - 1 in js and b in js
    clean = [Gs[7 * i + 3:7 * i + 3 + L] for i in range(len(js))]   # (every read starts at another alignment)
    assert all(len(r) == L for r in clean)
    weak = [(max(0, j - k + 1), min(j, n - 1)) for j in js]         # the positions that hold base j
    assert [b - a + 1 for a, b in weak] == [min(j, k - 1, L - 1 - j, n - 1) + 1 for j in js]
    ends, starts = {b for a, b in weak}, {a for a, b in weak}
    assert ends >= {0, 63, 64, 255, 256, 511, 512, n - 1} and starts >= {0, 63, 255, 256, n - 1}
    _made[k] = dict(c=c, rev=rev, auto=auto, clean=clean, js=js, weak=weak, L=L, n=n)
    return _made[k]


def same_strand(got, want, what):
    assert got.dtype == R.DTYPE and got.tolist() == want.tolist(), what


def probed(records, st, turned):
    """Ctx.as_probed with one flag per read: a corrected read's record was reverse-complemented on its way out where the
    read was turned."""
    return [S.revcomp(r) if (t and s == T.READ_CORRECTED) else r for r, s, t in zip(records, st.tolist(), turned)]


@pytest.mark.parametrize("letter", ["N", "n", "R"])
@pytest.mark.parametrize("k", [18, 21, 31])
def test_one_non_letter_at_every_edge(k, letter):
    m = made(k)
    c, n, L = m["c"], m["n"], m["L"]
    reads = [r[:j] + letter + r[j + 1:] for r, j in zip(m["clean"], m["js"])]
    # ---- from the reference alone: exactly the positions that hold base j are weak, all others solid
    for r, j, (a, b) in zip(reads, m["js"], m["weak"]):
        solid = S.counts(S.dna5(r), k, c.lookup) >= c.minc
        assert len(solid) == n and np.nonzero(~solid)[0].tolist() == list(range(a, b + 1)), (k, letter, j)
    seqs = [S.dna5(r) for r in reads]
    want_rows = c.ref(seqs)
    assert (want_rows["n_solid"] == [n - (b - a + 1) for a, b in m["weak"]]).all() and (want_rows["n_in"] == want_rows["n_solid"]).all()
    covers = [P.cover(s, k, c.minc, c.lookup) for s in seqs]
    rcs = [rc_raw(r) for r in reads]
    assert all(S.revcomp(S.dna5(x)) == s for x, s in zip(rcs, seqs))
    mixed = [x if i % 2 else r for i, (r, x) in enumerate(zip(reads, rcs))]
    flags = R.rows(mixed, k, c.minc, c.lookup)["reverse"].astype(bool)
    assert flags.tolist() == [bool(i % 2) for i in range(len(reads))]

    # ---- the device: (context, what it is given, which reads it turns); every context sees the sequences `seqs`
    for name, cx, given, turned in (("plain", c, reads, [False] * len(reads)), ("-rev", m["rev"], rcs, [True] * len(reads)),
                                    ("auto", m["auto"], mixed, flags.tolist())):
        what = "%s k=%d %r" % (name, k, letter)
        b = cx.ctx.batch(*G.pack_reads(given))
        try:
            same_strand(b.strand(), R.rows(given, k, c.minc, c.lookup), what + " vote")
            raw, none = b.solidity()
            assert none is None
            G.same_rows(raw, want_rows, what + " raw rows")
            for form in FORMS:
                got, offs = b.support("raw", form)
                GS.check(got, offs, covers, turned, k, form, what + " raw bytes")
            # after correct(): the references applied to whatever the records are
            b.correct()
            raw, cor = b.solidity()
            out, oo, st = b.fetch_corrected()
            records = G.seqs_of(out, oo)
            if name != "auto":
                assert probed(records, st, turned) == cx.as_probed(records, st)
            pr = probed(records, st, turned)
            G.same_rows(raw, want_rows, what + " raw rows after the correction")
            G.same_rows(cor, c.ref(pr), what + " corrected rows")
            flip = [t and s == T.READ_CORRECTED for t, s in zip(turned, st.tolist())]
            rec_cov = [P.cover(s, k, c.minc, c.lookup) for s in pr]
            for form in FORMS:
                got, offs = b.support("record", form)
                assert np.array_equal(offs, oo)
                GS.check(got, offs, rec_cov, flip, k, form, what + " record bytes")
        finally:
            b.close()
