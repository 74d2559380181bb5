"""tests/fold_ref.py, the numpy statement of the both-strands contract (docs/both_strands.md), against a naive
collections.Counter restatement over text, and the properties the contract promises."""
import numpy as np
import pytest

import fold_ref as F
import kmer_ref as R

KS = [18, 21, 30, 31]


def records(k):
    return R.hand_records() + F.palindrome_records(18) + F.palindrome_records(30)


def folded(recs, k):
    bases, offs = R.records_to_arrays(recs)
    return F.fold_records(bases, offs, k)


@pytest.mark.parametrize("k", KS)
def test_rc_and_canon_equal_the_text_definition(k):
    rng = np.random.default_rng(k)
    for _ in range(200):
        s = "".join(rng.choice(list("ACGT"), size=k))
        m = F.revcomp_text(s)
        x = np.uint64(F.pack_text(s))
        assert int(F.rc(x, k)) == F.pack_text(m)
        assert int(F.canon(x, k)) == F.pack_text(min(s, m))       # unsigned order is the lexicographic one
        assert int(F.rc(F.rc(x, k), k)) == int(x)
    assert int(F.rc(np.uint64(0), k)) == (1 << (2 * k)) - 1       # A...A <-> T...T


@pytest.mark.parametrize("k", KS)
def test_fold_equals_the_naive_counter(k):
    recs = records(k)
    y, c = folded(recs, k)
    want = F.naive_fold(recs, k)
    assert len(y) == len(want) > 0
    assert {F.pack_text(s): n for s, n in want.items()} == dict(zip(y.tolist(), c.tolist()))
    assert (y == F.canon(y, k)).all() and (np.diff(y.astype(object)) > 0).all()
    # the directional counts of the same records fold to the same sums
    d = R.naive_count(recs, k)
    y2, c2 = F.fold(np.array(list(d.keys()), dtype=np.uint64), np.array(list(d.values()), dtype=np.uint64), k)
    assert np.array_equal(y, y2) and np.array_equal(c, c2)


@pytest.mark.parametrize("k", KS)
def test_fold_is_invariant_under_reverse_complementing_any_subset(k):
    recs = records(k)
    y, c = folded(recs, k)
    rng = np.random.default_rng(3)
    for _ in range(4):
        flip = rng.random(len(recs)) < 0.5
        mixed = [F.revcomp_text(r) if f else r for r, f in zip(recs, flip)]
        y2, c2 = folded(mixed, k)
        assert np.array_equal(y, y2) and np.array_equal(c, c2)
    bases, offs = R.records_to_arrays(recs)
    fb, flip = F.flip_records(bases, offs, np.random.default_rng(1))
    assert flip.any() and not flip.all()
    y3, c3 = F.fold_records(fb, offs, k)
    assert np.array_equal(y, y3) and np.array_equal(c, c3)


@pytest.mark.parametrize("k", [18, 30])
def test_a_palindrome_counts_once_and_is_stored_once(k):
    recs = F.palindrome_records(k)
    y, c = folded(recs, k)
    pal = F.is_palindrome(y, k)
    assert pal.sum() >= len(recs) - 1                    # one per distinct record, on the seam
    naive = R.naive_count(recs, k)                       # directional: a palindromic window is ONE window
    for x, n in zip(y[pal].tolist(), c[pal].tolist()):
        assert n == naive[x]                             # not doubled
    first = F.pack_text(recs[0][len(recs[0]) // 2 - k // 2:len(recs[0]) // 2 + k // 2])
    assert F.is_palindrome(np.uint64(first), k) and dict(zip(y.tolist(), c.tolist()))[first] == 2    # the record is there twice
    km, ct = F.expand(y, c, k)
    assert len(km) == 2 * len(y) - int(pal.sum())


@pytest.mark.parametrize("k", [21, 31])
def test_odd_k_has_no_palindrome(k):
    y, _ = folded(records(k), k)
    assert not F.is_palindrome(y, k).any()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("min_count", [1, 2, 3])
def test_expand_lists_each_stored_kmer_once_with_the_folded_count(k, min_count):
    y, c = folded(records(k), k)
    km, ct = F.expand(y, c, k, min_count)
    assert len(np.unique(km)) == len(km) and (np.diff(km.astype(object)) > 0).all()
    assert (ct >= min_count).all()
    look = dict(zip(y.tolist(), c.tolist()))
    for x, n in zip(km.tolist(), ct.tolist()):
        assert look[int(F.canon(np.uint64(x), k))] == n
    stored = set(km.tolist())
    for x, n in look.items():                            # both strands of every kept k-mer, nothing of the others
        r = int(F.rc(np.uint64(x), k))
        assert ((x in stored) and (r in stored)) == (n >= min_count)
        assert (x in stored) == (r in stored)


def test_entries_add_up_and_a_zero_count_claims_nothing():
    k = 18
    x = np.uint64(F.pack_text("ACGTTGCAAGGCTTAACG"))
    r = F.rc(x, k)
    other = np.uint64(F.pack_text("AAAAAAAAAAAAAAAAAC"))
    y, c = F.fold(np.array([x, r, x, other, x], dtype=np.uint64), np.array([3, 4, 5, 0, 0]), k)
    assert y.tolist() == [int(min(x, r))] and c.tolist() == [12]
    y, c = F.fold(np.array([x, r], dtype=np.uint64), np.array([0xFFFFFFFF, 1]), k)
    assert c.tolist() == [1 << 32]                       # exact: the caller sees that 32 bits do not hold it
    with pytest.raises(AssertionError):
        F.expand(y, c, k)
