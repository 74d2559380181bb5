"""How the edit scripts size and place their alignments (talc_amd/csrc/talc_edit_plan.h), without a GPU: the LDS / global
switch, the words a pair takes, and the rounds that keep the words of the DPs running side by side under a budget."""
import numpy as np

from edits_util import plan, pure, words

EMPTY, INS, DEL, UNALIGNED, DP = range(5)
IN_LDS = (1 << 64) - 1


def test_the_lds_switch_and_the_words_of_a_pair():
    L = pure()
    lds = lambda n, m: bool(L.pure_edit_in_lds(n, m))
    for n, m, want in ((64, 64, True), (128, 128, True), (129, 128, False), (128, 129, False), (129, 85, True), (129, 86, False), (192, 85, True), (192, 86, False), (85, 192, True),
                       (86, 192, False), (1024, 16, True), (1024, 17, False), (1025, 16, False), (16, 1025, False), (1, 1, True), (1025, 1, False)):
        assert lds(n, m) == want, (n, m)
    rng = np.random.default_rng(3)
    for n, m in [(int(a), int(b)) for a, b in rng.integers(1, 9000, size=(400, 2))] + [(4096, 4096), (4097, 1), (1, 4097), (1 << 20, 512)]:
        nw, nt = (max(n, m) + 63) // 64, min(n, m)
        w = words(n, m)
        assert w % 16 == 0 and 0 <= w - (4 * nw * nt + 2 * ((nt + 63) // 64)) < 16          # the delta words, then the block carries; whole cache lines
        if lds(n, m):
            assert 4 * nw * nt <= 1024 and n + m <= 1280                                    # what k_edit_align's LDS arrays hold
        elif max(n, m) >= 64:
            assert 8 * w <= n * m + nt // 4 + 136, (n, m)                                   # one pair of <= 1 << 29 cells fits the 1 GiB budget


def test_rounds_keep_the_words_under_the_budget():
    a, b, c = (200, 150), (300, 100), (129, 129)          # three global pairs
    wa, wb, wc = words(*a), words(*b), words(*c)
    assert wa > wb > wc and wb + wc > wa
    small = (60, 59)                                      # in LDS: takes no words, never ends a round
    pairs = [small, a, small, b, (0, 5), (7, 0), (0, 0), (3000, 3000), c, small]
    for budget, want_rounds in ((wa + wb + wc, 1), (wa + wb + wc - 1, 2), (wa + wb, 2), (wa + wb - 1, 2), (wb + wc, 2), (wb + wc - 1, 3), (wa, 3)):
        rounds, kind, word, rnd, most = plan(pairs, 1 << 20, budget)
        assert kind == [DP, DP, DP, DP, INS, DEL, EMPTY, UNALIGNED, DP, DP]
        assert rounds == want_rounds, (budget, rounds)
        assert [word[i] for i in (0, 2, 9)] == [IN_LDS] * 3 and all(rnd[i] == -1 for i in (4, 5, 6, 7))
        assert rnd[0] <= rnd[1] <= rnd[2] <= rnd[3] <= rnd[8] <= rnd[9]                     # in order
        used = {}
        for i, w in ((1, wa), (3, wb), (8, wc)):
            start = used.get(rnd[i], 0)
            assert word[i] == start and start % 16 == 0                                     # side by side from word 0 of its round
            used[rnd[i]] = start + w
        assert most == max(used.values()) <= budget
    assert plan(pairs, 1 << 20, max(wa, wb, wc) - 1)[0] == -1                               # one pair alone beyond the budget
    assert plan([small, (0, 0)], 100, 0)[0] == 1 and plan([], 100, 10)[0] == 1              # nothing global: one (possibly empty) round
