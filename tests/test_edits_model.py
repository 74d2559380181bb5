"""Python models of the device code of the edit scripts (talc_amd/csrc/talc_kernels_edits.h), held against the numpy
contract (tests/edits_ref.py) without a GPU.  They guard the two pieces of logic the kernels add to what existed:

* wave_edit_trace: that the four delta words kept per column are enough for the canonical traceback — D[p][t] -
  D[p-1][t-1] is the vertical delta of (p, t) plus the horizontal delta of (p - 1, t) — with either sequence as the pattern
  and with the pattern taken in blocks that hand each other their last row's deltas;
* walk_edit_parts and the adds of k_edit_pack and of k_edit_align's second run, lane by lane: 64 segments per pass, the
  nearest non-empty part below, the last op carried between passes, the inclusive scan that places every part, and
  len << 4 | code added into zeroed ops.

The models restate the kernels' arithmetic; they do not run them (tests/test_gpu_edits.py does)."""
import itertools
import random

import numpy as np

import corr_map_ref as M
import edits_ref as E
import pieces_ref as P
from edits_util import batch_of, u8


def kept_words_script(a, b, BW):
    """(merged runs, distance) as wave_edit_trace makes them: the forward pass over blocks of BW pattern positions (one
    big integer per block stands for the 64 lanes' words and the carry that crosses them), every column's Pv, Mv, Ph, Mh
    kept, the blocks' hand-over of their last row's horizontal deltas, then the traceback from single bits of those words."""
    n, m = len(a), len(b)
    aIsPat = n >= m
    pat, txt = (a, b) if aIsPat else (b, a)
    np_, nt = len(pat), len(txt)
    nblk = (np_ + BW - 1) // BW
    mask = (1 << BW) - 1
    # store[t][blk] = (Pv, Mv, Ph, Mh)
    store = [[None] * nblk for _ in range(nt)]
    workP = [0] * nt; workM = [0] * nt
    score = np_
    for blk in range(nblk):
        last = blk + 1 == nblk
        pm = {}
        for i in range(BW):
            p = blk * BW + i
            if p < np_:
                pm[pat[p]] = pm.get(pat[p], 0) | (1 << i)
        top = (np_ - 1 - BW * blk) if last else BW - 1
        Pv, Mv = mask, 0
        for t in range(nt):
            Eq = pm.get(txt[t], 0)
            hp = workP[t] if blk > 0 else 1
            hm = workM[t] if blk > 0 else 0
            Xv = Eq | Mv
            Eqx = Eq | (1 if hm else 0)
            Xa = Eqx & Pv
            S = (Xa + Pv) & mask
            Xh = (S ^ Pv) | Eqx
            Ph = (Mv | ~(Xh | Pv)) & mask
            Mh = Pv & Xh
            up = (Ph >> top) & 1; dn = (Mh >> top) & 1
            if last: score += up - dn
            else: workP[t] = up; workM[t] = dn
            Phs = ((Ph << 1) | hp) & mask
            Mhs = ((Mh << 1) | hm) & mask
            Pv = (Mhs | ~(Xv | Phs)) & mask
            Mv = Phs & Xv
            store[t][blk] = (Pv, Mv, Ph, Mh)
    def bit(t, p, k):  # pattern position p (1-based), k index
        q = p - 1
        return (store[t - 1][q // BW][k] >> (q % BW)) & 1
    p, t = np_, nt
    ops = []
    while p > 0 and t > 0:
        dv = bit(t, p, 0) - bit(t, p, 1)
        dha = 1 if p < 2 else bit(t, p - 1, 2) - bit(t, p - 1, 3)
        neq = int(pat[p - 1] != txt[t - 1])
        if dv + dha == neq:
            ops.append(E.OP_X if neq else E.OP_EQ); p -= 1; t -= 1; continue
        dele = bit(t, p, 0) if aIsPat else bit(t, p, 2)
        ops.append(E.OP_D if dele else E.OP_I)
        if bool(dele) == aIsPat: p -= 1
        else: t -= 1
    ra, rb = (p, t) if aIsPat else (t, p)
    ops += [E.OP_D] * ra + [E.OP_I] * rb
    return E.merge([(c, 1) for c in reversed(ops)]), score


def check_kept_words(a, b, BW):
    want = E.align(u8(a), u8(b))
    got = kept_words_script(a, b, BW)
    assert got == want, (a, b, BW, got, want)


def test_kept_delta_words_give_the_canonical_script_on_all_short_pairs():
    words = ["".join(w) for n in range(1, 6) for w in itertools.product("AC", repeat=n)]
    for a in words:
        for b in words:
            for BW in (2, 3, 64):                 # blocks of 2 and 3 positions: every pair crosses block borders
                check_kept_words(a, b, BW)


def test_kept_delta_words_give_the_canonical_script_on_random_pairs():
    rng = random.Random(3)
    for _ in range(1500):
        la, lb = rng.randint(1, 40), rng.randint(1, 40)
        alpha = rng.choice(["A", "AC", "ACGTN"])
        a = "".join(rng.choice(alpha) for _ in range(la))
        if rng.random() < 0.5:                    # b = a with a few edits, else unrelated
            b = list(a)
            for _ in range(rng.randint(0, 6)):
                k, r = rng.randrange(len(b) + 1), rng.random()
                if r < .3 and b:
                    b.pop(min(k, len(b) - 1))
                elif r < .6:
                    b.insert(k, rng.choice(alpha))
                elif b:
                    b[min(k, len(b) - 1)] = rng.choice(alpha)
            b = "".join(b) or "A"
        else:
            b = "".join(rng.choice(alpha) for _ in range(lb))
        for BW in (4, 7, 16, 4096):
            check_kept_words(a, b, BW)


EMPTY, INS, DEL, UNAL, DP = range(5)
def kind_of(n, m, cap):
    if n == 0: return EMPTY if m == 0 else INS
    if m == 0: return DEL
    return UNAL if n * m > cap else DP

def walk(segs, parts, cap, emit):
    nseg = len(segs)
    row = dict(eq=0, x=0, i=0, d=0, nops=0, unal=0)
    openLast = 0
    for base in range(0, nseg, 64):
        L = []
        for lane in range(64):
            j = base + lane
            s = segs[j] if j < nseg else (M.RAW, 0, 0, 0, 0)
            knd, rs, rl, os_, ol = [int(x) for x in s]
            nRuns = first = last = 0; cnt = [0, 0, 0, 0]; unal = 0; kind = EMPTY
            if knd != M.CORRECTED:
                if ol: nRuns, first, last, cnt = 1, 7, 7, [ol, 0, 0, 0]
            else:
                kind = kind_of(rl, ol, cap)
                if kind == INS: nRuns, first, last, cnt = 1, 1, 1, [0, 0, ol, 0]
                elif kind == DEL: nRuns, first, last, cnt = 1, 2, 2, [0, 0, 0, rl]
                elif kind == UNAL: nRuns, first, last, cnt, unal = 2, 2, 1, [0, 0, ol, rl], 1
                elif kind == DP:
                    p = parts[j]; nRuns, first, last, cnt = p['nRuns'], p['first'], p['last'], p['cnt']
            L.append(dict(j=j, s=(knd, rs, rl, os_, ol), nRuns=nRuns, first=first, last=last, cnt=cnt, unal=unal, kind=kind))
        ne = sum((1 << l) for l in range(64) if L[l]['nRuns'] > 0)
        incl = []; acc = 0
        vs = []
        for lane in range(64):
            lower = ne & ((1 << lane) - 1)
            prevLane = lower.bit_length() - 1 if lower else 0
            prevLast = L[prevLane]['last'] if lower else openLast
            merges = L[lane]['nRuns'] > 0 and prevLast == L[lane]['first']
            v = L[lane]['nRuns'] - (1 if merges else 0)
            acc += v; incl.append(acc); vs.append((v, merges))
        for lane in range(64):
            v, merges = vs[lane]
            opBase = row['nops'] + incl[lane] - v - (1 if merges else 0)
            if L[lane]['j'] < nseg: emit(L[lane], opBase, merges)
        row['nops'] += incl[63]
        if ne: openLast = L[ne.bit_length() - 1]['last']
        for l in L:
            row['eq'] += l['cnt'][0]; row['x'] += l['cnt'][1]; row['i'] += l['cnt'][2]; row['d'] += l['cnt'][3]; row['unal'] += l['unal']
    return row

def device(reads, segs, so, rec, ro, cap):
    ops_all, oo, rows = [], [0], []
    for r in range(len(reads)):
        sg = segs[int(so[r]):int(so[r + 1])]
        raw = E.dna5_bytes(reads[r]); out = rec[int(ro[r]):int(ro[r + 1])]
        parts = {}
        for j, s in enumerate(sg):
            if s['kind'] == M.CORRECTED and kind_of(int(s['raw_len']), int(s['out_len']), cap) == DP:
                runs, dist = E.align(raw[int(s['raw_start']):int(s['raw_start']) + int(s['raw_len'])], out[int(s['out_start']):int(s['out_start']) + int(s['out_len'])])
                cnt = [sum(l for c, l in runs if c == k) for k in (7, 8, 1, 2)]
                parts[j] = dict(nRuns=len(runs), first=runs[0][0], last=runs[-1][0], cnt=cnt, runs=runs)
        place = {}
        row = walk(sg, parts, cap, lambda l, opBase, merges: place.__setitem__(l['j'], (opBase, merges)) if l['kind'] == DP else None)
        ops = [0] * row['nops']
        def add(at, code, ln, opens):
            if at < len(ops): ops[at] += (ln << 4) | (code if opens else 0)
        def pack(l, opBase, merges):
            knd, rs, rl, os_, ol = l['s']
            if knd != M.CORRECTED:
                if ol: add(opBase, 7, ol, not merges)
            elif l['kind'] == INS: add(opBase, 1, ol, not merges)
            elif l['kind'] == DEL: add(opBase, 2, rl, not merges)
            elif l['kind'] == UNAL: add(opBase, 2, rl, not merges); add(opBase + 1, 1, ol, True)
        walk(sg, parts, cap, pack)
        for j, (opBase, merges) in place.items():
            for k, (c, ln) in enumerate(parts[j]['runs']):
                add(opBase + k, c, ln, not (k == 0 and merges))
        ops_all += ops; oo.append(len(ops_all)); rows.append((row['eq'], row['x'], row['i'], row['d'], row['nops'], row['unal']))
    rr = np.zeros(len(rows), dtype=E.EDIT_ROW_DTYPE)
    for i, w in enumerate(rows): rr[i] = w
    return np.asarray(ops_all, dtype=np.uint32), np.asarray(oo, dtype=np.uint64), rr


def compare(args, cap):
    got, want = device(*args, cap), E.edits(*args, max_cells=cap)
    for g, w, n in zip(got, want, ("ops", "op_offsets", "rows")):
        assert np.array_equal(g, w), (n, cap)


def test_the_merge_walk_on_the_oracle_derived_map():
    s = M.map_set("default")
    segs, so, rec, ro, _ = P.from_expected(s.exp)
    for cap in (1 << 26, 4096, 300):
        compare((s.reads, segs, so, rec, ro), cap)


def test_the_merge_walk_where_a_64_segment_pass_ends():
    """Reads of 1 to 200 segments of random kinds, many of them empty, one-sided or (at the small caps) unaligned."""
    rng = np.random.default_rng(4)
    reads = []
    for nseg in (1, 2, 63, 64, 65, 127, 128, 129, 200):
        for rep in range(6):
            raw, spec = "", []
            for i in range(nseg):
                k = int(rng.choice([M.SOLID, M.CORRECTED, M.CORRECTED, M.RAW]))
                if k != M.CORRECTED:
                    ln = int(rng.choice([0, 0, 1, 5]))
                    t = "".join(rng.choice(list("AC"), size=ln))
                    raw += t
                    spec.append((k, ln, t))
                else:
                    rl, ol = int(rng.choice([0, 0, 1, 3, 9])), int(rng.choice([0, 0, 1, 3, 9]))
                    raw += "".join(rng.choice(list("AC"), size=rl))
                    spec.append((k, rl, "".join(rng.choice(list("AC"), size=ol))))
            reads.append((raw, spec))
    args = batch_of(reads)
    for cap in (1 << 26, 20, 2):
        compare(args, cap)
