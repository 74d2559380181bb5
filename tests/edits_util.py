"""Inputs the edit-script tests share: reads with a given number of map segments, and the edge inputs of a batch."""
import ctypes as C
import os
import random

import numpy as np

import corr_map_ref as M
import parity_util as PU
from talc_amd import build as B


def u8(s):
    return np.frombuffer(s.encode(), dtype=np.uint8)


def batch_of(reads):
    """reads: [(raw text, [(kind, raw_len, record text of the segment)])] -> the arguments of edits()."""
    segs, so, rec, ro, raws = [], [0], "", [0], []
    for raw, spec in reads:
        rs, start = 0, len(rec)
        for kind, rl, text in spec:
            segs.append((kind, rs, rl, len(rec) - start, len(text)))
            rs += rl
            rec += text
        assert rs == len(raw)
        raws.append(raw)
        so.append(len(segs))
        ro.append(len(rec))
    return raws, M.as_array(segs), np.asarray(so, dtype=np.uint64), u8(rec), np.asarray(ro, dtype=np.uint64)


def reads_with_regions(s, targets):
    """Prefixes of the set's comb reads that the oracle corrects with exactly R regions, one per target (2 R + 1 segments):
    R grows by one every K + g bases, so a bisection over the prefix length finds each."""
    out = {}
    for seq in s.reads:
        for R in targets:
            if R in out:
                continue
            lo, hi = 18 * R, min(len(seq), 34 * R)
            while lo < hi:
                mid = (lo + hi) // 2
                e = M.expected(s.pair.otab, seq[:mid])
                if e["R"] >= R:
                    hi = mid
                else:
                    lo = mid + 1
            for ln in range(lo, min(len(seq), lo + 4)):
                e = M.expected(s.pair.otab, seq[:ln])
                if e["status"] == 0 and e["R"] == R:
                    out[R] = seq[:ln]
                    break
        if len(out) == len(targets):
            break
    assert sorted(out) == sorted(targets), sorted(out)
    return [out[R] for R in targets]


def edge_reads(s0):
    """The empty read, reads of K and K + 1 bases, lower case, N and other letters, repeats, random text, two reads joined."""
    r = PU.seqs_of(*s0.pair.reads(5000, 8))
    return ["", r[0][:21], r[0][:22], r[1].lower(), r[2][:400] + "N" + r[2][400:],
            r[3][:300] + "N" * 10 + r[3][300:900] + "RYKM" + r[3][900:], "ACGT" * 300, "A" * 500,
            "".join(random.Random(1).choice("ACGT") for _ in range(1500)), r[4], r[5][:60], r[6] + r[7]]


# ---- the host's planner (talc_amd/csrc/talc_edit_plan.h) through the host test library
def pure():
    L = C.CDLL(os.path.join(B.OUT, "libtalc_pure.so"))
    L.pure_edit_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pure_edit_scratch_words.restype = C.c_uint64
    L.pure_edit_scratch_words.argtypes = [C.c_uint32, C.c_uint32]
    L.pure_edit_in_lds.argtypes = [C.c_uint32, C.c_uint32]
    return L


def plan(pairs, max_cells, budget):
    n = np.asarray([p[0] for p in pairs], dtype=np.uint32)
    m = np.asarray([p[1] for p in pairs], dtype=np.uint32)
    kind, rnd = np.zeros(len(pairs), dtype=np.int32), np.zeros(len(pairs), dtype=np.int32)
    word, most = np.zeros(len(pairs), dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    rounds = pure().pure_edit_plan(n.ctypes.data, m.ctypes.data, len(pairs), max_cells, budget, kind.ctypes.data, word.ctypes.data, rnd.ctypes.data, most.ctypes.data)
    return rounds, kind.tolist(), [int(w) for w in word], rnd.tolist(), int(most[0])


def words(n, m):
    return int(pure().pure_edit_scratch_words(n, m))
