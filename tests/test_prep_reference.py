"""tests/prep_ref.py alone (CPU): the composed contract reaches what it is there for on the dressed molecules, and chain()
equals the four contracts applied by hand, one after the other, with their plain-loop forms."""
import numpy as np

import chimera_ref as CR
import demux_ref as DR
import ends_ref as R
import prep_ref as P
import umi_ref as U

_set = {}


def composition():
    """200 random bodies of 500 to 1500 bases, dressed; every batch kind with every setting on.  Computed once, shared, left
    unchanged."""
    if not _set:
        rng = np.random.default_rng(8)
        bodies = [R.random_seq(rng, int(n)) for n in rng.integers(500, 1501, 200).tolist()]
        reads = P.reads_of(bodies, rng)
        kinds = {name: P.chain(reads, P.ENDS_KW, P.CHIMERA, P.DEMUX, P.UMI, clip=clip, split=split) for name, clip, split in P.KINDS}
        _set.update(bodies=bodies, reads=reads, kinds=kinds)
    return _set


def test_the_dressed_reads_reach_every_call_of_the_demux_table():
    s = composition()
    assert len(s["reads"]) == 185 and s["reads"][-4:-2] == ["", "ACGT"]
    for name, _, _ in P.KINDS:                                           # the rows of the reads as they came, whatever the kind
        assert s["kinds"][name]["demux"] is s["kinds"]["plain"]["demux"]
    d = s["kinds"]["plain"]["demux"]
    seen = np.bincount(d["status"], minlength=5)
    print("demux", seen.tolist(), len(set(d["barcode"][d["barcode"] > 0].tolist())))
    assert seen[DR.BOTH] >= 120
    assert seen[DR.CONFLICT] >= 10                                       # the joined reads
    assert (d["barcode"] == 0).sum() - seen[DR.CONFLICT] >= 15           # no call: the undressed and the edge reads
    assert len(set(d["barcode"][d["barcode"] > 0].tolist())) >= 60


def test_the_pieces_and_their_rows_reach_every_rule():
    s = composition()
    k = s["kinds"]["split + clip"]
    n, came = len(s["reads"]), k["came"]
    assert len(k["pieces"]) == len(came) > n + 10
    u, e = k["umi"], k["ends"]
    lens = np.array([len(x) for x in came])
    figures = dict(pieces=len(came), heads=int((u["end"] == 1).sum()), tails=int((u["end"] == 2).sum()), without=int((u["end"] == 0).sum()),
                   err=int((u["err"] > 0).sum()), gaps=sum(b"-" in x for x in u["umi"].tolist()), own=int((u["kept_start"] > e["kept_start"]).sum()),
                   empty=int((u["kept_len"] == 0).sum()), ends_cut=int((e["kept_len"] < lens).sum()))
    print(figures)
    assert figures["heads"] >= 60 and figures["tails"] >= 60 and figures["without"] >= 15
    assert figures["err"] >= 50 and figures["gaps"] >= 5
    assert figures["own"] >= 60                                          # the UMI's claim is the larger one
    assert figures["empty"] >= 1 and figures["ends_cut"] >= 150
    # the split kinds share hits and pieces; the UMI rows follow the plain formula unless the batch is clipped
    s_only = s["kinds"]["split"]
    assert (s_only["pieces"] == k["pieces"]).all() and (s_only["hits"] == k["hits"]).all() and s_only["came"] == came and s_only["texts"] == came
    assert (s_only["ends"] == e).all() and (s_only["umi"]["kept_len"] != u["kept_len"]).sum() >= 60
    assert (s_only["umi"][["end", "err", "start", "stop", "umi"]] == u[["end", "err", "start", "stop", "umi"]]).all()
    assert s["kinds"]["clip"]["hits"] is None and s["kinds"]["plain"]["hits"] is k["hits"] and s["kinds"]["plain"]["pieces"] is None
    assert sum(map(len, k["texts"])) < sum(map(len, came)) - 30 * len(came)      # (a dressed piece loses its UMI and poly-A: 44 bytes or more)


# ---------------------------------------------------------------- chain() against the steps by hand
BC = P.BC24[:6]
HAND_DEMUX = (BC, 20, 2)


def hand_reads():
    rng = np.random.default_rng(3)
    rc = lambda x: R.revcomp(x).decode()
    body = lambda n: "C" + R.random_seq(rng, n) + "C"
    umi = lambda: U.instance(rng, U.BARE)
    bodies = [body(150), body(180), body(160), body(170), body(140)]
    full = lambda b, bc, junk: bc + junk + P.SSP23 + umi() + "GGG" + b + "A" * 20 + rc(P.VNP) + junk + rc(bc)
    reads = [full(bodies[0], BC[0], "ACG"),                               # one full molecule
             rc(full(bodies[1], BC[1], "")),                              # one reverse-complemented
             full(bodies[2], BC[2], "TG") + "A" * 30 + rc(P.VNP) + CR.SSP + full(bodies[3], BC[3], "C"),   # a join of two
             bodies[4],                                                   # one undressed
             "ACGTACGTAC"]                                                # one shorter than every pattern
    return bodies, reads


def by_hand(reads, ends_on, chimera_on, demux_on, umi_on, clip, split):
    """The contracts' plain loops, one after the other, and host slicing."""
    out = dict.fromkeys(("demux", "hits", "pieces", "ends", "umi"))
    if demux_on:
        out["demux"] = DR.rows_plain(reads, *HAND_DEMUX)
    came = reads
    if chimera_on and (split or not clip):
        out["hits"] = CR.hits_plain(reads, P.ENDS_KW["adapters"], P.CHIMERA[1])
    if split:
        out["pieces"] = CR.pieces_plain([len(x) for x in reads], out["hits"], P.CHIMERA[2])[0]
        came = [reads[int(p["read"])][int(p["start"]):int(p["start"]) + int(p["len"])] for p in out["pieces"]]
    if ends_on:
        out["ends"] = R.rows_plain(came, **P.ENDS_KW)
    if umi_on:
        rows = U.rows_plain(came, *P.UMI)
        if clip and ends_on:                                             # docs/umi.md, "Clipping": the larger claim at either end
            for r, (w, e) in enumerate(zip(rows, out["ends"])):
                head, tail = int(e["head_adapter_len"]) + int(e["head_poly_len"]), int(e["tail_adapter_len"]) + int(e["tail_poly_len"])
                rows[r]["kept_start"], rows[r]["kept_len"] = U.kept(len(came[r]), int(w["end"]), int(w["stop"]), head, tail)
        out["umi"] = rows
    texts = came
    if clip:
        cut_by = out["umi"] if umi_on else out["ends"]
        texts = [x[int(w["kept_start"]):int(w["kept_start"]) + int(w["kept_len"])] for x, w in zip(came, cut_by)]
    out.update(came=came, texts=texts)
    return out


def test_chain_equals_the_steps_by_hand_under_every_subset_and_kind():
    bodies, reads = hand_reads()
    done = 0
    for ends_on, chimera_on, demux_on, umi_on in P.subsets():
        for name, clip, split in P.KINDS:
            if not P.legal(ends_on, chimera_on, umi_on, clip, split):
                continue
            got = P.chain(reads, P.ENDS_KW if ends_on else None, P.CHIMERA if chimera_on else None, HAND_DEMUX if demux_on else None,
                          P.UMI if umi_on else None, clip=clip, split=split)
            want = by_hand(reads, ends_on, chimera_on, demux_on, umi_on, clip, split)
            what = (ends_on, chimera_on, demux_on, umi_on, name)
            for key in ("demux", "hits", "pieces", "ends", "umi"):
                assert (got[key] is None) == (want[key] is None), (what, key)
                if want[key] is not None:
                    assert got[key].dtype == want[key].dtype and len(got[key]) == len(want[key]) and (got[key] == want[key]).all(), (what, key)
            assert got["came"] == want["came"] and got["texts"] == want["texts"], what
            done += 1
    assert done == 4 * 4 + 4 * 2 + 2 * 2 + 2 * 1                         # ends and chimera: 4 kinds; ends alone, UMI alone: 2; neither: 1
    # ... and what the five reads are there for, with everything on
    k = P.chain(reads, P.ENDS_KW, P.CHIMERA, HAND_DEMUX, P.UMI, clip=True, split=True)
    assert k["demux"]["status"].tolist() == [DR.BOTH, DR.BOTH, DR.CONFLICT, DR.NONE, DR.NONE] and k["demux"]["barcode"].tolist() == [1, 2, 0, 0, 0]
    assert k["pieces"]["read"].tolist() == [0, 1, 2, 2, 3, 4] and k["pieces"]["ordinal"].tolist() == [1, 1, 1, 2, 0, 0]
    assert k["umi"]["end"].tolist() == [1, 2, 1, 1, 0, 0] and (k["umi"]["err"] == 0).all()
    assert k["texts"] == [bodies[0], R.revcomp(bodies[1]).decode(), bodies[2], bodies[3], bodies[4], "ACGTACGTAC"]
    c = P.chain(reads, P.ENDS_KW, P.CHIMERA, HAND_DEMUX, P.UMI, clip=True)
    assert c["texts"][:2] == k["texts"][:2] and c["texts"][3:] == k["texts"][4:] and len(c["texts"]) == 5     # (the join is one read here)
    assert c["hits"] is None and (c["umi"][:2] != P.chain(reads, None, None, None, P.UMI, clip=True)["umi"][:2]).all()
