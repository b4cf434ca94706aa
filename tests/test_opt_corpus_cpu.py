"""The price-parser corpus (tests/optgen.py) against the oracle and its counters, no GPU.  tests/test_gpu_opt_corpus.py
compares the kernels with the oracle's bytes on these blocks; this module proves that the blocks are what they are named
for, so that those bytes depend on the code they are meant to reach:

* every case, at every level it is meant for, shows the events of its `witness` in the counters the oracle keeps in
  compressOptimal (oracle.binding.OPT_STATS), and both twins of a pair lie on their own side of the edge;
* the second restatement (tools/pyref) gives the same bytes AND the same counters, for every case at every level (it is
  fast enough at level 12 on these blocks: none holds a run, so no case is left out);
* meta["decodes"] holds: the streams of the early-encode exits that do not decode, and the block on which that exit's
  forward walk leaves the anchor past the input (OutputTooSmall), are kept on purpose -- the GPU must reproduce them.

Records 1000 and above are READ BACK, not only written: the windows beyond the split count reverse-traversal hops
(hi_hop) and opt[cur - ll] reads (hi_back) there, and the traversal that begins beyond 1000 and continues below it
(x_hop) decides every sequence of the window.  A kernel that lost or misplaced such a record would emit other bytes.
Their prices are compared with prices from below the split in the tie chains (window/tie, ends/far_llen/tie).  Their
literal lengths cannot show: only literal records use one, above the split those are trailing literals (1 .. 3), and
literalsPrice is linear there, so every stored value prices alike.
"""
import os
import sys

import pytest

import cases
import edgegen as eg
import hccapgen as hg
import optgen as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))

FAMILIES = ("window", "optnum", "sufficient", "price", "ends", "wide")


@pytest.fixture(scope="module")
def runs(oracle):
    """{(case name, level): (the oracle's result, its counters)}, computed once"""
    out = {}
    for _, name, b, m in og.cases():
        for level in m["levels"]:
            out[(name, level)] = oracle.compress_hc_stats(b, level)
    return out


def _holds(want, got):
    return want[0] <= got <= want[1] if isinstance(want, tuple) else got == want


def test_corpus_shape():
    cs = og.cases()
    assert {c[0] for c in cs} == set(FAMILIES)
    assert 70 <= len(cs) <= 150
    for fam, name, b, m in cs:
        assert og.longest_run(b) <= 8, name
        assert (len(b) == og.WIDE) == (fam == "wide"), name
        assert len(b) <= 65536 or fam == "wide", name
        assert set(m["levels"]) <= set(og.LEVELS) and m["levels"], name
        if not m.get("big") and fam != "wide":
            assert len(b) < 24 * 1024, name
    assert [c[1] for c in cs if len(c[2]) == 65536] == ["ends/full"]
    by_name = {c[1]: c for c in cs}
    for fam, name, b, m in cs:
        if "twin" in m:
            t = by_name[m["twin"]]
            assert t[0] == fam and t[3]["levels"] == m["levels"] and t[1] != name, name
            assert abs(len(t[2]) - len(b)) <= 2 or "parse" in m, name
    assert [by_name["window/t%d" % t] for t in og.WINDOW_SIZES]
    assert {m["front"] for f, n, _, m in cs if n.startswith("optnum/chain100")} == set(og.OPTNUM_FRONTS)


def test_counters_witness_every_case(runs):
    bad = []
    for fam, name, b, m in og.cases():
        assert m["witness"] or "parse" in m, name
        for level in m["levels"]:
            s = runs[(name, level)][1]
            for k, want in m["witness"].items():
                if not _holds(want, s[k]):
                    bad.append("%s l%d: %s = %d, expected %s" % (name, level, k, s[k], want))
    assert not bad, "%d: %s" % (len(bad), "; ".join(bad[:8]))


def test_price_cases_parse_as_priced(runs):
    """the sequences inside the probe are the ones the price model of optgen.choice() gives; the twin's differ"""
    by_name = {c[1]: c for c in og.cases()}
    n = 0
    for fam, name, b, m in og.cases():
        if "parse" not in m:
            continue
        for level in m["levels"]:
            got = [(q[0] - m["probe"][0], q[2]) for q in eg.in_probe(eg.walk(runs[(name, level)][0]), m["probe"])]
            assert got == m["parse"], (name, level, got)
            assert m["parse"] != by_name[m["twin"]][3]["parse"], name
            n += 1
    assert n >= 50
    # the figures of the construction, literally: a copy of 19 bytes costs as much as a literal and 18 bytes, and the
    # later candidate wins -- except where the extra literal crosses a step of literalsPrice (14 -> 15, 269 -> 270)
    assert [og.choice(ll, 19, 3) for ll in (12, 13, 14, 15, 269, 270)] == [1, 1, 0, 1, 0, 1]
    assert [og.choice(0, m, 3) for m in (18, 19, 20, 273, 274, 275)] == [0, 1, 0, 0, 1, 0]
    assert by_name["price/llen14/m19"][3]["parse"] == [(0, 19)] and by_name["price/llen15/m19"][3]["parse"] == [(1, 18)]


def test_twins_lie_on_both_sides(runs):
    """the pair's counters differ in the event the pair is about"""
    by_name = {c[1]: c for c in og.cases()}
    pairs = 0
    for fam, name, b, m in og.cases():
        if "twin" not in m or "parse" in m:
            continue
        for level in m["levels"]:
            a, t = runs[(name, level)][1], runs[(m["twin"], level)][1]
            exits = lambda s: (s["first_sufficient"], s["exit_sufficient"], s["exit_optnum"])   # noqa: E731
            assert exits(a) != exits(t), (name, level)
            pairs += 1
    assert pairs >= 2 * (9 + 3 + 1)
    lp = {t: runs[("optnum/long_pair/sum%d" % t, 12)] for t in (4095, 4096)}
    assert lp[4095][1]["max_noexit_sum"] == 4095 and lp[4095][1]["max_window"] == 4095    # record 4098 is written
    assert lp[4096][1]["min_optnum_sum"] == 4096 and lp[4096][0] == -1
    for level in (10, 11):                            # `len > sufficient_len` at cur > 0, behind sequences
        s = og.SUFFICIENT[level]
        assert runs[("sufficient/l%d/chained/len%d" % (level, s + 1), level)][1]["exit_sufficient"] == 1
        assert runs[("sufficient/l%d/chained/len%d" % (level, s), level)][1]["max_window"] == s + 40


def test_the_split_is_crossed_in_every_way(runs):
    """per level, over the window family: every kind of access lands beyond record 1000, and every kind of step lies on
    both sides of it"""
    for level in og.LEVELS:
        tot = dict.fromkeys(("hi_match", "hi_trail", "hi_back", "hi_hop", "x_lit", "x_match", "x_trail", "x_back", "x_hop"), 0)
        for fam, name, _, m in og.cases():
            if fam == "window":
                for k in tot:
                    tot[k] += runs[(name, level)][1][k]
        assert all(v > 0 for v in tot.values()), (level, tot)
    # the sizes around the split, one by one: the trailing literals of a window that ends on 997 .. 999 straddle it
    for t, x_trail, hi_match in ((996, False, False), (997, True, False), (998, True, False), (999, False, False),
                                 (1000, False, True), (1001, False, True)):
        s = runs[("window/t%d" % t, 10)][1]
        assert (s["x_trail"] > 0) == x_trail and (s["hi_match"] > 0) == hi_match, (t, s)
    # An accepted literal update (:1265) needs a record two dearer than its predecessor; no construction here gives
    # one, and none of the scanned corpora either.  If that changes, the corpus should grow a case for it.
    assert all(s["lit_updates"] == 0 for _, s in runs.values())


def test_decodes_as_recorded(oracle, runs):
    kinds = set()
    for fam, name, b, m in og.cases():
        for level in m["levels"]:
            r = runs[(name, level)][0]
            if m["decodes"] is None:
                assert r == oracle.OUTPUT_TOO_SMALL, (name, level)
            else:
                assert not isinstance(r, int), (name, level)
                assert (oracle.decompress_safe(r, len(b)) == b) == m["decodes"], (name, level)
            kinds.add((fam, m["decodes"]))
    assert {("optnum", None), ("optnum", False), ("optnum", True), ("sufficient", False), ("wide", False)} <= kinds


def test_pyref_gives_the_same_bytes_and_events(runs):
    """every case, every level it is meant for (no case is too slow for the Python restatement)"""
    import zig_lz4_pyref as pr
    for fam, name, b, m in og.cases():
        for level in m["levels"]:
            t = {}
            try:
                got = pr.compress_hc(b, level, t)
            except OverflowError:
                got = -1                              # iend - anchor underflows: the oracle reports OutputTooSmall
            want, s = runs[(name, level)]
            assert got == want, (name, level)
            assert t == s, (name, level, {k: (t[k], s[k]) for k in s if t[k] != s[k]})


def test_the_older_corpora_do_not_reach_these_edges(oracle):
    """why this corpus exists: tests/cases.py, the small edge corpus and the capacity inputs take no OPT_NUM exit at any
    level, and at levels 10 and 11 no window of theirs comes near record 1000 (level 12 has long windows, but they are
    one first match over a run or a period)"""
    corpus = cases.reference_test_inputs() + cases.seeded_cases(65536) + [(c[1], c[2]) for c in eg.small()] + hg.swept_inputs()
    assert len(corpus) > 600
    for level in og.LEVELS:
        widest = 0
        for name, b in corpus:
            if len(b) > 65536:
                continue
            _, s = oracle.compress_hc_stats(b, level)
            assert s["exit_optnum"] == 0, (name, level)
            widest = max(widest, s["max_window"])
        if level < 12:
            assert widest < og.SPLIT, (level, widest)
        assert widest >= 300, (level, widest)          # (the scan does see windows: 328 at levels 10 and 11)
