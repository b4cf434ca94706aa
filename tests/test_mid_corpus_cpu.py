"""The level-2 corpus (tests/midgen.py) against the oracle, no GPU.

tests/test_gpu_mid_corpus.py compares k_hc_mid_serial with the oracle byte for byte on these blocks; this file shows
what that comparison is worth:

* the parse inside each case's probe region is the one its construction predicts (midgen works `expect` out from
  where it put the copies, never from a compressor's output), and a case and its twin parse differently;
* tools/pyref gives the oracle's bytes on every case: the expected bytes do not rest on one restatement;
* tests/midmodel.py -- the kernel's loop in Python: prefetch and patch, fused candidate compare, clamp, index
  comparisons -- gives the oracle's bytes on every case, and with any ONE operator changed (midmodel.DEFECTS) it gives
  other bytes on a case of the family that operator belongs to.  So a kernel with that defect fails the GPU test.

UNWITNESSED names the comparisons of the kernel that no input can put on an edge, with the reason; the test fails
when the set of defects the corpus does not notice is not exactly that table.
"""
import os
import sys
from collections import defaultdict

import numpy as np
import pytest

import midgen as mg
import midmodel as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "pyref"))

# Sub-decisions no block can show (n = block length; mflimit = n - 12, matchlimit = n - 5, ilimit = n - 8).
UNWITNESSED = {
    "e_gt_4": "mid_fill_end's `e > 5`: a taken match has a source in 1 .. ip - 1, so ip >= 2 and e >= 6; 5 is never reached, "
              "and with e == 6 the entry e - 5 = 1 has been probed already",
    "fill_guard_le": "mid_fill_end's `e - 2 < ilimit`: on the edge (e - 2 == ilimit) the match ends at n - 6 > mflimit, no "
                     "probe follows that could read what the fill stored",
    "no_inner_guards": "the four `e - k <= ilimit` inside that guard follow from it: e - 2 < ilimit gives e - 1 <= ilimit",
    "no_begin_guards": "`ip + 1 <= ilimit`, `ip + 2 <= ilimit`: a match starts at ip <= mflimit = ilimit - 4, moved or not",
}


@pytest.fixture(scope="module")
def streams(oracle):
    """{case name: the oracle's level-2 stream}, computed once"""
    return {name: oracle.compress_hc(b, 2) for _, name, b, _ in mg.cases()}


def _rel(seqs, probe):
    return [(q[0] - probe[0], q[1], q[2]) for q in seqs]


def test_block_sizes():
    cs = mg.cases()
    assert 300 <= len(cs) <= 700
    assert {c[0] for c in cs} == set(mg.FAMILIES)
    assert all(13 <= len(c[2]) <= 4096 for c in mg.small()) and len(mg.small()) + len(mg.large()) == len(cs)
    assert all(c[0] == "reach" and 65536 < len(c[2]) <= 67 * 1024 for c in mg.large()) and len(mg.large()) <= 24
    assert {len(c[2]) for c in cs if c[0] == "end_clamp"} >= {13, 14, 20}
    assert sum(len(c[2]) for c in cs) < 4 << 20


def test_hashes_are_the_models():
    """midgen searches its collisions with its own statement of the two hashes; the model has another"""
    b = mg.rnd(300, 5)
    for i in range(290):
        assert mg.hash_mid4(b, i) == mm.hash_mid4(b, i) and mg.hash_mid8(b, i) == mm.hash_mid8(b, i)
    assert mg.hash_mid8(b"abcdefgX", 0) == mg.hash_mid8(b"abcdefgY", 0)      # seven bytes decide it
    assert mg.probed(512) == 512 and mg.probed(513) == 514 and mg.probed(1025) == 1027


def test_parses_are_the_constructed_ones(streams):
    bad = []
    for fam, name, b, m in mg.cases():
        got = mg.in_probe(mg.walk(streams[name]), m["probe"])
        if got != m["expect"]:
            bad.append("%s: %s, expected %s" % (name, got, m["expect"]))
    assert not bad, "%d: %s" % (len(bad), "; ".join(bad[:8]))


def test_twins_differ(streams):
    """every case names a twin of its family; the two parse differently, as predicted, counted from the probe's start"""
    by = {c[1]: c for c in mg.cases()}
    sides = defaultdict(set)
    for fam, name, b, m in mg.cases():
        tfam, tname, tb, tm = by[m["twin"]]
        assert tfam == fam and tname != name
        assert _rel(m["expect"], m["probe"]) != _rel(tm["expect"], tm["probe"]), name
        assert _rel(mg.in_probe(mg.walk(streams[name]), m["probe"]), m["probe"]) != \
            _rel(mg.in_probe(mg.walk(streams[tname]), tm["probe"]), tm["probe"]), name
        if tm["accept"] != m["accept"]:
            sides[fam].add(m["accept"])
    for fam in mg.FAMILIES:                          # (the parses themselves are witnessed by the test above)
        assert sides[fam] == {True, False}, fam


def test_pinned_values(streams):
    """the figures of the corpus's description: a copy at n - 12 counts 7 bytes, one byte earlier 8, one later none;
    65535 is in reach of both tables and of the lookup, 65536 of none"""
    by = {c[1]: c for c in mg.cases()}

    def at(name):
        m = by[name][3]
        return _rel(mg.in_probe(mg.walk(streams[name]), m["probe"]), m["probe"])

    for via in ("h8", "h4"):
        for arrive in ("pf", "match"):
            for ext in ("eight", "end"):
                got = [at("end_clamp/%s/%s/%s/v0/m%+d" % (via, arrive, ext, d)) for d in (-1, 0, 1)]
                assert [[q[2] for q in g] for g in got] == [[8], [7], []], (via, arrive, ext, got)
    assert at("end_clamp/n13/run") == [] and at("end_clamp/n14/run") == [(2, 1, 7)]
    for d in (65534, 65535):
        assert at("reach/h8/d%d" % d) == [(0, d, 12)] and at("reach/m2/d%d" % d) == [(1, d, 10)]
        assert [at("reach/h4/l%d/d%d" % (n, d)) for n in (4, 5, 6)] == [[(0, d, n)] for n in (4, 5, 6)]
    for d in (65536, 65537):
        assert at("reach/h8/d%d" % d) == [] and [q[2] for q in at("reach/m2/d%d" % d)] == [4]
        assert [at("reach/h4/l%d/d%d" % (n, d)) for n in (4, 5, 6)] == [[], [], []]
    for k, first in ((511, 0), (512, 0), (513, 1), (1023, 1), (1024, 0), (1025, 2)):
        for anchor in ("start", "match"):
            assert [q[0] for q in at("step/%s/v0/k%d" % (anchor, k))] == [first], (anchor, k)


def test_prefetched_probes_and_moves_happen():
    """the events the families are about do occur where the names say: the probe at the copy is served by the prefetch
    in the `pf` cases and not in the `match` cases, the clamp acts at mflimit only, moved matches move"""
    for fam, name, b, m in mg.small():
        tr = []
        mm.compress(b, trace=tr)
        p = m["probe"][0]
        if fam == "end_clamp" and "arrive" in m and m["delta"] <= 0:
            assert (("pf", p) in tr) == (m["arrive"] == "pf") and (("probe", p) in tr) == (m["arrive"] == "match"), name
            assert (("clamp", p) in tr) == (m["delta"] == 0), name
        if fam == "end_clamp" and m.get("delta") == 1:
            assert ("pf", p) not in tr and ("probe", p) not in tr, name
        if fam == "pf_patch" and "step" in m:
            assert ("pf", p + m["step"]) in tr and not any(t[1] in range(p + 1, p + m["step"]) for t in tr), name
        if fam == "moved_index":
            assert any(t[0] == "move" for t in tr) == (m["ln"] == 8), name


def test_pyref_gives_the_same_bytes(streams):
    import zig_lz4_pyref as pr
    for fam, name, b, m in mg.cases():
        assert pr.compress_hc(b, 2) == streams[name], name


def test_model_gives_the_oracles_bytes(streams):
    for fam, name, b, m in mg.cases():
        assert mm.compress(b) == streams[name], name


def _noticed(defect, cs, streams):
    return [c[1] for c in cs if mm.compress(c[2], defect) != streams[c[1]]]


@pytest.mark.parametrize("defect", sorted(mm.DEFECTS))
def test_every_defect_is_noticed_by_its_family(streams, defect):
    """one operator of the kernel's loop changed: a case of the family that operator belongs to gets other bytes"""
    fam = mm.DEFECTS[defect]
    assert fam in mg.FAMILIES
    hit = _noticed(defect, [c for c in mg.cases() if c[0] == fam], streams)
    assert hit, "no %s case notices %s" % (fam, defect)


def test_issue_defects_are_all_modelled():
    named = {"no_patch8", "no_patch4", "pf_survives_match", "no_clamp", "ml2_ge", "moved_index_exact", "e_gt_4",
             "fill_guard_le", "dist_le_65536", "step_from_ip", "pos_ge_0"}
    assert named <= set(mm.DEFECTS) | set(mm.EQUIVALENT)
    assert named - set(mm.DEFECTS) == {"e_gt_4", "fill_guard_le"}      # see UNWITNESSED


def test_unwitnessed_is_exactly_what_no_block_shows(oracle, streams):
    """the defects nothing notices -- not this corpus, not a sweep of small blocks over small alphabets, where every
    guard near the block's end is exercised -- are the ones UNWITNESSED gives a reason for, and no others"""
    silent = {d for d in list(mm.DEFECTS) + list(mm.EQUIVALENT) if d not in mm.DEFECTS or not _noticed(
        d, [c for c in mg.small() if c[0] == mm.DEFECTS[d]] + ([c for c in mg.large()] if mm.DEFECTS[d] == "reach" else []), streams)}
    assert silent == set(UNWITNESSED) == set(mm.EQUIVALENT)
    rng = np.random.default_rng(11)
    blocks = [c[2] for c in mg.small()]
    for _ in range(400):
        n, a = int(rng.integers(13, 80)), int(rng.integers(2, 5))
        blocks.append(rng.integers(0, a, n, dtype=np.uint8).tobytes())
    for b in blocks:
        want = oracle.compress_hc(b, 2)
        for d in mm.EQUIVALENT:
            assert mm.compress(b, d) == want, (d, b.hex())
