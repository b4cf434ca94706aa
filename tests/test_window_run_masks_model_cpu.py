"""The run masks of the window path, on the CPU: every scalar form that k_compress_fast uses for a pending run next to
the form it replaced (tools/emulate_window.py has both).

  * E_run - (mm_run << 1) (mod 2^64) is run_cover(): the lanes strictly inside the matches of a run
  * the highest bit of E_run | bit(a0) at or below a lane is the end of the nearest match lane below it, else a0 (`pend`)
  * the scalar literal mask is the ballot one
  * a == 0 iff no sequence has been found (the counter nseq is gone)
  * fastm / stopm give the fast-run steps J / S gave, and X / Q (own-lane bits only) give the exact step what XP / Q held
  * the trip with one exit test consumes the sequences of the trip with two

on made-up runs (disjoint, ordered; a last end at or past lane 64, a match that starts where the previous one ends, a
run of one match) and made-up windows, and -- inside compress_run_masks(check=True), which evaluates both forms wherever
the kernel evaluates one -- on every window of the run-mask corpus (tests/runmaskgen.py) and of the block-start corpus.
The emulator still gives the oracle's bytes."""
import random

import pytest

import blockstartgen as bg
import runmaskgen as rg

ew = rg.ew


def _random_run(rng, last_over=None, touching=False, single=False):
    """-> (mm_run, v_end, a0): match lanes j with end lanes e >= j + 4, ranges disjoint and in order; the search behind a
    match starts at e + 1 unless `touching` (the next match lane may be e itself)"""
    a0 = rng.randrange(0, 40)
    v_end = [i + 4 + rng.randrange(0, 44) for i in range(64)]        # what the vector code holds for the other lanes
    mm, lo = 0, a0 + (0 if a0 == 0 or touching else 1)
    while lo < 64:
        j = lo + (0 if touching and mm else rng.randrange(0, 12))
        if j >= 64: break
        e = j + 4 + rng.randrange(0, 30)
        mm |= 1 << j; v_end[j] = e
        if single or e >= 64: break
        lo = e if touching else e + 1
    if mm == 0: mm, v_end[a0 + 1] = 1 << (a0 + 1), a0 + 9
    jl = ew.msb(mm)
    if last_over is not None: v_end[jl] = max(jl + 4, last_over)
    return mm, v_end, a0


def _check_run(mm, v_end, a0):
    E = ew.ends_mask(mm, v_end)
    assert ew.cover_sub(E, mm) == ew.run_cover(mm, v_end), (hex(mm), [v_end[j] for j in ew.bits(mm)])
    lit = ew.litmask_scalar(mm, E, a0)
    assert lit == ew.litmask_ballot(mm, v_end, a0)
    for i in ew.bits(mm | lit):
        assert ew.pend_ends(E, a0, i) == ew.pend_permute(mm, v_end, a0, i), (i, hex(mm), hex(E), a0)


def test_cover_pend_and_literals_on_random_runs():
    rng = random.Random(28)
    for _ in range(3000):
        _check_run(*_random_run(rng))
    for over in (62, 63, 64, 65, 80, 110):
        for _ in range(300):
            _check_run(*_random_run(rng, last_over=over))
    for _ in range(600):
        _check_run(*_random_run(rng, touching=True))                 # e == j of the next match: no literals
    for _ in range(300):
        _check_run(*_random_run(rng, single=True))


def test_named_runs():
    v = [i + 4 for i in range(64)]
    # one match at lane 63: mm_run << 1 is 0, nothing is covered
    assert ew.cover_sub(0, 1 << 63) == 0 == ew.run_cover(1 << 63, v)
    # lanes 5 -> 20 and 20 -> 70: touching, the last one past the window
    v[5], v[20] = 20, 70
    mm = (1 << 5) | (1 << 20)
    E = ew.ends_mask(mm, v)
    assert E == 1 << 20
    assert ew.cover_sub(E, mm) == (((1 << 20) - 1) & ~((1 << 6) - 1)) | (((1 << 64) - 1) & ~((1 << 21) - 1))
    assert ew.pend_ends(E, 2, 20) == 20 and ew.pend_ends(E, 2, 5) == 2 and ew.pend_ends(E, 2, 4) == 2
    _check_run(mm, v, 2)
    # an end at lane 63 has its bit: lane 63 is not covered
    v[20] = 63
    assert not (ew.cover_sub(ew.ends_mask(mm, v), mm) >> 63) & 1
    _check_run(mm, v, 0)


def _random_window(rng):
    dens = rng.choice((0.02, 0.1, 0.3, 0.7))
    vom = sum(1 << i for i in range(64) if rng.random() < dens)
    nsing = sum(1 << i for i in range(1, 64) if rng.random() < rng.choice((0.0, 0.1, 0.4)))
    mlo = [rng.choice((0, 1, 3, 8, 11, 12, 20, 43, 44)) for _ in range(64)]
    lt44 = sum(1 << i for i in range(64) if mlo[i] < 44)
    cfast = vom & lt44
    slow = (nsing & ~cfast) | (vom & ~lt44)
    return cfast, slow & ew.M64, nsing, vom, mlo, [i + 4 + mlo[i] for i in range(64)]


def test_steps_and_exact_inputs_from_masks():
    rng = random.Random(29)
    for _ in range(1500):
        cfast, slow, nsing, vom, mlo, v_end = _random_window(rng)
        PKo, XP, Qo = ew.steps_old(cfast, slow, nsing, vom, mlo, v_end)
        PK, X, Q = ew.steps_new(cfast, slow, nsing, vom, mlo, v_end)
        for f in range(64):
            if PKo[f] == ew.M32:
                assert PK[f] == ew.M32
            else:
                j, e = PKo[f] & 63, PKo[f] >> 6
                assert PK[f] & 63 == j and (PK[f] >> 6) & 127 == e + 1 and bool(PK[f] >> 31) == (e >= 63)
                assert PK[f] & ~(0x80000000 | 0x1FFF) == 0
            assert ew.exact_inputs_new(X, Q, f) == ew.exact_inputs_old(XP, Qo, f)


def test_one_test_trip_consumes_what_the_two_test_trip_did():
    rng = random.Random(30)
    for _ in range(1500):
        cfast, slow, nsing, vom, mlo, v_end = _random_window(rng)
        PKo = ew.steps_old(cfast, slow, nsing, vom, mlo, v_end)[0]
        PK = ew.steps_new(cfast, slow, nsing, vom, mlo, v_end)[0]
        for f in (1, 2, 17, 40, 62, 63, 64):
            a = f - 1 if f > 1 else 0
            f2, a2, mm2, seqs2 = ew.fast_run_two_tests(PKo, f, a, 0)
            f1, a1, mm1, E1, seqs1 = ew.fast_run_one_test(PK, f, a, 0, 0)
            assert (f1, a1, mm1, seqs1) == (f2, a2, mm2, seqs2)
            assert E1 == sum(1 << e for _, e in seqs1 if e < 64)
            assert (a1 == a) == (not seqs1)                          # a moves iff a sequence was consumed


@pytest.fixture(scope="module")
def corpus():
    return rg.corpus() + [(n, b) for n, b in bg.corpus() if len(b) <= 4096]


def test_corpus_shows_every_event():
    assert rg.events() >= set(ew.EVENTS)


def test_both_forms_agree_on_every_window_and_the_bytes_are_the_oracles(oracle, corpus):
    seen = set()
    bad = [n for n, b in corpus if ew.compress_run_masks(b, events=seen, check=True) != oracle.compress_default(b)]
    assert not bad, "%d blocks: %s" % (len(bad), ", ".join(bad[:8]))
    assert seen >= set(ew.EVENTS)


def test_little_room(oracle, corpus):
    """capacities around the compressed size: the windows run `tight`, and a block that does not fit is refused"""
    for n, b in corpus[::9]:
        w = oracle.compress_default(b)
        assert ew.compress_run_masks(b, dst_len=len(w)) == w, n
        assert ew.compress_run_masks(b, dst_len=len(w) + 100) == w, n
        assert ew.compress_run_masks(b, dst_len=len(w) - 1) is None, n
