"""The window epilogue of k_compress_fast on the CPU (no GPU, pure Python): the covered mask that flushes and immediate
emissions accumulate (cov_acc) against the definition it replaced -- nearest match lane strictly below, over every
flushed and pending match lane, ORed with the lanes of the immediately emitted matches -- and the one-write table
commit against restore-then-commit.  The new forms are the ones of tools/emulate_window.py."""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import emulate_window as ew   # noqa: E402

ALL = (1 << 64) - 1


def below(i):
    return (1 << min(i, 64)) - 1


def covered_by_definition(mm_all, v_end, covered_x):
    """covered_now() as it was: per lane the nearest match lane strictly below it among all match lanes of the window's
    runs, flushed or pending; the lane is inside that match if it lies below its end"""
    m = covered_x
    pj = -1                             # nearest match lane strictly below lane i
    for i in range(64):
        if pj >= 0 and i < v_end[pj]:
            m |= 1 << i
        if (mm_all >> i) & 1:
            pj = i
    return m


def play(events, v_end):
    """events: ("run", [(j, e), ...]) = matches that join the pending run, flushed at the next immediate emission or at
    the window's end; ("imm", j, e) = a match emitted immediately.  After every event the covered mask an exact step
    would use (cov_acc, plus the pending run's own lanes while one is pending) is compared with the definition.
    -> the window's final covered mask."""
    v_end = list(v_end)
    cov_acc = covered_x = mm_win = mm_run = 0

    def check():
        new = cov_acc | (ew.run_cover(mm_run, v_end) if mm_run else 0)
        assert new == covered_by_definition(mm_win | mm_run, v_end, covered_x)

    def flush():
        nonlocal cov_acc, mm_win, mm_run
        cov_acc |= ew.run_cover(mm_run, v_end)
        mm_win |= mm_run
        mm_run = 0

    for ev in events:
        if ev[0] == "run":
            for j, e in ev[1]:
                v_end[j] = e            # (an exact step rewrites v_end of its own lane; a fast-run match has it already)
                mm_run |= 1 << j
                check()
        else:
            _, j, e = ev
            if mm_run:
                flush()
            covered_x |= ew.imm_cover(j, e)
            cov_acc |= ew.imm_cover(j, e)
            check()
    if mm_run:
        flush()
    assert mm_run == 0
    check()
    return cov_acc


def two_step_commit(table, h, mine, old, wr, grp, ins):
    for i in range(64):
        if wr[i] and not (ins >> i) & 1:
            table[h[i]] = old[i]
    for i in range(64):
        if (ins >> i) & 1 and (grp[i] & ins & ~below(i) & ~(1 << i)) == 0:
            table[h[i]] = mine[i]


def check_commit(rng, h, wr, ins):
    """both commits from the state the speculative put leaves (any lane of a group may have won the race)"""
    wrmask = sum(1 << i for i in range(64) if wr[i])
    assert ins & ~wrmask == 0
    slots = sorted(set(h))
    before = {s: rng.randrange(0, 60000) for s in slots}
    old = [before[h[i]] if wr[i] else 0 for i in range(64)]
    mine = [100000 + i for i in range(64)]
    members = {}
    for i in range(64):
        if wr[i]:
            members.setdefault(h[i], []).append(i)
    grp = [sum(1 << k for k in members[h[i]]) if wr[i] else 1 << i for i in range(64)]
    spec = dict(before)
    for s, m in members.items():
        spec[s] = mine[rng.choice(m)]
    t_old, t_new = dict(spec), dict(spec)
    two_step_commit(t_old, h, mine, old, wr, grp, ins)
    writes = ew.commit_one_write(t_new, h, mine, old, wr, grp, ins)
    assert t_new == t_old
    by_slot = {}
    for lane, slot, v in writes:
        assert by_slot.setdefault(slot, v) == v, "lanes write different values to one slot"
    assert len(set(lane for lane, _, _ in writes)) == len(writes)
    # and the table is what the serial loop leaves: the last put of every slot, else untouched
    for s in slots:
        put = [i for i in members.get(s, ()) if (ins >> i) & 1]
        assert t_new[s] == (mine[put[-1]] if put else before[s])


def random_window(rng):
    """a random split of the 64 lanes into runs and immediate sequences of non-overlapping matches"""
    v_end = [rng.randrange(0, 130) for _ in range(64)]          # lanes that never match hold anything
    events, run = [], []
    f = 1
    p_match = rng.choice((0.0, 0.05, 0.15, 0.4))
    p_imm = rng.choice((0.0, 0.2, 0.6))
    a = 0
    while f < 64:
        if rng.random() >= p_match:
            f += 1
            continue
        j = f
        e = j + 4 + rng.choice((0, 1, 3, 8, 20, 44, 60 - j, 64 - j - 4, 300))
        e = max(e, j + 4)
        if rng.random() < p_imm:
            if run:
                events.append(("run", run))
                run = []
            events.append(("imm", j, e))
        else:
            run.append((j, e))
        a = e
        f = e + 1
    if run:
        events.append(("run", run))
    return events, v_end, a


def random_hashes(rng):
    nslots = rng.choice((2, 5, 20, 64, 4096))
    return [rng.randrange(nslots) for _ in range(64)]


def finish(rng, events, v_end, a, has_ins=None, generic=False, h=None):
    cov = play(events, v_end)
    has_ins = rng.random() < 0.8 if has_ins is None else has_ins
    wr = [has_ins or i > 0 for i in range(64)]
    wrmask = sum(1 << i for i in range(64) if wr[i])
    f_end = 64 if generic or a >= 64 else a + 1
    ins = ew.ins_mask(wrmask, cov, f_end)
    # `ins` as it was: from the definition of the covered lanes
    mm = sum(1 << j for ev in events if ev[0] == "run" for j, _ in ev[1])
    ve = list(v_end)
    cx = 0
    for ev in events:
        if ev[0] == "run":
            for j, e in ev[1]:
                ve[j] = e
        else:
            cx |= ew.imm_cover(ev[1], ev[2])
    assert ins == wrmask & ~covered_by_definition(mm, ve, cx) & below(f_end)
    check_commit(rng, h if h is not None else random_hashes(rng), wr, ins)
    return ins


def test_random_windows():
    rng = random.Random(20240611)
    seen_imm_then_run = seen_two_flushes = seen_end_64 = seen_past_64 = 0
    for _ in range(2000):
        events, v_end, a = random_window(rng)
        kinds = [ev[0] for ev in events]
        seen_imm_then_run += any(x == "imm" and y == "run" for x, y in zip(kinds, kinds[1:]))
        seen_two_flushes += kinds.count("run") > 1
        seen_end_64 += a == 64
        seen_past_64 += a > 64
        finish(rng, events, v_end, a, generic=(not events))
    assert min(seen_imm_then_run, seen_two_flushes, seen_end_64, seen_past_64) > 50


def test_no_match_at_all():
    rng = random.Random(1)
    for has_ins in (False, True):
        ins = finish(rng, [], [rng.randrange(130) for _ in range(64)], 0, has_ins=has_ins, generic=True)
        assert ins == (ALL if has_ins else ALL & ~1)


def test_match_ending_exactly_at_lane_64():
    rng = random.Random(2)
    v_end = [7] * 64
    ins = finish(rng, [("run", [(3, 9), (40, 64)])], v_end, 64, has_ins=True)
    assert ins == ALL & ~(below(9) & ~below(4)) & ~(below(64) & ~below(41))
    ins = finish(rng, [("imm", 40, 64)], v_end, 64, has_ins=True)
    assert ins == below(41)


def test_immediate_sequence_then_run_in_one_window():
    rng = random.Random(3)
    v_end = [0] * 64        # lane values that would cover nothing if the immediate match were looked up as a run match
    ins = finish(rng, [("run", [(2, 8)]), ("imm", 10, 30), ("run", [(33, 40), (45, 52)])], v_end, 52, has_ins=True)
    want = below(53) & ~(below(8) & ~below(3)) & ~(below(30) & ~below(11)) & ~(below(40) & ~below(34)) & \
        ~(below(52) & ~below(46))
    assert ins == want


def test_group_whose_only_ins_lane_is_its_lowest():
    rng = random.Random(4)
    h = list(range(64))
    h[5] = h[12] = h[20] = 4000        # lanes 12 and 20 lie inside the match at lane 10
    ins = finish(rng, [("run", [(10, 30)])], [0] * 64, 30, has_ins=True, h=h)
    assert (ins >> 5) & 1 and not (ins >> 12) & 1 and not (ins >> 20) & 1


def test_group_with_no_ins_lane():
    rng = random.Random(5)
    h = list(range(64))
    h[12] = h[20] = h[50] = 4000       # two lanes inside the match, one past the frontier
    ins = finish(rng, [("run", [(10, 30)])], [0] * 64, 30, has_ins=True, h=h)
    assert ins & ((1 << 12) | (1 << 20) | (1 << 50)) == 0
