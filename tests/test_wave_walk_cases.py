"""CPU: the fixtures of tests/test_gpu_wave_walk.py pinned against the oracle.

Every planned step index and lane, the oracle's status and fail_step of every failure case, the truncation
property (a history cut after its failing event replays to the same row) in the oracle itself, the exact
live-set bounds of the staircases, the segment each is placed in under the three layouts, and that the cases
meant for the lane-parallel chunks hold none of the types that force the per-event walk.  With these fixed a
failure of the GPU file can only mean the kernel.
"""
import numpy as np
import pytest

import wave_walk_cases as wc
from cadence_amd import abi
from cadence_amd.abi import EventType as ET
from cadence_amd.flatten import WAVE_BIG_CAPS, WAVE_SMALL_TIER, fits_small_tier, live_set_bounds
from cadence_amd.result import diff_results


def _oracle():
    from oracle import oracle
    return oracle


def _rows_equal(res, batch, a, b):
    la, lb = res.live_rows(batch, a), res.live_rows(batch, b)
    for name in la:
        assert la[name].shape == lb[name].shape, name
        for f in la[name].dtype.names:
            if f != "reserved":
                assert (la[name][f] == lb[name][f]).all(), (name, f)


def test_failure_cases_plan():
    """The failing event sits at its planned step (lanes 0, 1, 31, 62, 63 of chunk 1, lanes 0 and 63 of chunk 2),
    events follow it, and only the ``type`` cases put a rare type into the failing chunk."""
    cases = wc.failure_cases()
    assert len({c.name for c in cases}) == len(cases)
    singles = [c for c in cases if "+" not in c.name and not c.name.startswith("chain:")]
    assert len(singles) == 9 * 7
    assert sorted({c.fail_step % 64 for c in singles if c.fail_step < 128}) == [0, 1, 31, 62, 63]
    assert sorted({c.fail_step % 64 for c in singles if c.fail_step >= 128}) == [0, 63]
    want_type = {"activity": ET.ActivityTaskStarted, "child": ET.ChildWorkflowExecutionStarted,
                 "domain": ET.ActivityTaskScheduled, "type": 99, "decision": ET.DecisionTaskStarted,
                 "id": ET.WorkflowExecutionSignaled, "version": ET.WorkflowExecutionSignaled,
                 "invalid": ET.WorkflowExecutionSignaled}
    for i, c in enumerate(cases):
        k = c.build(i)
        ty = wc.types_of(k)
        s, c0 = c.fail_step, c.fail_step // 64 * 64
        assert 64 <= s < 192 and len(ty) >= s + 14, c.name        # the tail (or the chain's rest) follows
        kind = c.name.split(":")[-1].split("@")[0]
        if kind == "empty":    # the empty batch is before the event at the failing step
            n = 0
            for b in k.batches:
                if not b:
                    break
                n += len(b)
            assert n == s, c.name
        elif not c.name.startswith("chain:") or kind in ("type", "activity"):
            assert ty[s] == int(want_type[kind]), (c.name, ty[s])
        assert c.fast == (not any(wc.is_rare(t) for t in ty[c0:c0 + 64])), c.name
        if not c.name.startswith("chain:"):   # the tail's state-changing events are among those after the failure
            after = set(ty[s + 1:])
            assert {int(ET.WorkflowExecutionCancelRequested), int(ET.DecisionTaskScheduled), int(ET.TimerStarted),
                    int(ET.DecisionTaskCompleted), int(ET.WorkflowExecutionSignaled)} <= after, c.name
            assert k.batches[-1][-1].version >= 11
    two = [c for c in cases if "+" in c.name]
    assert len(two) == len(wc.TWO_FAILURES)
    pro, walk = set(wc.PROLOGUE_KINDS), set(wc.WALK_KINDS)
    orders = {(f in pro, s in pro) for f, _a, s, _b in wc.TWO_FAILURES}
    assert orders == {(True, False), (False, True), (False, False)}
    assert all(f in pro | walk and s in pro | walk for f, _a, s, _b in wc.TWO_FAILURES)


@pytest.mark.parametrize("emit", [False, True])
def test_failure_cases_in_the_oracle(emit):
    """The oracle's status and fail_step are the planned ones (of two failures the earlier step wins), and the
    history cut after its failing event gives the same exec row -- only src_next differs -- the same live rows
    and the same version-history items: nothing after a failure reaches the state."""
    cases = wc.failure_cases()
    b = wc.flat(wc.failure_histories(cases))
    b.emit_tasks = emit
    r = _oracle().replay(b, 0)
    for i, c in enumerate(cases):
        for w in (2 * i, 2 * i + 1):
            assert r.exec["status"][w] == c.status and r.exec["fail_step"][w] == c.fail_step, \
                (c.name, r.exec["status"][w], r.exec["fail_step"][w])
        assert b.wf["ev_count"][2 * i + 1] == c.fail_step + 1 < b.wf["ev_count"][2 * i]
        differ = {f for f in abi.EXEC_ROW.names if r.exec[f][2 * i] != r.exec[f][2 * i + 1]}
        assert differ <= {"src_next", "reserved"}, (c.name, differ)
        _rows_equal(r, b, 2 * i, 2 * i + 1)


def _edge_histories(E):
    cases = wc.edge_cases(E)
    return cases, [wc._history(c.build(i), E * 1000 + i) for i, c in enumerate(cases)]


@pytest.mark.parametrize("E", wc.EDGES)
def test_edge_cases_plan(E):
    """Every planned event is at its step, the histories are valid and left open, no chunk after the first holds
    a rare type, and the histories meant to end at a chunk edge have exactly E events."""
    cases, hs = _edge_histories(E)
    assert {c.group for c in cases} == {"decision", "failed", "batch", "version", "timer", "reset"}
    b = wc.flat(hs + wc.ragged_histories(E * 1000 + 500))
    r = _oracle().replay(b, 0)
    assert (r.exec["status"] == 0).all()
    assert (r.exec["state"][:len(cases)] == abi.State.Running).all()
    assert list(b.wf["ev_count"][len(cases):]) == list(wc.RAGGED_COUNTS)
    by_name = {}
    for i, c in enumerate(cases):
        ty = [int(e.event_type) for e in hs[i].events]
        by_name[c.name.rsplit("@", 1)[0]] = i
        for s, t in c.plan.items():
            assert ty[s] == t, (c.name, s, ty[s], t)
        assert not any(wc.is_rare(t) for t in ty[64:]), c.name
    ex, n = r.exec, b.wf["ev_count"]
    for name in ("scheduled|", "batch last at 63, nothing after", "batch cut at 63"):
        assert n[by_name[name]] == E, name
    # the decision fields the carried-state arms produce
    i = by_name["scheduled,started|completed,activity"]
    assert ex["n_activity"][i] == 1 and ex["decision_schedule_id"][i] == abi.EMPTY_EVENT_ID
    i = by_name["batch first at 63, activity insert at 0"]
    act = r.live_rows(b, i)["act"]
    assert act["scheduled_batch_id"][0] == E and act["schedule_id"][0] == E + 1   # IDs are step + 1
    for last in (0, 1, 2):
        for k in (2, 3):
            i = by_name[f"{k} failures, last at {last}"]
            assert n[i] == E + last + 1 and ex["decision_attempt"][i] == 1
            # the transient decision's ScheduleID: NextEventID when the failure is applied (the batch end before it)
            assert ex["decision_schedule_id"][i] == E + last + 1 and ex["next_event_id"][i] == E + last + 2
    for name in ("scheduled(attempt 2)|timed out", "|scheduled(attempt 2), timed out"):
        assert ex["decision_attempt"][by_name[name]] == 3, name
    assert ex["decision_attempt"][by_name["failed|timed out, nothing between"]] == 2
    for name, at in (("failed, started inside a chunk", E + 12), ("|failed at 0, started", E), ("failed|started", E - 1)):
        i = by_name[f"transient: {name}"]   # started on the transient decision's ScheduleID, the failed event's ID
        assert ex["decision_schedule_id"][i] == at + 1 and ex["decision_started_id"][i] == at + 2, name
    for name, items in (("lane 0", 2), ("lane 63", 2), ("lanes 63 and 0", 3), ("lanes 0 and 63 of one chunk", 3),
                        ("all 64 lanes", 65)):
        assert ex["n_vh_items"][by_name[f"version bump at {name}"]] == items, name
    i = by_name["dirty maps, batch end at 0"]
    assert ex["n_activity"][i] == 1 and ex["n_timer"][i] == 1
    assert r.live_rows(b, i)["timer"]["task_status"][0] != 0 and r.live_rows(b, i)["act"]["timer_task_status"][0] != 0
    assert ex["n_reset_points"][by_name["reset point dedup"]] == 3   # bin-0, rp-x, rp-new


@pytest.mark.parametrize("E", wc.EDGES)
def test_edge_cases_split_for_resume(E):
    """The resumed runs cut every history of the first four groups at the batch boundary nearest E - 64 (the
    suffix's first chunk is then lane-parallel) and nearest E (the edge's carried state is the loaded row's);
    the prefix replays OK and Load reproduces it, so every one is in the comparison with the one-shot replay."""
    from resume_cases import load_stable
    cases, hs = _edge_histories(E)
    sel = [i for i, c in enumerate(cases) if c.group in wc.RESUME_GROUPS]
    assert len(sel) >= 20
    for target in (E - 64, E):
        parts = [wc.split_at(hs[i], target) for i in sel]
        for (pre, suf, cut), i in zip(parts, sel):
            assert pre.batches and suf.batches and cut + len(suf.events) == len(hs[i].events)
            assert abs(cut - target) <= 3, (cases[i].name, cut)
        pb = wc.flat([p[0] for p in parts])
        pr = _oracle().replay(pb, 0)
        assert (pr.exec["status"] == 0).all()
        loaded = pr.to_loaded(pb, mask=np.ones(pb.n_wf, bool))
        assert load_stable(loaded).all()


def test_staircase_bounds_are_exact():
    """live_set_bounds returns exactly the planned size for every map, the final live counts are the planned ones
    and no workflow is longer than about 1,000 events."""
    st = wc.staircases()
    assert len(st) == sum(len(v) for v in wc.STAIR_SIZES.values()) + sum(len(v) for v in wc.CROSS_SIZES.values())
    b = wc.flat([wc._history(s.walk, i) for i, s in enumerate(st)])
    assert b.wf["ev_count"].max() <= 1000
    lb = live_set_bounds(b)
    r = _oracle().replay(b, 0)
    assert (r.exec["status"] == 0).all()
    for i, s in enumerate(st):
        assert lb[s.map][i] == s.n, (s.name, lb[s.map][i])
        for m, f in wc.COUNT_FIELD.items():
            if m != s.map:
                assert lb[m][i] == (1 if m == "rp" else 0) and r.exec[f][i] == (1 if m == "rp" else 0), (s.name, m)
        assert r.exec[wc.COUNT_FIELD[s.map]][i] == s.final, (s.name, r.exec[wc.COUNT_FIELD[s.map]][i])
    assert wc.WAVE_SMALL == WAVE_SMALL_TIER
    # every arena limit and the size one above it: 40/32/16/8/8/24 (small per-wave arena), 64/48/24/16/16/32 (the tail
    # kernel's), 64 and 128 (host routing, the big segment's arena), 320/160/96/64/64/64 (the retry arena)
    for m, limits in {"act": (40, 64, 128, 320), "timer": (32, 48, 128, 160), "child": (16, 24, 64, 96),
                      "rc": (8, 16, 64), "sig": (8, 16, 64), "rp": (24, 32, 64)}.items():
        for lim in limits:
            assert lim in wc.STAIR_SIZES[m] and lim + 1 in wc.STAIR_SIZES[m], (m, lim)
    # the cross cases re-use slots 63 and 64, and the activity looked up by ActivityID lives in slot >= 64 (or 63)
    for s in st:
        if s.cross:
            assert s.final == s.n
            if s.map == "act":
                ev = [e for bt in s.walk.batches for e in bt if e.event_type == ET.ActivityTaskCancelRequested]
                assert len(ev) == 1 and ev[0].attrs["activity_id"] == f"a{s.n - 1}"


def test_staircase_segments_under_the_three_layouts():
    """tiered: a workflow past 64 entries in a map is in the replay_big_kernel segment [tiers[-1], n), the others
    in the tail kernel's; tail_only: every workflow in the tail kernel's segment; untiered: no segments, the tail
    inside the lane kernel's launch.  Every workflow is a wavefront's in all three."""
    st = wc.staircases()
    hs = [wc._history(s.walk, i) for i, s in enumerate(st)]
    assert set(WAVE_BIG_CAPS.values()) == {64}
    b = wc.wave_layout(wc.flat(hs), "tiered")
    pos = wc.device_pos(b)
    big = np.array([s.n > 64 for s in st])
    assert 0 < b.tiers[-1] < b.n_wf and b.tiers[-1] == b.n_wf - big.sum()
    assert ((pos >= b.tiers[-1]) == big).all()
    assert b.tiers[:5] == (0, 0, 0, 0, 0)
    b = wc.wave_layout(wc.flat(hs), "tail_only")
    assert b.tiers[-1] == b.n_wf and b.wave_begin == 0
    b = wc.wave_layout(wc.flat(hs), "untiered")
    assert b.tiers is None and b.wave_begin == 0 and not fits_small_tier(b)
    # the small per-wave arena: exactly the workflows within 40/32/16/8/8/24, and one more activity ends it
    small = [h for h, s in zip(hs, st) if wc.in_small_arena(s)]
    assert len(small) == 6
    for layout in ("tiered", "untiered"):
        assert fits_small_tier(wc.wave_layout(wc.flat(small), layout), lanes=False)
        one_more = small + [hs[[s.name for s in st].index("act-41")]]
        assert not fits_small_tier(wc.wave_layout(wc.flat(one_more), layout), lanes=False)


def test_layouts_agree_in_the_oracle():
    """The three layouts hold the same workflows: the oracle's rows are equal across them."""
    st = wc.staircases()[::5]
    hs = [wc._history(s.walk, i) for i, s in enumerate(st)]
    ref_b = wc.flat(hs)
    ref = _oracle().replay(ref_b, 0)
    for layout in wc.LAYOUTS:
        b = wc.wave_layout(wc.flat(hs), layout)
        d = diff_results(ref_b, ref, b, _oracle().replay(b, 0))
        assert not d, "\n".join(d)
