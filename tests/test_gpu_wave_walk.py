"""GPU: the wave-per-workflow walk (replay_body's WaveSource branch) at chunk edges, failures and arena limits.

Directed histories (tests/wave_walk_cases.py, pinned on the CPU by tests/test_wave_walk_cases.py), each replayed
by one wavefront, compared with the oracle in every field, bit for bit, in three layouts: the default segments
(``tiered``: replay_tail_kernel, and replay_big_kernel past 64 entries in a map), every workflow in
replay_tail_kernel (``tail_only``) and the tail inside the lane kernels' launch (``untiered``:
replay_lds_small_kernel, or replay_lds_kernel once a 41-activity workflow is in the batch, ``untiered_large``).
Each case runs with and without task emission: without it a chunk of common types is resolved lane-parallel,
with it the same chunk takes the per-event walk and the task rows are compared too.
"""
import numpy as np
import pytest

import wave_walk_cases as wc
from cadence_amd import abi, synth
from cadence_amd.flatten import flatten, interleave
from cadence_amd.result import diff_results, to_canonical_order
from resume_cases import KNOWN, compare_split_with_one_shot, load_stable

pytestmark = pytest.mark.gpu

LAYOUTS = wc.LAYOUTS + ("untiered_large",)


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


def _oracle():
    from oracle import oracle
    return oracle


def _layout(hs, layout, emit=False, loaded=None):
    """The histories as one wavefront each.  ``untiered_large``: a 41-activity workflow joins the batch (last in
    canonical order), so the untiered launch is replay_lds_kernel's and not the small tier's."""
    if layout == "untiered_large":
        assert loaded is None
        hs = hs + [wc._history(wc.staircase(9000, "act", 41).walk, 9000)]
    canon = flatten(hs, known_domains=KNOWN, loaded=loaded)
    return wc.wave_layout(canon, "untiered" if layout == "untiered_large" else layout, emit)


def check(engine, b):
    """Replay on the device, twice: every workflow against the oracle, every field; the retry lists, the retry
    pass's block count and the big segment's gate counter zeroed after each launch (the second launch starts
    from what the first left)."""
    import torch
    db = engine.upload(b)
    want = _oracle().replay(b, 0)
    assert want.exec.shape[0] == b.n_wf
    for _ in range(1 if b.init is not None else 2):   # a resumed replay continues its rows in place: one launch
        engine.launch(db)
        got = engine.download(db)
        torch.cuda.synchronize()
        sc = db.tensors["scratch"][:4].cpu().numpy()
        assert (sc == 0).all(), sc
        d = diff_results(b, got, b, want)
        assert not d, "\n".join(d)
    return got, db


@pytest.fixture(scope="module")
def chain_batch():
    b = interleave(synth.activity_chain(256, 3, synth.SEED_C1))
    return b, _oracle().replay(b, 0)


def _chain_still_right(engine, chain_batch):
    """A launch of the small activity-chain batch after the one under test still equals the oracle."""
    b, want = chain_batch
    d = diff_results(b, engine.replay(b), b, want)
    assert not d, "\n".join(d)


def _assert_untiered_kernel(b, db, layout):
    if layout == "untiered":
        assert db.c_in.flags & abi.IN_LDS_SMALL
    elif layout == "untiered_large":
        assert not db.c_in.flags & abi.IN_LDS_SMALL


@pytest.fixture(scope="module")
def fail_cases():
    cases = wc.failure_cases()
    return cases, wc.failure_histories(cases)


@pytest.mark.parametrize("emit", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_failures_with_events_after_them(engine, chain_batch, fail_cases, layout, emit):
    """A failing event at lanes 0, 1, 31, 62, 63 of chunk 1 and lanes 0, 63 of chunk 2 (event ID not increasing,
    lower version, invalid version, empty batch; missing activity, missing child, unknown domain, unknown type,
    DecisionTaskStarted without its decision), two failures in one chunk in both orders, and the lane loop's
    failure kinds inside an activity chain -- each followed by events that would change the state.  Every field
    equals the oracle's, status and fail_step are the planned ones, and the device's replay of the history cut
    after the failing event gives the same exec row (but src_next), live rows and version-history items."""
    cases, hs = fail_cases
    b = _layout(hs, layout, emit)
    got, db = check(engine, b)
    _assert_untiered_kernel(b, db, layout)
    ex = to_canonical_order(b, got)
    pos = wc.device_pos(b)
    for i, c in enumerate(cases):
        full, cut = 2 * i, 2 * i + 1
        for w in (full, cut):
            assert ex["status"][w] == c.status and ex["fail_step"][w] == c.fail_step, \
                (c.name, w, ex["status"][w], ex["fail_step"][w])
        differ = {f for f in abi.EXEC_ROW.names if ex[f][full] != ex[f][cut]}
        assert differ <= {"src_next", "reserved"}, (c.name, differ)
        la, lb = got.live_rows(b, int(pos[full])), got.live_rows(b, int(pos[cut]))
        for name in la:
            assert la[name].shape == lb[name].shape, (c.name, name)
            for f in la[name].dtype.names:
                if f != "reserved":
                    assert (la[name][f] == lb[name][f]).all(), (c.name, name, f)
    _chain_still_right(engine, chain_batch)


def _edge_histories():
    cases, hs = [], []
    for E in wc.EDGES:
        ec = wc.edge_cases(E)
        cases += ec
        hs += [wc._history(c.build(i), E * 1000 + i) for i, c in enumerate(ec)]
        hs += wc.ragged_histories(E * 1000 + 500)
    return cases, hs


@pytest.mark.parametrize("emit", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_state_carried_across_a_chunk_edge(engine, chain_batch, layout, emit):
    """For the edges 64 and 128: a decision scheduled at lane 63 and started at lane 0, completed at lane 0 with an
    insert behind it; failed and timed-out decisions with the transient pair in the next chunk, two and three
    failures straddling the edge and ending on one, attempts counted on from a carried decision; batches first at
    lane 63 and last at lane 0, histories of exactly 64 and 128 events, of 63, 65, 127, 129 and 192; version bumps
    at lane 0, lane 63, both, and in all 64 lanes of a chunk; maps dirtied in one chunk whose batch ends at lane 0
    of the next; reset points repeated inside a chunk and in the next.  All valid and left open, so the carried
    fields are the exec row's: every field equals the oracle's."""
    cases, hs = _edge_histories()
    b = _layout(hs, layout, emit)
    got, db = check(engine, b)
    _assert_untiered_kernel(b, db, layout)
    ex = to_canonical_order(b, got)
    assert (ex["status"] == 0).all()
    assert sorted(b.wf["ev_count"])[:2] == [63, 63]
    assert {64, 128, 192} <= set(int(x) for x in b.wf["ev_count"])
    _chain_still_right(engine, chain_batch)


@pytest.mark.parametrize("layout", wc.LAYOUTS)
def test_state_carried_in_from_a_loaded_row(engine, layout):
    """The decision, failed-decision, batch and version cases as resumed replays: cut at the batch boundary
    nearest E - 64 (the suffix's first chunk is lane-parallel, its carried state the loaded row's) and nearest E
    (the state the edge carries is the loaded row itself).  The loaded states are the oracle's replay of the
    prefix; the suffix equals the oracle's and, for every split workflow, the one-shot device replay."""
    whole, pre, suf = [], [], []
    for E in wc.EDGES:
        for i, c in enumerate(wc.edge_cases(E)):
            if c.group not in wc.RESUME_GROUPS:
                continue
            for target in (E - 64, E):
                h = wc._history(c.build(i), E * 1000 + i)
                p, s, _cut = wc.split_at(h, target)
                whole.append(h)
                pre.append(p)
                suf.append(s)
    n = len(whole)
    assert n >= 80
    one_b = _layout(whole, layout)
    one, _ = check(engine, one_b)
    pre_b = flatten(pre, known_domains=KNOWN)
    pre_r = _oracle().replay(pre_b, 0)
    assert (pre_r.exec["status"] == 0).all()
    loaded = pre_r.to_loaded(pre_b, mask=np.ones(n, bool))
    suf_b = _layout(suf, layout, loaded=loaded)
    assert ((suf_b.wf["flags"] & abi.WF_FLAG_RESUME) != 0).all()
    if layout == "tiered":
        assert suf_b.tiers[-1] == 0          # loaded states: the replay_big_kernel segment
    elif layout == "tail_only":
        assert suf_b.tiers[-1] == n          # replay_tail_kernel's resume instantiation
    suf_r, _ = check(engine, suf_b)
    assert (to_canonical_order(suf_b, suf_r)["status"] == 0).all()
    compared = compare_split_with_one_shot(one_b, one, pre_r.exec, suf_b, suf_r, load_stable(loaded))
    assert compared == n


@pytest.fixture(scope="module")
def stairs():
    st = wc.staircases()
    return st, [wc._history(s.walk, i) for i, s in enumerate(st)]


@pytest.mark.parametrize("layout", wc.LAYOUTS)
def test_arena_limits_every_route(engine, chain_batch, stairs, layout):
    """One workflow per (map, size): a map filled in one batch to an arena limit or one past it, every second entry
    closed, two more inserted; for the sizes that cross a register of the row tables, slots 63 and 64 freed and
    re-used and the last entry looked up by ActivityID / TimerID.  tiered: up to 64 entries in the tail kernel (its
    64/48/24/16/16/32 arena, then the retry wave list), above in replay_big_kernel (128 fits its segment arena,
    129 takes the 320/160/96/64/64/64 arena, 321 the HBM rows); tail_only: everything starts in the tail kernel;
    untiered: in replay_lds_kernel's wave tail.  The segment of every workflow is asserted, so each route is taken
    by construction, and the live counts are the planned ones."""
    st, hs = stairs
    b = _layout(hs, layout)
    pos = wc.device_pos(b)
    big = np.array([s.n > 64 for s in st])
    if layout == "tiered":
        assert b.tiers[-1] == b.n_wf - big.sum() and ((pos >= b.tiers[-1]) == big).all()
    elif layout == "tail_only":
        assert b.tiers[-1] == b.n_wf
    else:
        assert b.tiers is None
    got, db = check(engine, b)
    assert db.c_in.wave_begin == 0 and not db.c_in.flags & abi.IN_LDS_SMALL
    if layout != "untiered":
        assert db.c_in.big_begin == b.tiers[-1]
    ex = to_canonical_order(b, got)
    assert (ex["status"] == 0).all()
    for i, s in enumerate(st):
        for m, f in wc.COUNT_FIELD.items():
            assert ex[f][i] == (s.final if m == s.map else 1 if m == "rp" else 0), (s.name, m, ex[f][i])
    _chain_still_right(engine, chain_batch)


@pytest.mark.parametrize("layout", ["tiered", "untiered"])
def test_small_wave_arena_flag(engine, chain_batch, stairs, layout):
    """The workflows within 40/32/16/8/8/24 entries run with CRR_IN_LDS_SMALL (untiered: the wave tail of
    replay_lds_small_kernel); the 41-activity workflow beside them clears it.  Both batches equal the oracle."""
    st, hs = stairs
    small = [h for h, s in zip(hs, st) if wc.in_small_arena(s)]
    assert len(small) == 6
    b = _layout(small, layout)
    got, db = check(engine, b)
    assert db.c_in.flags & abi.IN_LDS_SMALL
    b = _layout(small + [hs[[s.name for s in st].index("act-41")]], layout)
    got, db = check(engine, b)
    assert not db.c_in.flags & abi.IN_LDS_SMALL
    _chain_still_right(engine, chain_batch)
