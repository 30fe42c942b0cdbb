"""Directed histories for the version-history prologue of the lane loop (replay_kernel.hip, replay_body).

Builders only, no GPU.  The lane loop tests one fused predicate per event -- a valid (ID, version), the version
of the history's last item, a larger ID, an open workflow, not the empty batch -- with a single ballot, and a
wavefront in which any lane misses it takes the full checks for that step.  A batch here is ``n`` activity
chains of 23 events that replay in lockstep, with one workflow of every wavefront perturbed in one way
(``KINDS``), so that on the perturbed step the wavefront takes the full checks with 63 usual lanes beside the
unusual one.  Every exit of the prologue is a kind: the five error codes, version growth with room for the item
and without, the empty batch at the first step, a middle step and past the last event, events after the
workflow closed, and a failure on the first and on the last event.

tests/test_lane_prologue_cases.py pins each kind's status and failing step against the CPU oracle;
tests/test_gpu_lane_prologue.py replays the batches on the device.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from cadence_amd import abi
from cadence_amd.abi import EventType as ET
from cadence_amd.flatten import HistoryBatch, flatten
from cadence_amd.history import WorkflowHistory
from cadence_amd.synth_mixed import _Walk

from wave_walk_cases import KNOWN, _history, chain

EVENTS = 23            # chain(w, 3); every kind keeps the count, so the device order is the canonical one
MID = 12               # ActivityTaskCompleted of the second round, the first event of its batch: one pending activity
LAST = EVENTS - 1
SIZES = (1, 63, 64, 65, 129)   # partial wavefronts, a full one, a block boundary (128 lanes) plus one lane

S = abi.Status


@dataclasses.dataclass
class Kind:
    build: Callable[[int], _Walk]
    status: int
    fail_step: int                     # -1: replays to the end
    vh_cap: Optional[int] = None       # the version-history capacity when not the flattener's (the interleaved layout
                                       # gives a wavefront's lanes one capacity, their largest: the other lanes need 1)
    vh_items: Optional[int] = None     # items of an OK replay


def _events(k: _Walk):
    return [e for b in k.batches for e in b]


def _edit(step: int, fn) -> Callable[[int], _Walk]:
    def build(w):
        k = chain(w, 3)
        fn(_events(k)[step], _events(k)[step - 1] if step else None)
        return k
    return build


def _neg_id(e, _p):
    e.id = -e.id


def _neg_version(e, _p):
    e.version = -7


def _empty_version(e, _p):
    e.version = abi.EMPTY_VERSION      # a valid item, but below the history's version


def _lower(e, _p):
    e.version -= 1


def _same_id(e, p):
    e.id = p.id


def _grow(w: int) -> _Walk:
    k = chain(w, 3)
    for e in _events(k)[MID:]:
        e.version += 1
    return k


def _empty_batch(before_step: int) -> Callable[[int], _Walk]:
    def build(w):
        k = chain(w, 3)
        at, n = 0, 0
        for at, b in enumerate(k.batches):
            if n == before_step:
                break
            n += len(b)
        else:
            at = len(k.batches)
        assert n == before_step or (before_step == EVENTS and at == len(k.batches))
        k.batches.insert(at, [])
        return k
    return build


def _after_completed(w: int) -> _Walk:
    """17 events that close the workflow, then six signals, the last at a higher version: it closes an item, and
    UpdateCurrentVersion leaves a closed workflow the version of the item before it."""
    k = chain(w, 2)
    for i in range(EVENTS - 17):
        if i == EVENTS - 18:
            k.version += 1
        k.emit([k.ev(ET.WorkflowExecutionSignaled)])
    return k


KINDS: Dict[str, Kind] = {
    # at a DecisionTaskStarted: a closing event with an odd ID makes the tier estimate expect two live activities
    "negative id": Kind(_edit(MID + 2, _neg_id), S.VH_INVALID_ITEM, MID + 2),
    "negative version": Kind(_edit(MID, _neg_version), S.VH_INVALID_ITEM, MID),
    "empty version": Kind(_edit(MID, _empty_version), S.VH_LOWER_VERSION, MID),
    "lower version": Kind(_edit(MID, _lower), S.VH_LOWER_VERSION, MID),
    "id not increasing": Kind(_edit(MID, _same_id), S.VH_EVENT_ID_NOT_INCREASING, MID),
    "growth with room": Kind(_grow, S.OK, -1, vh_items=2),
    "growth at capacity": Kind(_grow, S.CAPACITY, MID, vh_cap=1),
    "empty batch at 0": Kind(_empty_batch(0), S.EMPTY_HISTORY, 0),
    "empty batch in the middle": Kind(_empty_batch(MID), S.EMPTY_HISTORY, MID),
    "empty batch at the end": Kind(_empty_batch(EVENTS), S.EMPTY_HISTORY, EVENTS),
    "events after the close": Kind(_after_completed, S.OK, -1, vh_items=2),
    "first event fails": Kind(_edit(0, _neg_id), S.VH_INVALID_ITEM, 0),
    "last event fails": Kind(_edit(LAST, _lower), S.VH_LOWER_VERSION, LAST),
}
# every status the prologue can return for a history replayed from its first event
STATUSES = {int(S.EMPTY_HISTORY), int(S.VH_LOWER_VERSION), int(S.VH_EVENT_ID_NOT_INCREASING), int(S.VH_INVALID_ITEM),
            int(S.CAPACITY)}


def perturbed_lanes(n: int) -> List[int]:
    """One workflow of every wavefront of an n-workflow batch: lane 5 (or the last lane there is) of the even
    wavefronts, the last lane of the odd ones."""
    out = []
    for g, lo in enumerate(range(0, n, 64)):
        hi = min(lo + 64, n)
        out.append(lo + min(5, hi - lo - 1) if g % 2 == 0 else hi - 1)
    return out


def batch_of(kind: str, n: int) -> Tuple[HistoryBatch, List[int]]:
    """(canonical batch, the perturbed workflows): n chains, those of ``perturbed_lanes`` built by the kind."""
    c = KINDS[kind]
    lanes = perturbed_lanes(n)
    hs: List[WorkflowHistory] = [_history(c.build(w) if w in lanes else chain(w, 3), w) for w in range(n)]
    canon = flatten(hs, known_domains=KNOWN)
    assert (canon.wf["ev_count"] == EVENTS).all()
    if c.vh_cap is not None:
        canon.wf["vh_cap"][lanes] = c.vh_cap
    return canon, lanes


# ---- a history resumed from a loaded state -------------------------------------------------------------------
RESUME_CUT = 6         # batches in the prefix: 9 events, the second DecisionTaskCompleted opens the suffix
RESUME_KINDS = {"lower version": (S.VH_LOWER_VERSION, _lower), "id not increasing": (S.VH_EVENT_ID_NOT_INCREASING, _same_id),
                "negative version": (S.VH_INVALID_ITEM, _neg_version), "growth": (S.OK, None)}


def resume_histories(n: int) -> Tuple[List[WorkflowHistory], List[WorkflowHistory], Dict[int, str], int]:
    """(prefixes, suffixes, {workflow: kind}, events in a prefix): n chains cut after ``RESUME_CUT`` batches; in
    every wavefront four workflows have the first event of their suffix perturbed, which the prologue checks
    against the loaded history's last item."""
    plan: Dict[int, str] = {}
    for lo in range(0, n, 64):
        for i, kind in enumerate(RESUME_KINDS):
            if lo + 3 + 7 * i < n:
                plan[lo + 3 + 7 * i] = kind
    pre, suf, cut_events = [], [], 0
    for w in range(n):
        k = chain(w, 3)
        cut_events = sum(len(b) for b in k.batches[:RESUME_CUT])
        ev = _events(k)
        kind = plan.get(w)
        if kind == "growth":
            for e in ev[cut_events:]:
                e.version += 1
        elif kind is not None:
            RESUME_KINDS[kind][1](ev[cut_events], ev[cut_events - 1])
        h = _history(k, w)
        pre.append(dataclasses.replace(h, batches=h.batches[:RESUME_CUT], final_token=None, refresh_tasks=False))
        suf.append(dataclasses.replace(h, batches=h.batches[RESUME_CUT:]))
    return pre, suf, plan, cut_events


def statuses(batch: HistoryBatch, res) -> Tuple[np.ndarray, np.ndarray]:
    from cadence_amd.result import to_canonical_order
    ex = to_canonical_order(batch, res)
    return ex["status"].astype(np.int64), ex["fail_step"].astype(np.int64)
