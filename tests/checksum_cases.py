"""Shared cases for crr_checksum (the Load verify path) on states no replay of the same buffers wrote: loaded
rows uploaded from the host, a passive-replication state restored from its snapshot, and workflows whose step
ended in an error.  Used on the CPU (test_checksum_states: the references against each other, and the counts the
GPU tests rest on) and on the GPU (test_gpu_checksum_states: both paths of crr_checksum against the references).

Every expected value is ``oracle/checksum_py.payload_from_rows`` + ``crc32_ieee`` over rows the CPU holds; the
replay's own ``exec["checksum"]`` is only ever a second witness beside it.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from cadence_amd import abi, synth_mixed
from cadence_amd.flatten import LOADED_ID, flatten, interleave
from cadence_amd.replication import key_dict_from_events, last_batch_cut, split_descriptors, suffix_batch
from cadence_amd.result import ReplayResult, allocate_host
from oracle import checksum_py

from resume_cases import KNOWN, loaded_from, split_histories

LAYOUTS = {"interleaved": interleave, "canonical": lambda b: b, "lanes": lambda b: interleave(b, long_threshold=None)}


def expected_checksums(batch, res: ReplayResult) -> np.ndarray:
    """The independent encoder over every workflow's exec row and live rows (batch order), uint32 [n_wf]."""
    out = np.zeros(batch.n_wf, np.uint32)
    for w in range(batch.n_wf):
        token = checksum_py.token_of(batch, w, int(res.exec[w]["token_src"]))
        out[w] = checksum_py.crc32_ieee(checksum_py.payload_from_rows(res.exec[w], res.live_rows(batch, w), token))
    return out


def id_lists(batch, res: ReplayResult):
    """Per workflow (batch order) its five pending-ID lists in slot order, as one tuple of tuples."""
    out = []
    for w in range(batch.n_wf):
        live = res.live_rows(batch, w)
        out.append(tuple(tuple(int(x) for x in live[t][LOADED_ID[t]]) for t in abi.ID_TABLES))
    return out


def lists_differ(a, b) -> np.ndarray:
    return np.array([x != y for x, y in zip(a, b)], bool)


def slots_overwritten(before, after) -> np.ndarray:
    """Workflows for which a sidecar left by the state ``after`` misstates the state ``before``: a replay writes
    slots 0..n-1 of each column and leaves the rest, so what shows is a slot both states use holding another
    ID (a delete that is not the last entry moves the later IDs down; an insert or a delete at the end does not)."""
    return np.array([any(x[:min(len(x), len(y))] != y[:min(len(x), len(y))] for x, y in zip(b, a))
                     for b, a in zip(before, after)], bool)


def has_pending(lists) -> np.ndarray:
    return np.array([any(len(x) for x in ls) for ls in lists], bool)


def to_positions(batch, canon: np.ndarray) -> np.ndarray:
    """A per-workflow array in canonical order -> batch (device position) order."""
    return canon if batch.perm is None else canon[batch.perm]


@dataclasses.dataclass
class LoadedCase:
    pre_b: object                 # canonical prefix batch
    pre_r: ReplayResult           # the oracle's replay of it
    loaded: object                # LoadedStates (canonical order): the split workflows whose prefix replayed OK
    suf_canon: object             # the suffixes flattened onto ``loaded`` (canonical layout)

    def layout(self, name: str):
        return LAYOUTS[name](self.suf_canon)


@functools.lru_cache(maxsize=None)
def loaded_case(kind: str = "mixed") -> LoadedCase:
    """Histories split at a random batch (split seed 5), the prefixes replayed by the oracle and turned into
    loaded states.  ``mixed``: 600 histories with failing batches and new runs; ``long``: 40 long-tail ones, some
    of which land in the wave tail of the interleaved layout."""
    from oracle import oracle
    if kind == "mixed":
        hs = synth_mixed.mixed_histories(600, 61, multi_version=True, invalid_rate=0.1, can_rate=0.3)
    else:
        hs = synth_mixed.long_tail_histories(40, 62, max_len=4000, run_cap=2000, multi_version=True, caps=None)
    pre, suf, mask = split_histories(hs, 5)
    pre_b = flatten(pre, known_domains=KNOWN)
    pre_r = oracle.replay(pre_b, 2)
    loaded = loaded_from(pre_b, pre_r, mask)
    return LoadedCase(pre_b, pre_r, loaded, flatten(suf, known_domains=KNOWN, loaded=loaded))


@functools.lru_cache(maxsize=None)
def loaded_reference(kind: str, layout: str):
    """(suffix batch in ``layout``, its uploaded rows as the host holds them, expected checksum per position,
    loaded mask per position, the prefix replay's checksum per position)."""
    c = loaded_case(kind)
    b = c.layout(layout)
    rows = allocate_host(b)
    return (b, rows, expected_checksums(b, rows), to_positions(b, c.loaded.mask),
            to_positions(b, c.pre_r.exec["checksum"]))


# ---- PassiveReplication's split, on the CPU -------------------------------------------------------------------
PASSIVE_SEED = 17


@dataclasses.dataclass
class PassiveCase:
    batch: object                 # interleaved whole histories
    split: np.ndarray
    pre_b: object                 # the same layout with the prefix descriptors
    pre_r: ReplayResult           # the oracle's prefix replay
    suf_b: object                 # the new events with the suffix descriptors, ``pre_r``'s rows as loaded states
    suf_r: ReplayResult           # the oracle's replay of the step


# the events that insert into or delete from one of the five pending maps the checksum lists
_ET = abi.EventType
LIST_CHANGING = frozenset(int(t) for t in (
    _ET.ActivityTaskScheduled, _ET.ActivityTaskCompleted, _ET.ActivityTaskFailed, _ET.ActivityTaskTimedOut,
    _ET.ActivityTaskCanceled, _ET.TimerStarted, _ET.TimerFired, _ET.TimerCanceled,
    _ET.RequestCancelExternalWorkflowExecutionInitiated, _ET.RequestCancelExternalWorkflowExecutionFailed,
    _ET.ExternalWorkflowExecutionCancelRequested, _ET.StartChildWorkflowExecutionInitiated,
    _ET.StartChildWorkflowExecutionFailed, _ET.ChildWorkflowExecutionCompleted, _ET.ChildWorkflowExecutionFailed,
    _ET.ChildWorkflowExecutionCanceled, _ET.ChildWorkflowExecutionTimedOut, _ET.ChildWorkflowExecutionTerminated,
    _ET.SignalExternalWorkflowExecutionInitiated, _ET.SignalExternalWorkflowExecutionFailed,
    _ET.ExternalWorkflowExecutionSignaled))


def _trimmed(h):
    """``h`` without its trailing batches that touch no pending map (a history cut at a batch boundary is a
    history): its last batch is then one that changes an ID list."""
    b = list(h.batches)
    while len(b) > 2 and not any(int(e.event_type) in LIST_CHANGING for e in b[-1]):
        b.pop()
    return dataclasses.replace(h, batches=b)


def passive_histories(kind: str):
    """``as_generated``: mixed_histories(1500, 17, mean_len=40, invalid_rate=0.1, can_rate=0.3).  A generated
    history usually ends in a decision that closes the workflow, which touches no pending map: about 9 % of the
    last batches change an ID list, whatever the seed (17, 18, 19, 23: 130 to 141 of 1500).  ``trimmed``: the
    same generator without new runs, every even-numbered history cut back to its last batch that does."""
    if kind == "as_generated":
        return synth_mixed.mixed_histories(1500, PASSIVE_SEED, mean_len=40, invalid_rate=0.1, can_rate=0.3)
    hs = synth_mixed.mixed_histories(1500, PASSIVE_SEED, mean_len=40, invalid_rate=0.1)
    return [h if i % 2 else _trimmed(h) for i, h in enumerate(hs)]


@functools.lru_cache(maxsize=None)
def passive_batch(kind: str):
    return interleave(flatten(passive_histories(kind), known_domains=KNOWN))


@functools.lru_cache(maxsize=None)
def passive_case(kind: str) -> PassiveCase:
    """What replication.PassiveReplication does with this batch, replayed by the oracle: every workflow cut
    before its last event batch, the prefix replayed from scratch, the last batches applied onto its rows."""
    from oracle import oracle
    b = passive_batch(kind)
    cut = last_batch_cut(b)
    pre, suf, split = split_descriptors(b, cut)
    pre_b = dataclasses.replace(b, wf=pre)
    pre_r = oracle.replay(pre_b, 2)
    ok = pre_r.exec["status"] == 0
    mask_c = np.zeros(b.n_wf, bool)
    mask_c[b.perm if b.perm is not None else np.arange(b.n_wf)] = ok
    loaded = pre_r.to_loaded(pre_b, mask=mask_c)
    if b.perm is not None:
        loaded = loaded.permuted(b.perm)
    sb = suffix_batch(b, cut, split, suf)
    kd = sb.key_dict if sb.key_dict is not None else key_dict_from_events(b)
    suf_b = dataclasses.replace(sb, init=loaded, key_dict=kd)
    return PassiveCase(b, split, pre_b, pre_r, suf_b, oracle.replay(suf_b, 2))
