"""Real-shaped history blobs for the decoders' tests: every field of the reference's event schema, blobs
larger than the device ingest's LDS staging window, keys longer than the 16 bytes a KeyRef holds inline.

The synthetic encoders (thrift_codec, blob_encode.cpp) write the subset of each *EventAttributes struct the
replay reads plus a few skipped fields; a Cadence history service writes all of them.  This module holds
  (a) SCHEMA: the field ids, wire types and common/types JSON names of HistoryEvent, the 42 attribute
      structs and the structs nested in them (a table, from the ToWire methods of .gen/go/shared/shared.go;
      the line of each ToWire is cited per struct);
  (b) populate(): a blob with every schema field its attribute structs lack merged in (thrift_tree);
  (c) pad_blob() / many_events(): blobs of a chosen size;
  (d) window_path(): the staging loop of blob_decode_kernel restated, to classify a fixture's blobs;
  (e) window_batch(): one BlobSet that reaches every edge of that loop;
  (f) long_key_histories(): keys of 15..300 bytes, equal prefixes, str_hash collisions.
Test infrastructure only: the host decoder (history_decode.cpp) and flatten() stay the references."""
from __future__ import annotations

import base64
import copy
import dataclasses
import hashlib
import random
import struct
from typing import Dict, List, Optional

import numpy as np

from cadence_amd import synth_mixed
from cadence_amd.abi import EventType as ET
from cadence_amd.history import HistoryEvent, WorkflowHistory, det_uuid

from thrift_tree import (T_BOOL, T_DOUBLE, T_I32, T_I64, T_LIST, T_MAP, T_STRING, T_STRUCT, parse_blob, write_blob)

# ---- (a) the schema ----------------------------------------------------------------------------------------
# struct name -> (line of its ToWire in .gen/go/shared/shared.go, [(field id, type, JSON name), ...]).
# Types: bool double i32 i64 string binary, enum (an i32 on the wire, a name in JSON), struct:<Name>,
# list:string, list:struct:<Name>, map:string:binary.  JSON names: the tags of common/types/shared.go.
SCHEMA = {
    "HistoryEvent": (42000, [
        (10, "i64", "eventId"), (20, "i64", "timestamp"), (30, "enum", "eventType"), (35, "i64", "version"),
        (36, "i64", "taskId"),
        (40, "struct:WorkflowExecutionStartedEventAttributes", "workflowExecutionStartedEventAttributes"),
        (50, "struct:WorkflowExecutionCompletedEventAttributes", "workflowExecutionCompletedEventAttributes"),
        (60, "struct:WorkflowExecutionFailedEventAttributes", "workflowExecutionFailedEventAttributes"),
        (70, "struct:WorkflowExecutionTimedOutEventAttributes", "workflowExecutionTimedOutEventAttributes"),
        (80, "struct:DecisionTaskScheduledEventAttributes", "decisionTaskScheduledEventAttributes"),
        (90, "struct:DecisionTaskStartedEventAttributes", "decisionTaskStartedEventAttributes"),
        (100, "struct:DecisionTaskCompletedEventAttributes", "decisionTaskCompletedEventAttributes"),
        (110, "struct:DecisionTaskTimedOutEventAttributes", "decisionTaskTimedOutEventAttributes"),
        (120, "struct:DecisionTaskFailedEventAttributes", "decisionTaskFailedEventAttributes"),
        (130, "struct:ActivityTaskScheduledEventAttributes", "activityTaskScheduledEventAttributes"),
        (140, "struct:ActivityTaskStartedEventAttributes", "activityTaskStartedEventAttributes"),
        (150, "struct:ActivityTaskCompletedEventAttributes", "activityTaskCompletedEventAttributes"),
        (160, "struct:ActivityTaskFailedEventAttributes", "activityTaskFailedEventAttributes"),
        (170, "struct:ActivityTaskTimedOutEventAttributes", "activityTaskTimedOutEventAttributes"),
        (180, "struct:TimerStartedEventAttributes", "timerStartedEventAttributes"),
        (190, "struct:TimerFiredEventAttributes", "timerFiredEventAttributes"),
        (200, "struct:ActivityTaskCancelRequestedEventAttributes", "activityTaskCancelRequestedEventAttributes"),
        (210, "struct:RequestCancelActivityTaskFailedEventAttributes", "requestCancelActivityTaskFailedEventAttributes"),
        (220, "struct:ActivityTaskCanceledEventAttributes", "activityTaskCanceledEventAttributes"),
        (230, "struct:TimerCanceledEventAttributes", "timerCanceledEventAttributes"),
        (240, "struct:CancelTimerFailedEventAttributes", "cancelTimerFailedEventAttributes"),
        (250, "struct:MarkerRecordedEventAttributes", "markerRecordedEventAttributes"),
        (260, "struct:WorkflowExecutionSignaledEventAttributes", "workflowExecutionSignaledEventAttributes"),
        (270, "struct:WorkflowExecutionTerminatedEventAttributes", "workflowExecutionTerminatedEventAttributes"),
        (280, "struct:WorkflowExecutionCancelRequestedEventAttributes", "workflowExecutionCancelRequestedEventAttributes"),
        (290, "struct:WorkflowExecutionCanceledEventAttributes", "workflowExecutionCanceledEventAttributes"),
        (300, "struct:RequestCancelExternalWorkflowExecutionInitiatedEventAttributes",
         "requestCancelExternalWorkflowExecutionInitiatedEventAttributes"),
        (310, "struct:RequestCancelExternalWorkflowExecutionFailedEventAttributes",
         "requestCancelExternalWorkflowExecutionFailedEventAttributes"),
        (320, "struct:ExternalWorkflowExecutionCancelRequestedEventAttributes",
         "externalWorkflowExecutionCancelRequestedEventAttributes"),
        (330, "struct:WorkflowExecutionContinuedAsNewEventAttributes", "workflowExecutionContinuedAsNewEventAttributes"),
        (340, "struct:StartChildWorkflowExecutionInitiatedEventAttributes",
         "startChildWorkflowExecutionInitiatedEventAttributes"),
        (350, "struct:StartChildWorkflowExecutionFailedEventAttributes", "startChildWorkflowExecutionFailedEventAttributes"),
        (360, "struct:ChildWorkflowExecutionStartedEventAttributes", "childWorkflowExecutionStartedEventAttributes"),
        (370, "struct:ChildWorkflowExecutionCompletedEventAttributes", "childWorkflowExecutionCompletedEventAttributes"),
        (380, "struct:ChildWorkflowExecutionFailedEventAttributes", "childWorkflowExecutionFailedEventAttributes"),
        (390, "struct:ChildWorkflowExecutionCanceledEventAttributes", "childWorkflowExecutionCanceledEventAttributes"),
        (400, "struct:ChildWorkflowExecutionTimedOutEventAttributes", "childWorkflowExecutionTimedOutEventAttributes"),
        (410, "struct:ChildWorkflowExecutionTerminatedEventAttributes", "childWorkflowExecutionTerminatedEventAttributes"),
        (420, "struct:SignalExternalWorkflowExecutionInitiatedEventAttributes",
         "signalExternalWorkflowExecutionInitiatedEventAttributes"),
        (430, "struct:SignalExternalWorkflowExecutionFailedEventAttributes",
         "signalExternalWorkflowExecutionFailedEventAttributes"),
        (440, "struct:ExternalWorkflowExecutionSignaledEventAttributes", "externalWorkflowExecutionSignaledEventAttributes"),
        (450, "struct:UpsertWorkflowSearchAttributesEventAttributes", "upsertWorkflowSearchAttributesEventAttributes")]),
    # nested structs
    "WorkflowType": (101344, [(10, "string", "name")]),
    "ActivityType": (4379, [(10, "string", "name")]),
    "TaskList": (86014, [(10, "string", "name"), (20, "enum", "kind")]),
    "WorkflowExecution": (92843, [(10, "string", "workflowId"), (20, "string", "runId")]),
    "RetryPolicy": (74154, [
        (10, "i32", "initialIntervalInSeconds"), (20, "double", "backoffCoefficient"),
        (30, "i32", "maximumIntervalInSeconds"), (40, "i32", "maximumAttempts"),
        (50, "list:string", "nonRetriableErrorReasons"), (60, "i32", "expirationIntervalInSeconds")]),
    "Header": (40488, [(10, "map:string:binary", "fields")]),
    "Memo": (51418, [(10, "map:string:binary", "fields")]),
    "SearchAttributes": (76231, [(10, "map:string:binary", "indexedFields")]),
    "ResetPoints": (66496, [(10, "list:struct:ResetPointInfo", "points")]),
    "ResetPointInfo": (65942, [
        (10, "string", "binaryChecksum"), (20, "string", "runId"), (30, "i64", "firstDecisionCompletedId"),
        (40, "i64", "createdTimeNano"), (50, "i64", "expiringTimeNano"), (60, "bool", "resettable")]),
    # the attribute structs, by event type
    "WorkflowExecutionStartedEventAttributes": (98271, [
        (10, "struct:WorkflowType", "workflowType"), (12, "string", "parentWorkflowDomain"),
        (14, "struct:WorkflowExecution", "parentWorkflowExecution"), (16, "i64", "parentInitiatedEventId"),
        (20, "struct:TaskList", "taskList"), (30, "binary", "input"),
        (40, "i32", "executionStartToCloseTimeoutSeconds"), (50, "i32", "taskStartToCloseTimeoutSeconds"),
        (54, "string", "continuedExecutionRunId"), (55, "enum", "initiator"), (56, "string", "continuedFailureReason"),
        (57, "binary", "continuedFailureDetails"), (58, "binary", "lastCompletionResult"),
        (59, "string", "originalExecutionRunId"), (60, "string", "identity"), (61, "string", "firstExecutionRunId"),
        (70, "struct:RetryPolicy", "retryPolicy"), (80, "i32", "attempt"), (90, "i64", "expirationTimestamp"),
        (100, "string", "cronSchedule"), (110, "i32", "firstDecisionTaskBackoffSeconds"), (120, "struct:Memo", "memo"),
        (121, "struct:SearchAttributes", "searchAttributes"), (130, "struct:ResetPoints", "prevAutoResetPoints"),
        (140, "struct:Header", "header")]),
    "WorkflowExecutionCompletedEventAttributes": (94598, [
        (10, "binary", "result"), (20, "i64", "decisionTaskCompletedEventId")]),
    "WorkflowExecutionFailedEventAttributes": (96277, [
        (10, "string", "reason"), (20, "binary", "details"), (30, "i64", "decisionTaskCompletedEventId")]),
    "WorkflowExecutionTimedOutEventAttributes": (100283, [(10, "enum", "timeoutType")]),
    "DecisionTaskScheduledEventAttributes": (23920, [
        (10, "struct:TaskList", "taskList"), (20, "i32", "startToCloseTimeoutSeconds"), (30, "i64", "attempt")]),
    "DecisionTaskStartedEventAttributes": (24254, [
        (10, "i64", "scheduledEventId"), (20, "string", "identity"), (30, "string", "requestId")]),
    "DecisionTaskCompletedEventAttributes": (22184, [
        (10, "binary", "executionContext"), (20, "i64", "scheduledEventId"), (30, "i64", "startedEventId"),
        (40, "string", "identity"), (50, "string", "binaryChecksum")]),
    "DecisionTaskTimedOutEventAttributes": (24796, [
        (10, "i64", "scheduledEventId"), (20, "i64", "startedEventId"), (30, "enum", "timeoutType"),
        (40, "string", "baseRunId"), (50, "string", "newRunId"), (60, "i64", "forkEventVersion"),
        (70, "string", "reason"), (80, "enum", "cause")]),
    "DecisionTaskFailedEventAttributes": (23123, [
        (10, "i64", "scheduledEventId"), (20, "i64", "startedEventId"), (30, "enum", "cause"), (35, "binary", "details"),
        (40, "string", "identity"), (50, "string", "reason"), (60, "string", "baseRunId"), (70, "string", "newRunId"),
        (80, "i64", "forkEventVersion"), (90, "string", "binaryChecksum")]),
    "ActivityTaskScheduledEventAttributes": (2368, [
        (10, "string", "activityId"), (20, "struct:ActivityType", "activityType"), (25, "string", "domain"),
        (30, "struct:TaskList", "taskList"), (40, "binary", "input"), (45, "i32", "scheduleToCloseTimeoutSeconds"),
        (50, "i32", "scheduleToStartTimeoutSeconds"), (55, "i32", "startToCloseTimeoutSeconds"),
        (60, "i32", "heartbeatTimeoutSeconds"), (90, "i64", "decisionTaskCompletedEventId"),
        (110, "struct:RetryPolicy", "retryPolicy"), (120, "struct:Header", "header")]),
    "ActivityTaskStartedEventAttributes": (3314, [
        (10, "i64", "scheduledEventId"), (20, "string", "identity"), (30, "string", "requestId"), (40, "i32", "attempt"),
        (50, "string", "lastFailureReason"), (60, "binary", "lastFailureDetails")]),
    "ActivityTaskCompletedEventAttributes": (1500, [
        (10, "binary", "result"), (20, "i64", "scheduledEventId"), (30, "i64", "startedEventId"),
        (40, "string", "identity")]),
    "ActivityTaskFailedEventAttributes": (1899, [
        (10, "string", "reason"), (20, "binary", "details"), (30, "i64", "scheduledEventId"),
        (40, "i64", "startedEventId"), (50, "string", "identity")]),
    "ActivityTaskTimedOutEventAttributes": (3840, [
        (5, "binary", "details"), (10, "i64", "scheduledEventId"), (20, "i64", "startedEventId"),
        (30, "enum", "timeoutType"), (40, "string", "lastFailureReason"), (50, "binary", "lastFailureDetails")]),
    "TimerStartedEventAttributes": (89026, [
        (10, "string", "timerId"), (20, "i64", "startToFireTimeoutSeconds"), (30, "i64", "decisionTaskCompletedEventId")]),
    "TimerFiredEventAttributes": (88751, [(10, "string", "timerId"), (20, "i64", "startedEventId")]),
    "ActivityTaskCancelRequestedEventAttributes": (762, [
        (10, "string", "activityId"), (20, "i64", "decisionTaskCompletedEventId")]),
    "RequestCancelActivityTaskFailedEventAttributes": (63739, [
        (10, "string", "activityId"), (20, "string", "cause"), (30, "i64", "decisionTaskCompletedEventId")]),
    "ActivityTaskCanceledEventAttributes": (1039, [
        (10, "binary", "details"), (20, "i64", "latestCancelRequestedEventId"), (30, "i64", "scheduledEventId"),
        (40, "i64", "startedEventId"), (50, "string", "identity")]),
    "TimerCanceledEventAttributes": (88351, [
        (10, "string", "timerId"), (20, "i64", "startedEventId"), (30, "i64", "decisionTaskCompletedEventId"),
        (40, "string", "identity")]),
    "CancelTimerFailedEventAttributes": (7407, [
        (10, "string", "timerId"), (20, "string", "cause"), (30, "i64", "decisionTaskCompletedEventId"),
        (40, "string", "identity")]),
    "MarkerRecordedEventAttributes": (51027, [
        (10, "string", "markerName"), (20, "binary", "details"), (30, "i64", "decisionTaskCompletedEventId"),
        (40, "struct:Header", "header")]),
    "WorkflowExecutionSignaledEventAttributes": (97915, [
        (10, "string", "signalName"), (20, "binary", "input"), (30, "string", "identity")]),
    "WorkflowExecutionTerminatedEventAttributes": (99951, [
        (10, "string", "reason"), (20, "binary", "details"), (30, "string", "identity")]),
    "WorkflowExecutionCancelRequestedEventAttributes": (93681, [
        (10, "string", "cause"), (20, "i64", "externalInitiatedEventId"),
        (30, "struct:WorkflowExecution", "externalWorkflowExecution"), (40, "string", "identity")]),
    "WorkflowExecutionCanceledEventAttributes": (94077, [
        (10, "i64", "decisionTaskCompletedEventId"), (20, "binary", "details")]),
    "RequestCancelExternalWorkflowExecutionInitiatedEventAttributes": (65085, [
        (10, "i64", "decisionTaskCompletedEventId"), (20, "string", "domain"),
        (30, "struct:WorkflowExecution", "workflowExecution"), (40, "binary", "control"),
        (50, "bool", "childWorkflowOnly")]),
    "RequestCancelExternalWorkflowExecutionFailedEventAttributes": (64542, [
        (10, "enum", "cause"), (20, "i64", "decisionTaskCompletedEventId"), (30, "string", "domain"),
        (40, "struct:WorkflowExecution", "workflowExecution"), (50, "i64", "initiatedEventId"),
        (60, "binary", "control")]),
    "ExternalWorkflowExecutionCancelRequestedEventAttributes": (35153, [
        (10, "i64", "initiatedEventId"), (20, "string", "domain"), (30, "struct:WorkflowExecution", "workflowExecution")]),
    "WorkflowExecutionContinuedAsNewEventAttributes": (95215, [
        (10, "string", "newExecutionRunId"), (20, "struct:WorkflowType", "workflowType"),
        (30, "struct:TaskList", "taskList"), (40, "binary", "input"),
        (50, "i32", "executionStartToCloseTimeoutSeconds"), (60, "i32", "taskStartToCloseTimeoutSeconds"),
        (70, "i64", "decisionTaskCompletedEventId"), (80, "i32", "backoffStartIntervalInSeconds"),
        (90, "enum", "initiator"), (100, "string", "failureReason"), (110, "binary", "failureDetails"),
        (120, "binary", "lastCompletionResult"), (130, "struct:Header", "header"), (140, "struct:Memo", "memo"),
        (150, "struct:SearchAttributes", "searchAttributes")]),
    "StartChildWorkflowExecutionInitiatedEventAttributes": (82109, [
        (10, "string", "domain"), (20, "string", "workflowId"), (30, "struct:WorkflowType", "workflowType"),
        (40, "struct:TaskList", "taskList"), (50, "binary", "input"),
        (60, "i32", "executionStartToCloseTimeoutSeconds"), (70, "i32", "taskStartToCloseTimeoutSeconds"),
        (81, "enum", "parentClosePolicy"), (90, "binary", "control"), (100, "i64", "decisionTaskCompletedEventId"),
        (110, "enum", "workflowIdReusePolicy"), (120, "struct:RetryPolicy", "retryPolicy"),
        (130, "string", "cronSchedule"), (140, "struct:Header", "header"), (150, "struct:Memo", "memo"),
        (160, "struct:SearchAttributes", "searchAttributes"), (170, "i32", "delayStartSeconds")]),
    "StartChildWorkflowExecutionFailedEventAttributes": (81491, [
        (10, "string", "domain"), (20, "string", "workflowId"), (30, "struct:WorkflowType", "workflowType"),
        (40, "enum", "cause"), (50, "binary", "control"), (60, "i64", "initiatedEventId"),
        (70, "i64", "decisionTaskCompletedEventId")]),
    "ChildWorkflowExecutionStartedEventAttributes": (10058, [
        (10, "string", "domain"), (20, "i64", "initiatedEventId"), (30, "struct:WorkflowExecution", "workflowExecution"),
        (40, "struct:WorkflowType", "workflowType"), (50, "struct:Header", "header")]),
    "ChildWorkflowExecutionCompletedEventAttributes": (8773, [
        (10, "binary", "result"), (20, "string", "domain"), (30, "struct:WorkflowExecution", "workflowExecution"),
        (40, "struct:WorkflowType", "workflowType"), (50, "i64", "initiatedEventId"), (60, "i64", "startedEventId")]),
    "ChildWorkflowExecutionFailedEventAttributes": (9478, [
        (10, "string", "reason"), (20, "binary", "details"), (30, "string", "domain"),
        (40, "struct:WorkflowExecution", "workflowExecution"), (50, "struct:WorkflowType", "workflowType"),
        (60, "i64", "initiatedEventId"), (70, "i64", "startedEventId")]),
    "ChildWorkflowExecutionCanceledEventAttributes": (8231, [
        (10, "binary", "details"), (20, "string", "domain"), (30, "struct:WorkflowExecution", "workflowExecution"),
        (40, "struct:WorkflowType", "workflowType"), (50, "i64", "initiatedEventId"), (60, "i64", "startedEventId")]),
    "ChildWorkflowExecutionTimedOutEventAttributes": (10971, [
        (10, "enum", "timeoutType"), (20, "string", "domain"), (30, "struct:WorkflowExecution", "workflowExecution"),
        (40, "struct:WorkflowType", "workflowType"), (50, "i64", "initiatedEventId"), (60, "i64", "startedEventId")]),
    "ChildWorkflowExecutionTerminatedEventAttributes": (10512, [
        (10, "string", "domain"), (20, "struct:WorkflowExecution", "workflowExecution"),
        (30, "struct:WorkflowType", "workflowType"), (40, "i64", "initiatedEventId"), (50, "i64", "startedEventId")]),
    "SignalExternalWorkflowExecutionInitiatedEventAttributes": (77905, [
        (10, "i64", "decisionTaskCompletedEventId"), (20, "string", "domain"),
        (30, "struct:WorkflowExecution", "workflowExecution"), (40, "string", "signalName"), (50, "binary", "input"),
        (60, "binary", "control"), (70, "bool", "childWorkflowOnly")]),
    "SignalExternalWorkflowExecutionFailedEventAttributes": (77360, [
        (10, "enum", "cause"), (20, "i64", "decisionTaskCompletedEventId"), (30, "string", "domain"),
        (40, "struct:WorkflowExecution", "workflowExecution"), (50, "i64", "initiatedEventId"),
        (60, "binary", "control")]),
    "ExternalWorkflowExecutionSignaledEventAttributes": (35488, [
        (10, "i64", "initiatedEventId"), (20, "string", "domain"), (30, "struct:WorkflowExecution", "workflowExecution"),
        (40, "binary", "control")]),
    "UpsertWorkflowSearchAttributesEventAttributes": (91217, [
        (10, "i64", "decisionTaskCompletedEventId"), (20, "struct:SearchAttributes", "searchAttributes")]),
}

WIRE = {"bool": T_BOOL, "double": T_DOUBLE, "i32": T_I32, "enum": T_I32, "i64": T_I64, "string": T_STRING,
        "binary": T_STRING, "struct": T_STRUCT, "map": T_MAP, "list": T_LIST}


def wire_type(ty: str) -> int:
    return WIRE[ty.split(":")[0]]


def attr_struct_name(event_type: int) -> Optional[str]:
    """The attribute struct of an event type, None for an unknown type."""
    if event_type not in ET._value2member_map_:
        return None
    return ET(event_type).name + "EventAttributes"


# event type -> its attribute field in HistoryEvent (ids 180..320 are not in EventType order)
ATTR_FIELD = {int(ET[ty.split(":")[1][:-len("EventAttributes")]]): fid
              for fid, ty, _n in SCHEMA["HistoryEvent"][1] if fid >= 40}


# The fields the decoders read (history_decode.cpp read_attributes / read_retry_policy / read_reset_points; the
# device ingest and the JSON decoder read the same ones): populate() never adds one of these with its own
# type to a struct that lacks it -- that would change the history's meaning.
DECODER_READS = {
    "WorkflowExecutionStartedEventAttributes": {12, 40, 50, 55, 80, 90, 110, 130},
    "DecisionTaskScheduledEventAttributes": {20, 30},
    "DecisionTaskStartedEventAttributes": {10},
    "DecisionTaskCompletedEventAttributes": {30, 50},
    "DecisionTaskTimedOutEventAttributes": {30},
    "ActivityTaskScheduledEventAttributes": {10, 25, 45, 50, 55, 60, 110},
    "ActivityTaskStartedEventAttributes": {10},
    "ActivityTaskTimedOutEventAttributes": {10},
    "ActivityTaskCompletedEventAttributes": {20},
    "ActivityTaskFailedEventAttributes": {30},
    "ActivityTaskCanceledEventAttributes": {30},
    "ActivityTaskCancelRequestedEventAttributes": {10},
    "TimerFiredEventAttributes": {10},
    "TimerCanceledEventAttributes": {10},
    "TimerStartedEventAttributes": {10, 20},
    "StartChildWorkflowExecutionInitiatedEventAttributes": {10},
    "RequestCancelExternalWorkflowExecutionInitiatedEventAttributes": {20},
    "SignalExternalWorkflowExecutionInitiatedEventAttributes": {20},
    "StartChildWorkflowExecutionFailedEventAttributes": {60},
    "ChildWorkflowExecutionFailedEventAttributes": {60},
    "ChildWorkflowExecutionStartedEventAttributes": {20},
    "ChildWorkflowExecutionCompletedEventAttributes": {50},
    "ChildWorkflowExecutionCanceledEventAttributes": {50},
    "ChildWorkflowExecutionTimedOutEventAttributes": {50},
    "RequestCancelExternalWorkflowExecutionFailedEventAttributes": {50},
    "SignalExternalWorkflowExecutionFailedEventAttributes": {50},
    "ChildWorkflowExecutionTerminatedEventAttributes": {40},
    "ExternalWorkflowExecutionCancelRequestedEventAttributes": {10},
    "ExternalWorkflowExecutionSignaledEventAttributes": {10},
    # nested structs the decoders read into
    "RetryPolicy": {60},
    "ResetPoints": {10},
    "ResetPointInfo": {10},
}

MODES = ("full", "empty", "wrong_type", "general")
KNOWN_DOMAIN_DECOY = b"domain-a"      # a name of blobs.KNOWN_DOMAINS, written into fields that are not domains
DECOY_ID = 900                        # an event-level field id no schema struct has (thrift_tree's range)


# ---- (b) populate ------------------------------------------------------------------------------------------
class _Decoys:
    """Decoy values of the schema's types; strings are numbered so that every one is distinct."""

    def __init__(self, rng: random.Random, zero: bool):
        self.rng, self.zero, self.n = rng, zero, 0

    def string(self, name: str) -> bytes:
        if self.zero:
            return b""
        self.n += 1
        if self.rng.random() < 0.2:
            return KNOWN_DOMAIN_DECOY
        return f"{name}-{self.n}".encode()

    def value(self, ty: str, fid: int, name: str):
        """(wire type, thrift_tree value) of a field of type `ty`."""
        rng, zero = self.rng, self.zero
        parts = ty.split(":")
        k = parts[0]
        if k == "i64":
            return T_I64, struct.pack(">q", 0 if zero else 0x5A5A5A5A5A5A5A5A + fid)
        if k in ("i32", "enum"):
            return T_I32, struct.pack(">i", 0 if zero else 0x5A5A00 + fid)
        if k == "bool":
            return T_BOOL, b"\0" if zero else b"\1"
        if k == "double":
            return T_DOUBLE, struct.pack(">d", 0.0 if zero else 2.5)
        if k == "string":
            return T_STRING, self.string(name)
        if k == "binary":
            return T_STRING, b"" if zero else bytes(rng.randrange(256) for _ in range(rng.randrange(41)))
        if k == "struct":
            if zero:
                return T_STRUCT, []
            out = []
            for i, t, n in SCHEMA[parts[1]][1]:
                wt, v = self.value(t, i, n)
                out.append([wt, i, v])
            return T_STRUCT, out
        if k == "list":
            n = 0 if zero else rng.randrange(4)
            if parts[1] == "struct":
                return T_LIST, (T_STRUCT, [self.value("struct:" + parts[2], 0, name)[1] for _ in range(n)])
            return T_LIST, (T_STRING, [self.string(name) for _ in range(n)])
        if k == "map":
            n = 0 if zero else rng.randrange(4)
            return T_MAP, (T_STRING, T_STRING, [(self.string(name + "-key"), self.value("binary", 0, name)[1])
                                                for _ in range(n)])
        raise ValueError(ty)


def _wrong_value(ty: str):
    """A value of another wire type than `ty`'s (thriftrw skips a field whose type is not the schema's)."""
    if wire_type(ty) == T_I64:
        return T_I32, struct.pack(">i", 0x7E57)
    if wire_type(ty) == T_STRING:
        return T_I64, struct.pack(">q", 0x7E577E57)
    if wire_type(ty) == T_I32:
        return T_I64, struct.pack(">q", 0x7E57)
    return T_STRING, b"not-a-" + ty.encode()      # struct / list / map


def _merge(fields, sname: str, mode: str, d: _Decoys):
    """`fields` ([type, id, value] triples of one struct `sname`) with the schema fields it lacks, ascending."""
    reads = DECODER_READS.get(sname, set())
    have = {f[1]: f for f in fields}
    out = []
    for fid, ty, name in SCHEMA[sname][1]:
        f = have.pop(fid, None)
        if f is not None:
            f = list(f)
            parts = ty.split(":")
            if f[0] == wire_type(ty):   # a present nested struct (or list of structs) is merged as well
                if parts[0] == "struct":
                    f[2] = _merge(f[2], parts[1], mode, d)
                elif parts[0] == "list" and parts[1] == "struct" and f[2][0] == T_STRUCT:
                    f[2] = (T_STRUCT, [_merge(x, parts[2], mode, d) for x in f[2][1]])
            out.append(f)
        elif fid in reads:
            if mode == "wrong_type":
                t, v = _wrong_value(ty)
                out.append([t, fid, v])
        elif mode != "wrong_type":
            t, v = d.value(ty, fid, name)
            out.append([t, fid, v])
    out += [list(f) for f in have.values()]        # fields outside the schema stay
    out.sort(key=lambda f: f[1])
    return out


def _events_of(hist):
    for f in hist:
        if f[1] == 10 and f[0] == T_LIST:
            return f
    return None


def _event_type(ev) -> Optional[int]:
    for ft, fid, v in ev:
        if fid == 30 and ft == T_I32:
            return struct.unpack(">i", v)[0]
    return None


def populate(blob: bytes, mode: str, rng: random.Random) -> bytes:
    """`blob` with each event's attribute struct merged with the schema fields it lacks, ids ascending
    (thriftrw's order: the blob stays on the device's fast pass).  `full`: every absent field with its real
    type and a decoy value; `empty`: present but zero (empty strings, maps, lists, structs), and an empty
    list<struct> on the first event; `wrong_type`: only the decoder-read fields the struct lacks, each with
    another wire type (thriftrw skips such a field); `general`: `full` plus a list<struct> decoy on the first
    event (the fast pass must defer the blob).  A decoder-read field the struct lacks is never added with
    its own type."""
    assert mode in MODES
    if not blob:
        return blob
    hist = parse_blob(blob)
    lf = _events_of(hist)
    if lf is None:
        return blob
    d = _Decoys(rng, zero=mode == "empty")
    evs = []
    for k, ev in enumerate(lf[2][1]):
        ev = [list(f) for f in ev]
        sname = attr_struct_name(_event_type(ev))
        if sname is not None:
            fid_attr = ATTR_FIELD[_event_type(ev)]
            for f in ev:
                if f[1] == fid_attr and f[0] == T_STRUCT:
                    f[2] = _merge(f[2], sname, "full" if mode == "general" else mode, d)
        if k == 0 and mode == "general":
            ev.append([T_LIST, DECOY_ID, (T_STRUCT, [[[T_STRING, 1, b"decoy"], [T_I32, 2, b"\0\0\0\1"]]] * 2)])
        elif k == 0 and mode == "empty":   # an empty list whose element type is struct
            ev.append([T_LIST, DECOY_ID, (T_STRUCT, [])])
        evs.append(ev)
    lf[2] = (lf[2][0], evs)
    return write_blob(hist)


def _field_ids(fields):
    return [f[1] for f in fields]


def _check_struct(new, old, sname: str, mode: str):
    reads = DECODER_READS.get(sname, set())
    schema = {fid: ty for fid, ty, _n in SCHEMA[sname][1]}
    old_by = {f[1]: f for f in old}
    ids = _field_ids(new)
    assert ids == sorted(ids), (sname, ids)
    lacking_reads = {fid for fid in reads if fid not in old_by}
    if mode == "wrong_type":
        assert set(ids) == set(old_by) | lacking_reads, (sname, ids)
    else:
        assert set(ids) == (set(schema) - lacking_reads) | set(old_by), (sname, ids)
    for f in new:
        fid = f[1]
        if fid in old_by:
            assert f[0] == old_by[fid][0]
            ty = schema.get(fid, "")
            parts = ty.split(":")
            if parts[0] == "struct" and f[0] == T_STRUCT:
                _check_struct(f[2], old_by[fid][2], parts[1], mode)
            elif parts[:2] == ["list", "struct"] and f[0] == T_LIST and f[2][0] == T_STRUCT:
                assert len(f[2][1]) == len(old_by[fid][2][1])
                for x, y in zip(f[2][1], old_by[fid][2][1]):
                    _check_struct(x, y, parts[2], mode)
            else:
                assert f[2] == old_by[fid][2], (sname, fid)
        elif fid in lacking_reads:
            assert f[0] != wire_type(schema[fid]), (sname, fid)     # only ever with another type
        else:
            assert f[0] == wire_type(schema[fid]), (sname, fid)


def check_populated(old_blob: bytes, new_blob: bytes, mode: str) -> int:
    """Re-parse a populated blob: every attribute struct holds exactly the schema's field set -- less the
    decoder-read fields the original lacked (`wrong_type`: those alone, never with their own type) -- and the
    original's fields unchanged.  Returns the number of attribute structs checked."""
    if not old_blob:
        assert new_blob == old_blob
        return 0
    n = 0
    old_evs, new_evs = _events_of(parse_blob(old_blob))[2][1], _events_of(parse_blob(new_blob))[2][1]
    assert len(old_evs) == len(new_evs)
    for k, (o, w) in enumerate(zip(old_evs, new_evs)):
        extra = [f for f in w if f[1] == DECOY_ID]
        assert len(extra) == (1 if k == 0 and mode in ("general", "empty") else 0)
        if extra and mode == "general":
            assert extra[0][0] == T_LIST and extra[0][2][0] == T_STRUCT and extra[0][2][1]
        w = [f for f in w if f[1] != DECOY_ID]
        assert _field_ids(w) == _field_ids(o)
        sname = attr_struct_name(_event_type(o))
        for fo, fw in zip(o, w):
            if sname is not None and fo[1] == ATTR_FIELD[_event_type(o)] and fo[0] == T_STRUCT:
                _check_struct(fw[2], fo[2], sname, "full" if mode == "general" else mode)
                n += 1
            else:
                assert fo == fw
    return n


def populate_sources(sources, mode: str, seed: int = 1):
    """Host-decoder inputs (decode.WorkflowSource) with every thriftrw blob populated."""
    rng = random.Random(seed)
    out = []
    for s in sources:
        out.append(dataclasses.replace(s, blobs=[populate(b, mode, rng) for b in s.blobs]))
    return out


# -- JSON: the same with the schema's common/types names -------------------------------------------------------
def _json_decoy(ty: str, fid: int, name: str, rng: random.Random, n: List[int]):
    parts = ty.split(":")
    k = parts[0]
    if k == "i64":
        return 0x5A5A5A5A5A5A5A5A + fid
    if k == "i32":
        return 0x5A5A00 + fid
    if k == "enum":
        return str(fid % 3)             # UnmarshalText's decimal fallback
    if k == "bool":
        return True
    if k == "double":
        return 2.5
    if k == "string":
        n[0] += 1
        return "domain-a" if rng.random() < 0.2 else f"{name}-{n[0]}"
    if k == "binary":
        return base64.b64encode(bytes(rng.randrange(256) for _ in range(rng.randrange(41)))).decode()
    if k == "struct":
        return {nm: _json_decoy(t, i, nm, rng, n) for i, t, nm in SCHEMA[parts[1]][1]}
    if k == "list":
        if parts[1] == "struct":
            return [_json_decoy("struct:" + parts[2], 0, name, rng, n) for _ in range(rng.randrange(3))]
        return [_json_decoy("string", 0, name, rng, n) for _ in range(rng.randrange(4))]
    if k == "map":
        return {f"{name}-key-{j}": _json_decoy("binary", 0, name, rng, n) for j in range(rng.randrange(4))}
    raise ValueError(ty)


def _merge_json(obj: Dict, sname: str, mode: str, rng: random.Random, n: List[int]) -> Dict:
    reads = DECODER_READS.get(sname, set())
    out = dict(obj)
    for fid, ty, name in SCHEMA[sname][1]:
        parts = ty.split(":")
        if name in out:
            v = out[name]
            if parts[0] == "struct" and isinstance(v, dict):
                out[name] = _merge_json(v, parts[1], mode, rng, n)
            elif parts[:2] == ["list", "struct"] and isinstance(v, list):
                out[name] = [_merge_json(x, parts[2], mode, rng, n) if isinstance(x, dict) else x for x in v]
        elif fid in reads:
            out[name] = None                 # null leaves the field unset (encoding/json)
        elif mode == "empty":
            out[name] = {} if parts[0] in ("struct", "map") and rng.random() < 0.5 else None
        else:
            out[name] = _json_decoy(ty, fid, name, rng, n)
    return out


def populate_json_event(d: Dict, mode: str, rng: random.Random) -> Dict:
    """A json_codec.event_json object with every key of its attribute struct present: `full` typed decoys
    (a decoder-read key the event lacks: null), `empty` null / {}."""
    assert mode in ("full", "empty")
    out = dict(d)
    for fid, ty, name in SCHEMA["HistoryEvent"][1]:
        if fid >= 40 and isinstance(out.get(name), dict):
            out[name] = _merge_json(out[name], ty.split(":")[1], mode, rng, [0])
    return out


# ---- (c) blobs of a chosen size ---------------------------------------------------------------------------------
# (attribute field of HistoryEvent, its skipped binary field): the inputs of WorkflowExecutionStarted and
# ActivityTaskScheduled
_PAD_FIELDS = ((40, 30), (130, 40))


def can_pad(blob: bytes) -> bool:
    if not blob:
        return False
    for ev in _events_of(parse_blob(blob))[2][1]:
        for f in ev:
            if f[0] == T_STRUCT and any(f[1] == a and any(g[1] == i and g[0] == T_STRING for g in f[2])
                                        for a, i in _PAD_FIELDS):
                return True
    return False


def pad_blob(blob: bytes, length: int) -> bytes:
    """`blob` grown to exactly `length` bytes through a skipped binary field: `input` (id 30) of its first
    WorkflowExecutionStarted event, else id 40 of its first ActivityTaskScheduled event."""
    grow = length - len(blob)
    assert grow >= 0, (length, len(blob))
    hist = parse_blob(blob)
    for ev in _events_of(hist)[2][1]:
        for f in ev:
            for a, i in _PAD_FIELDS:
                if f[0] == T_STRUCT and f[1] == a:
                    for g in f[2]:
                        if g[1] == i and g[0] == T_STRING:
                            g[2] = bytes(g[2]) + bytes((7 * j + 1) & 0xFF for j in range(grow))
                            out = write_blob(hist)
                            assert len(out) == length
                            return out
    raise ValueError("no started / activity-scheduled event to pad")


def pad_event(blob: bytes, k: int, length: int) -> bytes:
    """`blob` grown to exactly `length` bytes through the first string field of event k's attribute struct that
    the decoders skip (a populated blob has one for every event type but a few): for blobs without a
    WorkflowExecutionStarted or ActivityTaskScheduled event."""
    grow = length - len(blob)
    assert grow >= 0, (length, len(blob))
    hist = parse_blob(blob)
    ev = _events_of(hist)[2][1][k]
    sname = attr_struct_name(_event_type(ev))
    for f in ev:
        if f[0] == T_STRUCT and f[1] == ATTR_FIELD[_event_type(ev)]:
            for g in f[2]:
                if g[0] == T_STRING and g[1] not in DECODER_READS.get(sname, set()):
                    g[2] = bytes(g[2]) + b"\x5a" * grow
                    out = write_blob(hist)
                    assert len(out) == length
                    return out
    raise ValueError("no skipped string field in event %d" % k)


def populated_task_blobs(bs, beyond: int = 13 * 1024, seed: int = 4):
    """A BlobSet of replication tasks' event blobs (exec_blob_cases.task_blob_set) as a history service
    persists them: every blob populated `full`, and each workflow's first blob padded through its first event
    so that every later event of the task lies more than `beyond` bytes into the task's bytes."""
    from cadence_amd.blobs import blobset_from_sources
    from cadence_amd.decode import WorkflowSource
    rng = random.Random(seed)
    src = []
    for r in bs.wf:
        b0, n = int(r["blob_begin"]), int(r["blob_count"])
        blobs = [populate(bs.blob(b0 + i), "full", rng) for i in range(n)]
        if blobs and blobs[0]:
            for k in range(len(_events_of(parse_blob(blobs[0]))[2][1])):   # (an Upsert event has no string field)
                try:
                    blobs[0] = pad_event(blobs[0], k, max(len(blobs[0]), beyond + 512))
                    break
                except ValueError:
                    continue
        src.append(WorkflowSource(blobs=blobs))
    return blobset_from_sources(src)[0]


def many_events(length: int, seed: int = 3, first_id: int = 3, version: int = 1):
    """A batch that reaches `length` bytes with hundreds of small events instead of padding: (events, its
    `full`-populated blob), the blob at least `length` bytes."""
    from cadence_amd.thrift_codec import serialize_batch_events
    rng = random.Random(seed)
    evs, trees, size = [], [], 1 + 3 + 5 + 1      # preamble, list field header, list header, stop
    ts, k = synth_mixed.BASE_TS, 0
    while size < length:
        eid = first_id + len(evs)
        ts += 1_000_000
        kind = k % 8
        if kind == 6:
            e = HistoryEvent(int(ET.TimerStarted), eid, version, ts, 5000 + eid,
                             {"timer_id": f"many-{k}", "start_to_fire_timeout_seconds": 30})
        elif kind == 7:
            e = HistoryEvent(int(ET.TimerFired), eid, version, ts, 5000 + eid, {"timer_id": f"many-{k - 1}"})
        elif kind % 2:
            e = HistoryEvent(int(ET.WorkflowExecutionSignaled), eid, version, ts, 5000 + eid, {})
        else:
            e = HistoryEvent(int(ET.MarkerRecorded), eid, version, ts, 5000 + eid, {})
        k += 1
        one = populate(serialize_batch_events([e]), "full", rng)
        tree = _events_of(parse_blob(one))[2][1][0]
        size += len(one) - (1 + 3 + 5 + 1)
        evs.append(e)
        trees.append(tree)
    blob = write_blob([[T_LIST, 10, (T_STRUCT, trees)]])
    assert len(blob) == size
    return evs, blob


# ---- (d) the staging loop of blob_decode_kernel, restated -------------------------------------------------------
# ingest_kernel.hip: CRR_INGEST_STAGE_KB = 13, kStageBytes = 13 * 1024 (the LDS window a wavefront stages its
# 64 blobs through).  Pinned here: a fixture built for another window size would prove nothing.
K_STAGE_BYTES = 13 * 1024


@dataclasses.dataclass
class BlobPath:
    kind: str          # "staged" | "hbm" | "empty"
    wave: int          # the wavefront (blob index // 64)
    lane: int
    window: int        # the loop iteration of its wavefront that served it (staged: "staged in window k")
    slack: int         # staged: lim - (((b1 - 1) & ~15) + 32), 0 = it fits with nothing to spare; hbm: < 0

    def __str__(self):
        return {"staged": f"staged in window {self.window}", "hbm": "walked from HBM", "empty": "empty"}[self.kind]


def window_path(blob_off):
    """ingest_kernel.hip blob_decode_kernel's loop (`for (;;) { pending = ballot(!done) ... }`) over the blob
    offsets: per blob, staged in window k / walked from HBM / empty; and per wavefront, how many times the
    loop ran (each run stages the window again).  Classifies a fixture; no output's reference."""
    off = [int(x) for x in blob_off]
    n = len(off) - 1
    out: List[Optional[BlobPath]] = [None] * n
    iterations = []
    for w0 in range(0, n, 64):
        last = min(w0 + 64, n)
        stage_cap = (off[last] + 31) & ~15
        it = 0
        while True:
            pend = [i for i in range(w0, last) if out[i] is None]
            if not pend:
                break
            f = pend[0]
            s = off[f] & ~15
            lim = min(s + K_STAGE_BYTES, stage_cap)
            for i in pend:
                b0, b1 = off[i], off[i + 1]
                need = ((b1 - 1) & ~15) + 32
                if b1 == b0:
                    out[i] = BlobPath("empty", w0 // 64, i - w0, it, 0)
                elif b0 >= s and need <= lim:
                    out[i] = BlobPath("staged", w0 // 64, i - w0, it, lim - need)
                elif i == f:
                    out[i] = BlobPath("hbm", w0 // 64, i - w0, it, lim - need)
            it += 1
        iterations.append(it)
    return out, iterations


# ---- shared: histories -> host-decoder inputs --------------------------------------------------------------------
def sources_of(hs):
    from test_decode import sources_of as so
    return so(hs)


def blobset_of(sources):
    from cadence_amd.blobs import blobset_from_sources
    return blobset_from_sources(sources)[0]


# ---- (e) the staging-window fixture ------------------------------------------------------------------------------
LONG_ACTIVITY_ID = 40
CHECKSUM_LEN = 32


def _long_ids(h: WorkflowHistory):
    """ActivityIDs of 40 bytes, binary checksums and previous reset points of 32 (an md5 in hex, as Cadence
    workers report), consistently over the workflow."""
    for e in h.events:
        a = e.attrs
        if a.get("activity_id"):
            a["activity_id"] = ("activity-" + a["activity_id"] + "-").ljust(LONG_ACTIVITY_ID, "#")[:LONG_ACTIVITY_ID]
        if a.get("binary_checksum"):
            a["binary_checksum"] = hashlib.md5(a["binary_checksum"].encode()).hexdigest()
        if isinstance(a.get("prev_auto_reset_points"), list):
            a["prev_auto_reset_points"] = [hashlib.md5(p.encode()).hexdigest() for p in a["prev_auto_reset_points"]]


def _act(eid, version, ts, name):
    return HistoryEvent(int(ET.ActivityTaskScheduled), eid, version, ts, 9000 + eid,
                        {"activity_id": name.ljust(LONG_ACTIVITY_ID, "="), "domain": "domain-b",
                         "schedule_to_start_timeout_seconds": 10, "schedule_to_close_timeout_seconds": 20,
                         "start_to_close_timeout_seconds": 15, "heartbeat_timeout_seconds": 0,
                         "retry_policy": {"expiration_interval_in_seconds": 99}})


def _edge_workflow(w: int) -> WorkflowHistory:
    """Batches of one ActivityTaskScheduled event each (every blob paddable), one empty batch: the sequence
    window_batch() sizes blob by blob (see its EDGE_* roles)."""
    ts = synth_mixed.BASE_TS + 777
    batches = [[HistoryEvent(int(ET.WorkflowExecutionStarted), 1, 1, ts, 9001,
                             {"task_start_to_close_timeout_seconds": 10, "execution_start_to_close_timeout_seconds": 600,
                              "first_decision_task_backoff_seconds": 0}),
                HistoryEvent(int(ET.DecisionTaskScheduled), 2, 1, ts + 1, 9002, {"start_to_close_timeout_seconds": 10})],
               [HistoryEvent(int(ET.DecisionTaskStarted), 3, 1, ts + 2, 9003,
                             {"scheduled_event_id": 2, "request_id": det_uuid("edge", w)})],
               [HistoryEvent(int(ET.DecisionTaskCompleted), 4, 1, ts + 3, 9004,
                             {"scheduled_event_id": 2, "started_event_id": 3, "binary_checksum": "e" * CHECKSUM_LEN}),
                _act(5, 1, ts + 4, "edge-5")]]
    eid = 6
    for k in range(3, 12):
        if k == EDGE_EMPTY:
            batches.append([])
            continue
        batches.append([_act(eid, 1, ts + eid, f"edge-{eid}")])
        eid += 1
    return WorkflowHistory(batches=batches, workflow_id=f"edge-{w}", run_id=det_uuid("edge-run", w),
                           branch_id=det_uuid("edge-branch", w), now_ns=synth_mixed.BASE_TS + 10 ** 15)


# batch indices of the edge workflow
EDGE_ALIGN, EDGE_HBM15, EDGE_FIT0, EDGE_FIT16, EDGE_SMALL, EDGE_EMPTY, EDGE_ALONE = 3, 4, 5, 6, 7, 8, 9
FIT0_BYTES = K_STAGE_BYTES - 16       # a blob starting at residue r of a window fits it up to 13296 - r bytes


@dataclasses.dataclass
class WindowBatch:
    hs: List[WorkflowHistory]
    bs: object                         # blobs.BlobSet, bytes of exactly n_bytes + 32 (CRR_INGEST_PAD)
    roles: Dict[str, int]              # role -> blob index
    path: List[BlobPath]
    iterations: List[int]
    has: Dict[str, List[int]]          # what a blob holds -> blob indices


_window_batch_cache = None


def window_batch() -> WindowBatch:
    """One BlobSet of a few wavefronts (about 220 blobs, 0.4 MB and one blob of 1 MB) from mixed_histories
    workflows, populated `full`, some blobs then padded so that every edge of blob_decode_kernel's staging
    loop is reached; tests/test_decode_full_events.py asserts each edge from window_path()."""
    global _window_batch_cache
    if _window_batch_cache is not None:
        return _window_batch_cache
    from cadence_amd.thrift_codec import serialize_batch_events
    rng = random.Random(97)
    mixed = synth_mixed.mixed_histories(10, 97, multi_version=True, invalid_rate=0.2)
    for h in mixed:
        _long_ids(h)
        first = next((e for e in h.events if e.event_type == ET.ActivityTaskScheduled), None)
        if first is not None:
            first.attrs["domain"] = "domain-a"
            first.attrs["retry_policy"] = {"expiration_interval_in_seconds": 77}
    mixed[0].batches[0][0].attrs["prev_auto_reset_points"] = [hashlib.md5(b"p0").hexdigest(), hashlib.md5(b"p1").hexdigest()]
    # the edge workflow where all of it lies in one wavefront, its first blob not at lane 0
    counts = np.cumsum([0] + [len(h.batches) for h in mixed])
    k_edge = next(k for k in range(1, len(mixed)) if 1 <= counts[k] % 64 <= 64 - 14)
    many_evs, many_blob = many_events(30_000)
    tail = WorkflowHistory(batches=[[HistoryEvent(int(ET.WorkflowExecutionStarted), 1, 1, synth_mixed.BASE_TS, 4001,
                                                  {"task_start_to_close_timeout_seconds": 10}),
                                     HistoryEvent(int(ET.DecisionTaskScheduled), 2, 1, synth_mixed.BASE_TS + 1, 4002,
                                                  {"start_to_close_timeout_seconds": 10})], many_evs],
                           workflow_id="many", run_id=det_uuid("many-run"), branch_id=det_uuid("many-branch"),
                           now_ns=synth_mixed.BASE_TS + 10 ** 15)
    hs = mixed[:k_edge] + [_edge_workflow(k_edge)] + mixed[k_edge:] + [tail]
    src = sources_of(hs)
    blobs, wf_of, batch_of = [], [], []
    for w, (h, s) in enumerate(zip(hs, src)):
        for j, b in enumerate(s.blobs):
            blobs.append(many_blob if h is tail and j == 1 else populate(b, "full", rng))
            wf_of.append(w)
            batch_of.append(j)
    n = len(blobs)
    paddable = [can_pad(b) for b in blobs]

    def holds(i, pred):
        return any(pred(e) for e in hs[wf_of[i]].batches[batch_of[i]])

    has = {"act40": [i for i in range(n) if holds(i, lambda e: e.event_type == ET.ActivityTaskScheduled
                                                   and len(e.get("activity_id", "")) == LONG_ACTIVITY_ID
                                                   and e.get("domain", "") and e.attrs.get("retry_policy") is not None)],
           "prev_points": [i for i in range(n) if holds(i, lambda e: e.event_type == ET.WorkflowExecutionStarted
                                                         and isinstance(e.attrs.get("prev_auto_reset_points"), list)
                                                         and e.attrs["prev_auto_reset_points"])],
           "checksum32": [i for i in range(n) if holds(i, lambda e: e.event_type == ET.DecisionTaskCompleted
                                                        and len(e.get("binary_checksum", "")) == CHECKSUM_LEN)]}
    # -- which blob plays which role (indices only; the sizes follow in one ascending pass) --
    e0 = int(counts[k_edge])
    roles = {"hbm_res0": 0, "edge_align": e0 + EDGE_ALIGN, "hbm_res15": e0 + EDGE_HBM15, "fit0": e0 + EDGE_FIT0,
             "fit16": e0 + EDGE_FIT16, "edge_small": e0 + EDGE_SMALL, "edge_empty": e0 + EDGE_EMPTY,
             "edge_alone": e0 + EDGE_ALONE, "many_events": n - 1}
    edge_end = e0 + len(hs[k_edge].batches)
    wishes = [("hbm_res1", 1, "act40", 16_000), ("hbm_res8", 8, "checksum32", 1 << 20)]
    align_for = {}
    aligner = None
    for i in range(edge_end, n - 2):
        if not paddable[i]:
            continue
        if wishes and aligner is not None and i in has[wishes[0][2]] and 1 <= i % 64 <= 50:
            name = wishes.pop(0)[0]
            roles[name] = i
            align_for[aligner] = (i, {"hbm_res1": 1, "hbm_res8": 8}[name])
            aligner = None
        else:
            aligner = i
    assert not wishes, wishes
    align_for[roles["edge_align"]] = (roles["hbm_res15"], 15)
    sizes = {"hbm_res0": 20_000, "hbm_res1": 16_000, "hbm_res8": 1 << 20, "hbm_res15": 40_000, "edge_alone": 13_200}
    by_index = {v: k for k, v in roles.items()}
    pos = 0
    for i in range(n):
        role = by_index.get(i)
        if i in align_for:        # grown by 0..15 bytes: the target blob then starts at its residue mod 16
            tgt, r = align_for[i]
            between = sum(len(blobs[j]) for j in range(i + 1, tgt))
            blobs[i] = pad_blob(blobs[i], len(blobs[i]) + (r - (pos + len(blobs[i]) + between)) % 16)
        elif role in sizes:
            blobs[i] = pad_blob(blobs[i], sizes[role])
        elif role == "fit0":      # first pending after an HBM walk: the window starts at pos & ~15
            blobs[i] = pad_blob(blobs[i], FIT0_BYTES - pos % 16)
        elif role == "fit16":     # the same blob one 16-byte step longer
            blobs[i] = pad_blob(blobs[i], len(blobs[i - 1]) + 16)
        pos += len(blobs[i])
    k = 0
    for s in src:
        s.blobs = blobs[k:k + len(s.blobs)]
        k += len(s.blobs)
    bs = blobset_of(src)
    path, iterations = window_path(bs.blob_off)
    _window_batch_cache = WindowBatch(hs, bs, roles, path, iterations, has)
    return _window_batch_cache


# ---- (f) long and colliding keys -----------------------------------------------------------------------------------
_M = 0xFFFFFFFF


def str_hash_init(n: int) -> int:                  # ingest_kernel.hip:136
    return (2166136261 ^ (n * 0x9E3779B1)) & _M


def str_hash_step(h: int, v: int) -> int:          # ingest_kernel.hip:137-140 (v: 8 little-endian bytes)
    h = ((h ^ (v & _M)) * 16777619) & _M
    return ((h ^ (v >> 32)) * 16777619) & _M


def str_hash_final(h: int) -> int:                 # ingest_kernel.hip:141-144
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M
    h ^= h >> 16
    return h


def str_hash(b: bytes) -> int:
    """RdT::hash (ingest_kernel.hip:281-288): eight bytes per step, the tail zero-padded."""
    h = str_hash_init(len(b))
    for i in range(0, len(b), 8):
        h = str_hash_step(h, int.from_bytes(b[i:i + 8].ljust(8, b"\0"), "little"))
    return str_hash_final(h)


def colliding_pair(prefix16: bytes, rng: random.Random):
    """Two distinct 24-byte printable keys with the prefix and the same str_hash.  After the two steps over
    the prefix the state is h; the third step maps (lo, hi) to ((h ^ lo) * p ^ hi) * p, so for lo1 != lo2
    hi2 = hi1 ^ (h ^ lo1) * p ^ (h ^ lo2) * p collides (p is odd: the last multiply is a bijection)."""
    assert len(prefix16) == 16
    p = 16777619
    h = str_hash_init(24)
    h = str_hash_step(h, int.from_bytes(prefix16[:8], "little"))
    h = str_hash_step(h, int.from_bytes(prefix16[8:], "little"))
    alpha = b"abcdefghijklmnopqrstuvwxyz0123456789"
    while True:
        lo1, lo2, hi1 = (bytes(rng.choice(alpha) for _ in range(4)) for _ in range(3))
        if lo1 == lo2:
            continue
        a, b = int.from_bytes(lo1, "little"), int.from_bytes(lo2, "little")
        hi2 = (int.from_bytes(hi1, "little") ^ ((h ^ a) * p) ^ ((h ^ b) * p)) & _M
        t = hi2.to_bytes(4, "little")
        if all(0x21 <= c <= 0x7E and c not in b'"\\' for c in t):
            k1, k2 = prefix16 + lo1 + hi1, prefix16 + lo2 + t
            assert k1 != k2 and str_hash(k1) == str_hash(k2)
            return k1.decode(), k2.decode()


KEY_LENGTHS = (15, 16, 17, 24, 32, 36, 64, 300)


def _long_key(w: int, idx: int, pairs: Dict, rng: random.Random) -> str:
    """The idx-th distinct key of workflow w: the lengths of KEY_LENGTHS in turn; the keys over 16 bytes of one
    round share their first 16 bytes; pairs differ only at the last byte, in the middle, or collide."""
    j, kind = divmod(idx, 12)
    pre = f"w{w:05d}j{j:03d}-lkey-"
    assert len(pre) == 16
    tag = f"{idx:03d}"
    if kind == 0:
        return (tag + pre)[:15]
    if kind == 1:
        return (tag + pre)[:16]
    if kind in (2, 3):
        return pre + "AB"[kind - 2]                               # 17 bytes, differ at the last
    if kind in (4, 5):
        if (w, j) not in pairs:
            pairs[(w, j)] = colliding_pair(pre.encode(), rng)
        return pairs[(w, j)][kind - 4]                            # 24 bytes, the same str_hash
    if kind == 6:
        return pre + hashlib.md5(tag.encode()).hexdigest()[:16]   # 32
    if kind == 7:
        return pre + det_uuid(w, idx)[:20]                        # 36
    if kind in (8, 9):
        return pre + "y" * 45 + tag                               # 64; 8 and 9 differ at the last byte
    if kind == 10:
        return pre + "z" * 281 + tag                              # 300
    return pre + "z" * 140 + "Q" + "z" * 140 + tag                # 300, differs from kind 10 in the middle too


_KEY_ATTR = {int(ET.ActivityTaskScheduled): "activity_id", int(ET.ActivityTaskCancelRequested): "activity_id",
             int(ET.TimerStarted): "timer_id", int(ET.TimerFired): "timer_id", int(ET.TimerCanceled): "timer_id",
             int(ET.DecisionTaskCompleted): "binary_checksum"}


def workflow_keys(h: WorkflowHistory) -> List[str]:
    """The key strings a workflow's events carry, in event order (a Started event's previous reset points with
    it); "" (key 0) left out."""
    out = []
    for e in h.events:
        if e.event_type == ET.WorkflowExecutionStarted and isinstance(e.attrs.get("prev_auto_reset_points"), list):
            out += [p for p in e.attrs["prev_auto_reset_points"] if p]
        name = _KEY_ATTR.get(int(e.event_type))
        if name and e.get(name, ""):
            out.append(e.get(name))
    return out


_long_key_cache = None


def long_key_histories() -> List[WorkflowHistory]:
    """About 200 mixed workflows (most of at most 64 events: wf_pass_wave_kernel; 30 longer ones and the ones
    with previous reset points: wf_pass_kernel) whose every key string is replaced, consistently within the
    workflow, by _long_key's: which events share a key is unchanged, what the keys look like is production's."""
    global _long_key_cache
    if _long_key_cache is None:
        rng = random.Random(1234)
        hs = synth_mixed.mixed_histories(170, 51, multi_version=True, invalid_rate=0.1, can_rate=0.3)
        hs += synth_mixed.mixed_histories(30, 52, mean_len=150, multi_version=True)
        # three of 600 events: more than 64 distinct keys (a resume ingest then seeds its hash table with them)
        hs += [synth_mixed.random_workflow(rng, len(hs) + k, 600, multi_version=True) for k in range(3)]
        for w in range(0, len(hs), 9):      # more previous reset points than the walk's one in ten
            st = hs[w].batches[0][0]
            if st.event_type == ET.WorkflowExecutionStarted and not hs[w].is_new_run:
                st.attrs["prev_auto_reset_points"] = [f"bin-{k}" for k in range(1 + w % 4)]
        pairs: Dict = {}
        for w, h in enumerate(hs):
            names: Dict[str, str] = {}

            def ren(s):
                if s not in names:
                    names[s] = _long_key(w, len(names), pairs, rng)
                return names[s]
            for e in h.events:
                a = e.attrs
                if e.event_type == ET.WorkflowExecutionStarted and isinstance(a.get("prev_auto_reset_points"), list):
                    a["prev_auto_reset_points"] = [ren(p) if p else p for p in a["prev_auto_reset_points"]]
                name = _KEY_ATTR.get(int(e.event_type))
                if name and e.get(name, ""):
                    a[name] = ren(e.get(name))
        _long_key_cache = hs
    return copy.deepcopy(_long_key_cache)


def key_statistics(hs) -> Dict:
    """Over the workflows' distinct keys: the length histogram, how many exceed 16 bytes, and how many pairs
    of distinct keys of one workflow have the same length and str_hash (only those make same_bytes return
    false after a hash match)."""
    hist: Dict[int, int] = {}
    n_long = n_coll = n_prefix = 0
    for h in hs:
        keys = sorted(set(workflow_keys(h)))
        by = {}
        for k in keys:
            b = k.encode()
            hist[len(b)] = hist.get(len(b), 0) + 1
            n_long += len(b) > 16
            by.setdefault((len(b), str_hash(b)), []).append(b)
        n_coll += sum(len(v) * (len(v) - 1) // 2 for v in by.values())
        pre = {}
        for k in keys:
            if len(k) > 16:
                pre[k[:16]] = pre.get(k[:16], 0) + 1
        n_prefix += sum(v * (v - 1) // 2 for v in pre.values())
    return {"lengths": hist, "longer_than_16": n_long, "colliding_pairs": n_coll, "same_prefix_pairs": n_prefix}
