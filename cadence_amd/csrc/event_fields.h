// HistoryEvent's attribute fields (.gen/go/shared/shared.go:42000-42460): one *EventAttributes struct per event
// type at ids 40, 50, ... 450.  The ids follow the thrift struct's declaration order, which leaves the
// EventType order (cadence_replay.h CRR_EV_*) in slots 14..28: ids 180..320 hold TimerStarted, TimerFired,
// ActivityTaskCancelRequested, RequestCancelActivityTaskFailed, ActivityTaskCanceled, TimerCanceled,
// CancelTimerFailed, MarkerRecorded, WorkflowExecutionSignaled, WorkflowExecutionTerminated,
// WorkflowExecutionCancelRequested, WorkflowExecutionCanceled, RequestCancelExternalWorkflowExecutionInitiated,
// RequestCancelExternalWorkflowExecutionFailed, ExternalWorkflowExecutionCancelRequested.  Both directions as a
// nibble table of (difference + 5): no memory access, shared by the host decoder, the device ingest, the JSON
// transcode and the blob encoder.
#ifndef CADENCE_EVENT_FIELDS_H_
#define CADENCE_EVENT_FIELDS_H_

#if defined(__HIPCC__)
#define CRR_FIELDS_HD __host__ __device__
#else
#define CRR_FIELDS_HD
#endif

// field id -> event type (CRR_EV_*), -1: not an attribute field
static inline CRR_FIELDS_HD int event_attr_type_of_field(int id) {
  if (id < 40 || id > 450 || id % 10) return -1;
  const int k = (id - 40) / 10;
  if (k < 14 || k > 28) return k;
  return k + (int)((0x22222AAA4633388ull >> (4 * (k - 14))) & 15) - 5;
}

// event type (0 .. CRR_EV_TYPE_COUNT - 1) -> field id
static inline CRR_FIELDS_HD int event_attr_field_of_type(int t) {
  const int k = t < 14 || t > 28 ? t : t + (int)((0x000888884622777ull >> (4 * (t - 14))) & 15) - 5;
  return 40 + 10 * k;
}

#endif  // CADENCE_EVENT_FIELDS_H_
