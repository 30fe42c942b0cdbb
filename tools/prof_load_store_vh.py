"""The VersionHistories blob to store for routed replication tasks (include/cadence_load_store_vh.h) on
tools/prof_load_store.py's workload: config-3 shard prefix states (every history cut before its last batch), 30 % of
them given a second branch, one replication task per state, decided and routed on the device first, then every
appendable task's route set to NON_CURRENT so that every such task generates its blob.

  * device: the plan (crr_load_store_vh_plan: the size kernel, two scans, the read-back and its synchronisation all
    inside the span) and the emit kernel alone (crr_load_store_vh_run), HIP events around each call, median of --reps
    after one warm-up; the bytes written and the resulting GB/s;
  * beside them in the same call, load_store_kernel (crr_load_store_checksums) over the same tasks: it reads the same
    inputs and streams the same bytes (and the scalars and ID lists) through the CRC without storing them;
  * the host restatement (crr_load_store_vh_host) on --threads threads, the load and the branch walk it repeats
    included, both of its calls (sizing, then writing).

Prints one JSON line.  On a shared machine run it as one step under a time limit of its own, chained behind the
build:

    python __graft_entry__.py && timeout -k 10 900 python tools/prof_load_store_vh.py [--wf 1250000] [--reps 5] [--threads 16]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--wf", type=int, default=1_250_000)
    p.add_argument("--sample", type=int, default=20_000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    a = p.parse_args()
    import numpy as np
    import torch
    from cadence_amd import abi, persisted
    from cadence_amd.engine import ReplayEngine, _dev_bytes
    from prof_load_ndc import workload

    t0 = time.time()
    _sample, _sel, _n_second, _s_tasks, _s_inc, sbs, tasks, inc = workload(a.wf, a.sample)
    setup_s = time.time() - t0
    n = int(tasks.shape[0])
    last = np.zeros(n, abi.LAST_EVENT)
    last["event_id"], last["version"] = tasks["first_event_id"], tasks["first_event_version"]

    eng = ReplayEngine(0)
    ld = persisted.StateLoader(eng)
    ds = ld.upload(sbs)
    ld.plan(ds)
    results, routes, _out = ld.ndc_prepare(ds, tasks, inc)
    br, out = ld.last_ndc
    forced = routes.copy()
    forced["route"][(results["status"] == 0) & (results["action"] == abi.NDC_APPEND)] = abi.ROUTE_NON_CURRENT
    raw = torch.from_numpy(forced.view(np.uint8).reshape(-1).copy())
    out["routes"][:raw.numel()].copy_(raw)

    def timed(fn):
        ms = []
        for _ in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms[1:])), ms

    # the calls themselves (the wrappers upload their arguments and copy the results back: not part of the kernels)
    L = ld.lib
    vp = ctypes.c_void_p
    d_tasks, d_last = _dev_bytes(torch, tasks, eng.dev), _dev_bytes(torch, last, eng.dev)
    d_sums = torch.empty(max(n, 1) * abi.STORE_ROW.itemsize, dtype=torch.uint8, device=eng.dev)
    d_rows = torch.empty(max(n, 1) * abi.VH_BLOB_ROW.itemsize, dtype=torch.uint8, device=eng.dev)
    d_off = torch.empty((n + 1) * 8, dtype=torch.uint8, device=eng.dev)
    work_bytes = int(L.crr_load_store_vh_scratch_bytes(n))
    d_work = torch.empty(work_bytes + 16, dtype=torch.uint8, device=eng.dev)
    P = abi.CVhBlobSizes()
    head = (ctypes.byref(ds.c), vp(ld.scratch.data_ptr()), ctypes.c_size_t(ld.scratch_bytes), ctypes.byref(ld.summary),
            vp(d_tasks.data_ptr()), vp(d_last.data_ptr()))
    tail = (vp(out["results"].data_ptr()), vp(out["routes"].data_ptr()), ctypes.byref(br.c), ctypes.byref(br.plan), None, None, None)

    def checksums():
        rc = L.crr_load_store_checksums(*head, n, *tail, vp(d_sums.data_ptr()), ld._stream())
        assert rc == 0, rc

    def plan():
        rc = L.crr_load_store_vh_plan(*head, n, *tail, vp(d_rows.data_ptr()), vp(d_off.data_ptr()), vp(d_work.data_ptr()),
                                      ctypes.c_size_t(work_bytes), ctypes.byref(P), ld._stream())
        assert rc == 0 and P.err == 0, (rc, P.err)

    plan_ms, plan_all = timed(plan)
    n_bytes = int(P.n_bytes)
    padded = (n_bytes + 15) // 16 * 16
    d_out = torch.empty(max(padded, 16), dtype=torch.uint8, device=eng.dev)

    def emit():
        rc = L.crr_load_store_vh_run(*head, *tail, vp(d_rows.data_ptr()), vp(d_off.data_ptr()), ctypes.byref(P),
                                     vp(d_out.data_ptr()), ctypes.c_size_t(padded), ld._stream())
        assert rc == 0, rc

    emit_ms, emit_all = timed(emit)
    sums_ms, sums_all = timed(checksums)
    rows = d_rows[:n * abi.VH_BLOB_ROW.itemsize].cpu().numpy().view(abi.VH_BLOB_ROW).copy()
    off = d_off.cpu().numpy().view(np.uint64).copy()
    data = d_out[:n_bytes].cpu().numpy()

    host_s = []
    for _ in range(max(a.reps // 2, 1)):
        t1 = time.perf_counter()
        h_rows, h_off, h_data = persisted.store_version_histories_host(sbs, tasks, last, results, forced, threads=a.threads)
        host_s.append(time.perf_counter() - t1)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    print(json.dumps({
        "workload": f"config-3 shard shape prefix states: {sbs.n_wf} workflows, {n} tasks, {int(br.plan.n_branches)} branches, "
                    "every appendable task routed NON_CURRENT",
        "commit": commit, "workflows": sbs.n_wf, "tasks": n, "generated": int(P.n_generated), "blob_bytes": n_bytes,
        "mean_blob_bytes": n_bytes / max(int(P.n_generated), 1),
        "plan": {"ms": plan_ms, "passes_ms": plan_all},
        "emit_kernel": {"ms": emit_ms, "passes_ms": emit_all, "GB_per_s_written": padded / emit_ms / 1e6 if emit_ms else 0.0},
        "load_store_kernel_same_tasks": {"ms": sums_ms, "passes_ms": sums_all},
        "host_restatement": {"threads": a.threads, "ms": float(np.median(host_s)) * 1e3,
                             "equals_device": bool(h_rows.tobytes() == rows.tobytes() and h_off.tobytes() == off.tobytes()
                                                   and h_data.tobytes() == data.tobytes())},
        "outcomes": {str(k): int(v) for k, v in enumerate(np.bincount(rows["outcome"], minlength=8))},
        "setup_s": setup_s}), flush=True)


if __name__ == "__main__":
    main()
