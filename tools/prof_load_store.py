"""The checksum to store for routed replication tasks (include/cadence_load_store.h) on tools/prof_load_ndc.py's
workload: config-3 shard prefix states (every history cut before its last batch), 30 % of them given a second
branch, one replication task per state, decided and routed on the device first.

  * device: load_store_kernel alone (crr_load_store_checksums), HIP events around the call, median of --reps after
    one warm-up -- once as routed without a resumed replay (the tasks on the current route end as not resumed,
    the others are generated or refused), and once with every appendable task's route set to NON_CURRENT, so that
    every such task generates its payload from the loaded image and the branch table (the full payload work per
    task; the replayed rows of an APPLIED task are the same number of bytes from another place);
  * beside it in the same call, load_verify_kernel (crr_load_states_verify) over the same states: the nearest
    existing kernel, one payload per state from the same scratch;
  * the host restatement (crr_load_store_checksums_host) on --threads threads, the load and the branch walk it
    repeats included.

Prints one JSON line.

    python tools/prof_load_store.py [--wf 1250000] [--sample 20000] [--reps 5] [--threads 16]
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
    from cadence_amd.engine import ReplayEngine
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

    # the calls themselves (the wrappers upload their arguments and copy the rows back: not part of the kernel)
    L = ld.lib
    br, out = ld.last_ndc
    from cadence_amd.engine import _dev_bytes
    d_tasks, d_last = _dev_bytes(torch, tasks, eng.dev), _dev_bytes(torch, last, eng.dev)
    d_rows = torch.empty(max(n, 1) * abi.STORE_ROW.itemsize, dtype=torch.uint8, device=eng.dev)
    d_verify = torch.empty(max(sbs.n_wf, 1) * abi.VERIFY_ROW.itemsize, dtype=torch.uint8, device=eng.dev)
    vp = ctypes.c_void_p

    def store():
        rc = L.crr_load_store_checksums(ctypes.byref(ds.c), vp(ld.scratch.data_ptr()), ctypes.c_size_t(ld.scratch_bytes),
                                        ctypes.byref(ld.summary), vp(d_tasks.data_ptr()), vp(d_last.data_ptr()), n,
                                        vp(out["results"].data_ptr()), vp(out["routes"].data_ptr()), ctypes.byref(br.c),
                                        ctypes.byref(br.plan), None, None, None, vp(d_rows.data_ptr()), ld._stream())
        assert rc == 0, rc

    def verify():
        rc = L.crr_load_states_verify(ctypes.byref(ds.c), vp(ld.scratch.data_ptr()), ctypes.c_size_t(ld.scratch_bytes),
                                      ctypes.byref(ld.summary), None, 0, vp(d_verify.data_ptr()), ld._stream())
        assert rc == 0, rc

    def rows():
        return d_rows[:n * abi.STORE_ROW.itemsize].cpu().numpy().view(abi.STORE_ROW).copy()

    routed_ms, routed_all = timed(store)
    routed = rows()
    verify_ms, verify_all = timed(verify)
    # every appendable task generated from the loaded image
    forced = routes.copy()
    forced["route"][(results["status"] == 0) & (results["action"] == abi.NDC_APPEND)] = abi.ROUTE_NON_CURRENT
    raw = torch.from_numpy(forced.view(np.uint8).reshape(-1).copy())
    out["routes"][:raw.numel()].copy_(raw)
    full_ms, full_all = timed(store)
    full = rows()

    host_s = []
    for _ in range(max(a.reps // 2, 1)):
        t1 = time.perf_counter()
        h = persisted.store_checksums_host(sbs, tasks, last, results, forced, threads=a.threads)
        host_s.append(time.perf_counter() - t1)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    gen = int(np.isin(full["outcome"], [abi.StoreOutcome.APPLIED, abi.StoreOutcome.BACKFILLED]).sum())
    print(json.dumps({
        "workload": f"config-3 shard shape prefix states: {sbs.n_wf} workflows, {n} tasks, {int(br.plan.n_branches)} branches",
        "commit": commit, "workflows": sbs.n_wf, "tasks": n,
        "as_routed_without_replay": {"kernel_ms": routed_ms, "passes_ms": routed_all,
                                     "outcomes": {str(k): int(v) for k, v in enumerate(np.bincount(routed["outcome"], minlength=8))}},
        "every_appendable_task_generated": {"kernel_ms": full_ms, "passes_ms": full_all, "generated": gen,
                                            "payload_bytes": int(full["payload_len"].astype(np.int64).sum()),
                                            "tasks_per_s": n / full_ms * 1e3,
                                            "outcomes": {str(k): int(v) for k, v in enumerate(np.bincount(full["outcome"], minlength=8))}},
        "load_verify_kernel_same_states": {"kernel_ms": verify_ms, "passes_ms": verify_all},
        "host_restatement": {"threads": a.threads, "ms": float(np.median(host_s)) * 1e3, "rows_equal_device": bool(h.tobytes() == full.tobytes())},
        "setup_s": setup_s}), flush=True)


if __name__ == "__main__":
    main()
