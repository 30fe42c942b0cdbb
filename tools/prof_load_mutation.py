"""The pending-entry mutation to store for routed replication tasks (include/cadence_load_mutation.h) on
tools/prof_load_store_vh.py's workload: config-3 shard prefix states (every history cut before its last batch), 30 %
of them given a second branch, one replication task per state, decided and routed on the device.

The states after come from a real resumed replay: the sample's tasks are decided, its states placed and its suffixes
replayed on the device; the rows that replay left are then tiled, like the blobs, into a canonical (stride 1) layout
of --wf positions whose slot tables hold exactly those rows.  The mutation kernels only read them.

  * device: the plan (crr_load_mutation_plan: the count kernel, the scan of the block sums, the offsets pass, the
    read-back and its synchronisation all inside the span) and the run (crr_load_mutation_run: the directory's memset,
    the emit kernel and the six gathers), HIP events around each call, median of --reps after one warm-up; the bytes
    the mutation holds;
  * beside them in the same call, crr_compact_rows over the same post-replay rows with its bytes: the snapshot
    download the mutation replaces;
  * the host restatement (crr_load_mutation_host) on --threads threads, the load and the branch walk it repeats
    included, both of its calls (sizing, then writing).

Prints one JSON line.  On a shared machine run it as one step under a time limit of its own, chained behind the
build:

    python __graft_entry__.py && timeout -k 10 1100 python tools/prof_load_mutation.py [--wf 1250000] [--reps 5] [--threads 16]
"""
import argparse
import ctypes
import dataclasses
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
    from cadence_amd import abi, persisted, synth_mixed
    from cadence_amd.engine import DeviceBatch, ReplayEngine, _dev_bytes
    from cadence_amd.flatten import HistoryBatch, LoadedStates, flatten
    from prof_load_ndc import workload
    from resume_cases import KNOWN, split_histories

    t0 = time.time()
    sample, _sel, _n_second, s_tasks, s_inc, sbs, tasks, inc = workload(a.wf, a.sample)
    # the suffixes of workload()'s histories (the same generator and split)
    hs = synth_mixed.mixed_histories(a.sample, 44, mean_len=120, multi_version=True, can_rate=0.3)
    _pre, suf, _split = split_histories(hs, 7, last_only=True)
    n = int(tasks.shape[0])
    last = np.zeros(n, abi.LAST_EVENT)
    last["event_id"], last["version"] = tasks["first_event_id"], tasks["first_event_version"]

    eng = ReplayEngine(0)
    ld = persisted.StateLoader(eng)
    # the sample's resumed replay
    ds_s = ld.upload(sample)
    ld.plan(ds_s)
    _res, s_routes, _out = ld.ndc_prepare(ds_s, s_tasks, s_inc)
    mask = persisted.apply_mask(s_routes, s_tasks, sample.n_wf)
    lay = flatten(suf, known_domains=KNOWN, loaded=ld.read().resumable(mask))
    db_s = eng.upload(dataclasses.replace(lay, init=None), live_ids=True)
    ld.place(db_s, perm=lay.perm)
    eng.launch(db_s)
    after_s = eng.download(db_s).to_loaded(lay, mask=mask)
    replay_failed = int(((after_s.exec["status"] != 0) & mask).sum())
    del db_s, ds_s

    # ... tiled into a canonical layout of the full size
    n_wf, reps = sbs.n_wf, -(-sbs.n_wf // sample.n_wf)
    ex = np.tile(after_s.exec, reps)[:n_wf]
    big_mask = np.tile(mask, reps)[:n_wf]
    wf = np.zeros(n_wf, abi.WORKFLOW)
    wf["flags"][big_mask] = abi.WF_FLAG_RESUME
    T = {"exec": torch.from_numpy(ex.view(np.uint8).reshape(-1).copy()).to(eng.dev)}
    ci, co = abi.CInputs(), abi.COutputs()
    co.exec = T["exec"].data_ptr()
    table_rows, snapshot_bytes = {}, ex.nbytes
    for name, dt, base_f, cap_f, _n_f in abi.TABLES[:7]:
        c = np.tile(after_s.counts(name), reps)[:n_wf]
        off = np.cumsum(c) - c
        total = int(c.sum())
        wf[base_f], wf[cap_f] = off, c
        rows = np.tile(after_s.rows[name], reps)[:total]
        T["out_" + name] = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(eng.dev) if total else \
            torch.zeros(dt.itemsize, dtype=torch.uint8, device=eng.dev)
        setattr(co, name, T["out_" + name].data_ptr())
        table_rows[name] = total
        snapshot_bytes += total * dt.itemsize
    T["out_tasks"] = torch.zeros(abi.TASK_ROW.itemsize, dtype=torch.uint8, device=eng.dev)
    co.tasks = T["out_tasks"].data_ptr()
    T["wf"] = torch.from_numpy(wf.view(np.uint8).reshape(-1).copy()).to(eng.dev)
    ci.wf, ci.n_wf, ci.stride = T["wf"].data_ptr(), n_wf, 1
    batch = HistoryBatch(cols={}, act_side=None, start_side=None, reset_keys=None, arena=None, wf=wf, stride=1)
    batch.table_rows = table_rows
    db = DeviceBatch(batch=batch, tensors=T, c_in=ci, c_out=co, device=0)
    after = LoadedStates(ex, {name: np.tile(after_s.rows[name], reps)[:table_rows[name]] for name in table_rows}, big_mask, None)

    ds = ld.upload(sbs)
    ld.plan(ds)
    results, routes, _out = ld.ndc_prepare(ds, tasks, inc)
    br, out = ld.last_ndc
    setup_s = time.time() - t0

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
    d_rows = torch.empty(max(n, 1) * abi.MUTATION_ROW.itemsize, dtype=torch.uint8, device=eng.dev)
    work_bytes = int(L.crr_load_mutation_scratch_bytes(n))
    d_work = torch.empty(work_bytes + 16, dtype=torch.uint8, device=eng.dev)
    P = abi.CMutationSizes()
    head = (ctypes.byref(ds.c), vp(ld.scratch.data_ptr()), ctypes.c_size_t(ld.scratch_bytes), ctypes.byref(ld.summary),
            vp(d_tasks.data_ptr()), vp(d_last.data_ptr()))
    tail = (vp(out["results"].data_ptr()), vp(out["routes"].data_ptr()), ctypes.byref(br.c), ctypes.byref(br.plan),
            ctypes.byref(ci), ctypes.byref(co), None)

    def plan():
        rc = L.crr_load_mutation_plan(*head, n, *tail, vp(d_rows.data_ptr()), vp(d_work.data_ptr()), ctypes.c_size_t(work_bytes),
                                      ctypes.byref(P), ld._stream())
        assert rc == 0 and P.err == 0, (rc, P.err)

    plan_ms, plan_all = timed(plan)
    mplan = persisted.MutationPlan(n, P, {"rows": d_rows, "work": d_work}, head, tail)
    outs = {}

    def run():
        outs.update(ld.mutation_run(mplan, out=outs or None))

    run_ms, run_all = timed(run)
    got = mplan.download(outs)
    compact_ms, compact_all = timed(lambda: eng.compact(db))
    cmp_off = T["cmp_offsets"].cpu().numpy().reshape(-1, n_wf + 1)
    compact_bytes = ex.nbytes + sum(int(cmp_off[t, n_wf]) * dt.itemsize for t, (_name, dt, *_r) in enumerate(abi.TABLES[:7]))

    host_s = []
    for _ in range(max(a.reps // 2, 1)):
        t1 = time.perf_counter()
        h = persisted.mutation_host(sbs, tasks, last, results, routes, after, threads=a.threads)
        host_s.append(time.perf_counter() - t1)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    payload = got.n_bytes - got.rows.nbytes
    print(json.dumps({
        "workload": f"config-3 shard shape prefix states: {n_wf} workflows, {n} tasks; the rows after are a resumed replay of "
                    f"{sample.n_wf} states tiled",
        "commit": commit, "workflows": n_wf, "tasks": n, "sample_replays_failed": replay_failed,
        "outcomes": {str(k): int(v) for k, v in enumerate(np.bincount(got.rows["outcome"], minlength=8))},
        "exec_rows": int(P.n_exec), "upserted_rows": dict(zip(abi.MUTATION_MAPS, (int(x) for x in P.n_upsert))),
        "deleted_keys": dict(zip(abi.MUTATION_MAPS, (int(x) for x in P.n_delete))),
        "live_rows_after": {k: int(v) for k, v in table_rows.items()},
        "plan": {"ms": plan_ms, "passes_ms": plan_all},
        "run": {"ms": run_ms, "passes_ms": run_all, "directory_bytes": int(P.run_work_needed)},
        "mutation_bytes": {"exec_upserts_keys": payload, "task_rows": int(got.rows.nbytes), "all": got.n_bytes},
        "crr_compact_rows_same_rows": {"ms": compact_ms, "passes_ms": compact_all, "bytes": compact_bytes,
                                       "bytes_expected": snapshot_bytes},
        "bytes_ratio_mutation_to_snapshot": got.n_bytes / compact_bytes,
        "host_restatement": {"threads": a.threads, "ms": float(np.median(host_s)) * 1e3,
                             "equals_device": bool(h.image_bytes() == got.image_bytes())},
        "setup_s": setup_s}), flush=True)


if __name__ == "__main__":
    main()
