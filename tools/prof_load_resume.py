"""The resumed replay of routed replication tasks planned on the device (include/cadence_load_resume.h) on
tools/prof_load_mutation.py's workload: config-3 shard prefix states (every history cut before its last batch), 30 %
of them given a second branch, one replication task per state carrying its last batch's blob, decided and routed on
the device.

  * device: crr_load_resume_plan (the bids, the rows, the counts, the scan of the block sums, the offsets pass, the
    read-back and its synchronisation inside the span), crr_load_resume_gather (the index kernel and the byte gather)
    and crr_load_resume_finalize (the capacities, their scan, the descriptors and the arena, the read-back), HIP
    events around each call, median of --reps after one warm-up; crr_ingest_plan_resume over the gathered batch, which
    runs between the gather and the finalize, is timed beside them; the bytes each call writes;
  * beside them in the same run, what they replace, as a caller did it before: ``loader.read()`` (the whole dense image
    to the host), the host ``flatten`` of the suffixes onto it, and ``engine.upload`` of the result -- wall clock, the
    device idle before and after each, and the bytes that cross the bus in each direction;
  * the host restatement's plan and gather (crr_load_resume_host without counts) on one thread.

Prints one JSON line.  On a shared machine run it as one step under a time limit of its own, chained behind the
build:

    python __graft_entry__.py && timeout -k 10 1100 python tools/prof_load_resume.py [--wf 1250000] [--reps 5]
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


def tile_blobs(bs, reps: int, n_wf: int):
    """``bs`` repeated ``reps`` times, cut to ``n_wf`` workflows (the tasks' blobs as prof_load_ndc.workload tiles the
    tasks)."""
    import numpy as np
    from cadence_amd.blobs import BlobSet
    nb, n_bytes = bs.n_blobs, bs.n_bytes
    wf = np.tile(bs.wf, reps)
    wf["blob_begin"] = (np.arange(reps, dtype=np.int64)[:, None] * nb + bs.wf["blob_begin"][None, :].astype(np.int64)).reshape(-1)
    wf = wf[:n_wf]
    blobs = int(wf["blob_begin"][-1]) + int(wf["blob_count"][-1]) if n_wf else 0
    off = (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(n_bytes) + bs.blob_off[None, :-1]).reshape(-1)
    off = np.concatenate([off, [np.uint64(reps) * np.uint64(n_bytes)]]).astype(np.uint64)[:blobs + 1]
    data = np.concatenate([np.tile(bs.bytes[:n_bytes], reps)[:int(off[-1])], np.zeros(32, np.uint8)])
    return BlobSet(bytes=data, blob_off=off, wf=wf, strings=bs.strings)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--wf", type=int, default=1_250_000)
    p.add_argument("--sample", type=int, default=20_000)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    import numpy as np
    import torch
    from cadence_amd import abi, persisted, synth_mixed
    from cadence_amd.engine import ReplayEngine, _dev_bytes
    from cadence_amd.flatten import flatten
    from cadence_amd.ingest import DeviceIngest
    from load_resume_cases import task_blob_set
    from prof_load_ndc import workload
    from resume_cases import KNOWN, split_histories

    t0 = time.time()
    sample, _sel, _n_second, s_tasks, _s_inc, sbs, tasks, inc = workload(a.wf, a.sample)
    # the suffixes of workload()'s histories (the same generator and split)
    hs = synth_mixed.mixed_histories(a.sample, 44, mean_len=120, multi_version=True, can_rate=0.3)
    _pre, suf, _split = split_histories(hs, 7, last_only=True)
    n, n_wf = int(tasks.shape[0]), sbs.n_wf
    reps = -(-n_wf // sample.n_wf)
    tbs = tile_blobs(task_blob_set([suf[int(w)] for w in s_tasks["wf"]]), reps, n)

    eng = ReplayEngine(0)
    ld = persisted.StateLoader(eng)
    ing = DeviceIngest(eng)
    ds = ld.upload(sbs)
    ld.plan(ds)
    ld.ndc_prepare(ds, tasks, inc, on_device=True)
    _br, out = ld.last_ndc
    dtb = ing.upload(tbs)
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

    # the calls themselves (the wrappers upload their arguments and allocate: not part of the calls)
    L, vp = ld.lib, ctypes.c_void_p
    d_tasks = _dev_bytes(torch, tasks, eng.dev)
    d_rows = torch.empty(max(n, 1) * abi.LOAD_RESUME_ROW.itemsize, dtype=torch.uint8, device=eng.dev)
    work_bytes = int(L.crr_load_resume_scratch_bytes(n_wf, n))
    d_work = torch.empty(work_bytes + 16, dtype=torch.uint8, device=eng.dev)
    P = abi.CLoadResumeSizes()

    def plan():
        rc = L.crr_load_resume_plan(ctypes.byref(ds.c), vp(ld.scratch.data_ptr()), ctypes.c_size_t(ld.scratch_bytes),
                                    ctypes.byref(ld.summary), vp(d_tasks.data_ptr()), vp(out["routes"].data_ptr()), n,
                                    ctypes.byref(dtb.c), vp(d_rows.data_ptr()), vp(d_work.data_ptr()), ctypes.c_size_t(work_bytes),
                                    ctypes.byref(P), ld._stream())
        assert rc == 0 and P.err == 0, (rc, P.err)

    plan_ms, plan_all = timed(plan)
    rplan = persisted.ResumePlan(n, P, {"tasks": d_tasks, "rows": d_rows, "work": d_work, "work_bytes": work_bytes,
                                        "routes": out["routes"]}, ds, dtb)
    outs = {}

    def gather():
        outs.update(ld.resume_gather(rplan, out=outs or None))

    gather_ms, gather_all = timed(gather)
    gdb, R = ld.resume_blobs(rplan)
    S = [None]

    def ingest_plan():
        S[0] = ing.plan(gdb, resume=R)

    ingest_ms, ingest_all = timed(ingest_plan)
    arena = torch.zeros(int(P.token_bytes) + 16, dtype=torch.uint8, device=eng.dev)
    Q = [None]

    def finalize():
        Q[0] = ld.resume_finalize(rplan, gdb, ing, arena=arena)

    finalize_ms, finalize_all = timed(finalize)
    sizes = ld.resume_out_sizes(P)
    written = {"plan": n * abi.LOAD_RESUME_ROW.itemsize + work_bytes, "gather": int(sum(sizes.values())),
               "finalize": n_wf * abi.WORKFLOW.itemsize + int(P.token_bytes)}

    # what the three calls replace: the image to the host, the host layout, the upload
    def wall(fn):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t1) * 1e3

    routes = out["routes"][:n * abi.NDC_ROUTE.itemsize].cpu().numpy().view(abi.NDC_ROUTE).copy()
    mask = persisted.apply_mask(routes, tasks, n_wf)
    image, read_ms = wall(ld.read)
    image_bytes = sum(len(b) for b in image.image_bytes().values())
    suffixes = [suf[w % sample.n_wf] for w in range(n_wf)]
    lay, flatten_ms = wall(lambda: flatten(suffixes, known_domains=KNOWN, loaded=image.resumable(mask)))
    db, upload_ms = wall(lambda: eng.upload(dataclasses.replace(lay, init=None), live_ids=True))
    uploaded = sum(int(np.asarray(lay.cols[name]).nbytes) for name, _t in abi.EVENT_COLUMNS) + lay.act_side.nbytes + \
        lay.start_side.nbytes + lay.reset_keys.nbytes + lay.arena.nbytes + lay.wf.nbytes
    del db

    t1 = time.perf_counter()
    h = persisted.load_resume_host(sbs, tasks, routes, tbs)
    host_ms = (time.perf_counter() - t1) * 1e3
    got = rplan.download(outs)
    same = all(getattr(h, f).tobytes() == getattr(got, f).tobytes()
               for f in ("rows", "bytes", "blob_off", "wf", "key_begin", "key_count", "key_off", "key_len", "task_of"))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    print(json.dumps({
        "workload": f"config-3 shard shape prefix states: {n_wf} workflows, {n} tasks of one blob each ({sample.n_wf} states and "
                    f"tasks tiled)",
        "commit": commit, "workflows": n_wf, "tasks": n,
        "plan_sizes": {f: int(getattr(P, f)) for f in ("n_applied", "n_blobs", "blob_bytes", "n_keys", "key_bytes", "token_bytes",
                                                       "n_bytes", "work_needed")},
        "events_of_the_applied_tasks": int(S[0].n_events), "table_rows": [int(x) for x in Q[0].table_rows],
        "plan": {"ms": plan_ms, "passes_ms": plan_all, "bytes_written": written["plan"]},
        "gather": {"ms": gather_ms, "passes_ms": gather_all, "bytes_written": written["gather"]},
        "finalize": {"ms": finalize_ms, "passes_ms": finalize_all, "bytes_written": written["finalize"]},
        "crr_ingest_plan_resume_between": {"ms": ingest_ms, "passes_ms": ingest_all},
        "replaced_host_path": {"loader_read_ms": read_ms, "image_bytes_to_host": image_bytes, "flatten_ms": flatten_ms,
                               "upload_ms": upload_ms, "bytes_uploaded": int(uploaded),
                               "total_ms": read_ms + flatten_ms + upload_ms, "events_flattened": int(lay.n_events)},
        "host_restatement_plan_and_gather": {"threads": 1, "ms": host_ms, "equals_device": bool(same)},
        "setup_s": setup_s}), flush=True)


if __name__ == "__main__":
    main()
