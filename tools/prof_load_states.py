"""Persisted mutable-state loader probe (include/cadence_load.h): the config-3 shard's prefix states -- every
history cut before its last batch, as the passive-replication line of the bench cuts them -- written as the
SQL store persists them, then

  * device: crr_load_states_plan + crr_load_states_place on blobs resident in HBM, HIP events around the pair
    (the plan's two stream synchronisations are inside the span), median of --reps after one warm-up;
  * host:   crr_load_states_host on --threads threads, wall time, median of --reps.

The Python reference encoder writes about 10k states/s, so --sample states are encoded and the blob set is
tiled to --wf workflows (the loader treats every workflow independently; the tile keeps the shard's mix of
pending entries, reset points and version-history items).  Prints one JSON line.

    python tools/prof_load_states.py [--wf 1250000] [--sample 20000] [--reps 5] [--threads 16]
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


def bench_blob_step_ms():
    """BENCH_r06.json: passive_replication.blob_path.device_resident_ms (the step the load is compared with)."""
    import re
    with open(os.path.join(ROOT, "BENCH_r06.json")) as f:
        txt = f.read()
    m = re.search(r'passive_replication.{0,600}?device_resident_ms\\*"?: ?([0-9.]+)', txt, re.S)
    return float(m.group(1))


def tile(sbs, n_wf):
    """The blob set repeated until it holds n_wf workflows."""
    import numpy as np
    from cadence_amd import abi
    from cadence_amd.persisted import StateBlobSet
    reps = -(-n_wf // sbs.n_wf)
    nb, nbytes = sbs.n_blobs, sbs.n_bytes
    data = np.concatenate([np.tile(sbs.bytes[:nbytes], reps), np.zeros(abi.INGEST_PAD, np.uint8)])
    off = (np.arange(reps, dtype=np.uint64)[:, None] * np.uint64(nbytes) + sbs.blob_off[None, :-1]).reshape(-1)
    off = np.concatenate([off, np.array([reps * nbytes], np.uint64)])
    blob = np.tile(sbs.blob, reps)
    wf = np.tile(sbs.wf, reps)
    wf["blob_begin"] = (np.arange(reps, dtype=np.int64)[:, None] * nb + sbs.wf["blob_begin"][None, :].astype(np.int64)).reshape(-1)
    keep = n_wf
    n_blobs = int(wf["blob_begin"][keep - 1]) + int(wf["blob_count"][keep - 1])
    end = int(off[n_blobs])
    data = np.concatenate([data[:end], np.zeros(abi.INGEST_PAD, np.uint8)])
    return StateBlobSet(data, off[:n_blobs + 1].copy(), blob[:n_blobs].copy(), wf[:keep].copy(), sbs.strings)


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
    from cadence_amd.engine import DeviceBatch, ReplayEngine
    from cadence_amd.flatten import HistoryBatch, flatten
    from oracle import oracle
    from resume_cases import KNOWN, split_histories

    t0 = time.time()
    hs = synth_mixed.mixed_histories(a.sample, 44, mean_len=120, multi_version=True, can_rate=0.3)
    pre, _suf, _mask = split_histories(hs, 7, last_only=True)
    pre_b = flatten(pre, known_domains=KNOWN)
    sample = persisted.encode_states(pre_b, oracle.replay(pre_b, 0), pre)
    sbs = tile(sample, a.wf)
    setup_s = time.time() - t0

    # host
    L = persisted._host_lib()
    c = persisted._c_batch(sbs, lambda x: x.ctypes.data)
    S = abi.CLoadSummary()
    assert L.crr_load_states_host(ctypes.byref(c), None, ctypes.byref(S), a.threads) == 0
    buf = persisted._ImageBuffers(S)
    host_s = []
    for _ in range(a.reps):
        t1 = time.perf_counter()
        assert L.crr_load_states_host(ctypes.byref(c), ctypes.byref(buf.c), ctypes.byref(S), a.threads) == 0
        host_s.append(time.perf_counter() - t1)
    host = buf.image(S) if sbs.n_wf <= 50_000 else None
    tot = [int(x) for x in S.totals]

    # device: a canonical (stride 1) layout whose slot tables hold exactly the loaded rows
    eng = ReplayEngine(0)
    ld = persisted.StateLoader(eng)
    ds = ld.upload(sbs)
    wf = np.zeros(sbs.n_wf, abi.WORKFLOW)
    wf["flags"] = abi.WF_FLAG_RESUME
    for t, (name, _dt, base_f, cap_f, _n) in enumerate(abi.TABLES[:7]):
        wf[base_f] = buf.offsets[t][:-1]
        wf[cap_f] = np.diff(buf.offsets[t])
    T = {"wf": torch.from_numpy(wf.view(np.uint8)).to(eng.dev),
         "exec": torch.zeros(sbs.n_wf * abi.EXEC_ROW.itemsize, dtype=torch.uint8, device=eng.dev)}
    ci, co = abi.CInputs(), abi.COutputs()
    ci.wf, ci.n_wf, ci.stride = T["wf"].data_ptr(), sbs.n_wf, 1
    co.exec = T["exec"].data_ptr()
    for t, (name, dt, *_r) in enumerate(abi.TABLES[:7]):
        T["out_" + name] = torch.zeros(max(tot[t], 1) * dt.itemsize, dtype=torch.uint8, device=eng.dev)
        setattr(co, name, T["out_" + name].data_ptr())
    for t, name in enumerate(abi.ID_TABLES):
        T["ids_" + name] = torch.zeros(max(tot[t], 1), dtype=torch.int64, device=eng.dev)
        co.live_ids[t] = T["ids_" + name].data_ptr()
    batch = HistoryBatch(cols={}, act_side=None, start_side=None, reset_keys=None, arena=None, wf=wf, stride=1)
    db = DeviceBatch(batch=batch, tensors=T, c_in=ci, c_out=co, device=0)
    dev_ms, plan_ms = [], []
    for _ in range(a.reps + 1):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize()
        e0.record()
        ld.plan(ds)
        e1.record()
        ld.place(db, perm=None)
        e2.record()
        torch.cuda.synchronize()
        plan_ms.append(e0.elapsed_time(e1))
        dev_ms.append(e0.elapsed_time(e2))
    same = None
    if host is not None:
        same = ld.read().image_bytes() == host.image_bytes()
    placed = T["exec"].cpu().numpy().view(abi.EXEC_ROW)
    rows_ok = bool((placed["status"] == 0).all() and placed.tobytes() == buf.exec.tobytes())
    d_ms, h_s = float(np.median(dev_ms[1:])), float(np.median(host_s))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    print(json.dumps({
        "workload": f"config-3 shard shape prefix states: {sbs.n_wf} workflows tiled from {sample.n_wf} encoded ones",
        "commit": commit, "workflows": sbs.n_wf, "blobs": sbs.n_blobs, "blob_bytes": sbs.n_bytes,
        "rows": dict(zip(abi.LOAD_ROW_TABLES, tot[:7])), "failed": int(S.n_failed),
        "device": {"plan_place_ms": d_ms, "plan_ms": float(np.median(plan_ms[1:])), "states_per_s": sbs.n_wf / d_ms * 1e3,
                   "GBs": sbs.n_bytes / d_ms / 1e6, "placed_exec_rows_equal_host": rows_ok, "image_equals_host": same,
                   "passes_ms": dev_ms},
        "host": {"threads": a.threads, "ms": h_s * 1e3, "states_per_s": sbs.n_wf / h_s, "GBs": sbs.n_bytes / h_s / 1e9},
        "device_vs_host": h_s * 1e3 / d_ms,
        "share_of_bench_r06_blob_step": d_ms / bench_blob_step_ms(),
        "setup_s": setup_s}), flush=True)


if __name__ == "__main__":
    main()
