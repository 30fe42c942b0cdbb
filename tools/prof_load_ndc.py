"""Branch decision and routing from persisted states (include/cadence_load_ndc.h): tools/prof_load_states.py's
config-3 shard prefix states (every history cut before its last batch), 30 % of them given a second branch, one
replication task per state -- the state's last batch, carrying the history's version-history items after it --

  * device: crr_load_ndc_plan + crr_load_ndc_run (branch extraction, crr_ndc_prepare, routing) on states, tasks
    and incoming items resident in HBM, after crr_load_states_plan; HIP events around the pair (the planning
    call's one stream synchronisation is inside the span), median of --reps after one warm-up;
  * the route without it: the states' VersionHistories blobs parsed on the host, ndc.pack, upload and
    crr_ndc_prepare.  That route is Python per state, so it is run on the --sample encoded states only and its
    wall time is reported per state and scaled linearly to --wf (labelled as such).

--sample states are encoded and tiled to --wf workflows as in prof_load_states.py.  Prints one JSON line.

    python tools/prof_load_ndc.py [--wf 1250000] [--sample 20000] [--reps 5]
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def parse_version_histories(raw: bytes):
    """shared.VersionHistories (0x59 preamble, thrift binary) -> (current index, [items per branch]): what a host
    that holds only the persisted bytes has to do before ndc.pack."""
    pos = 1
    current, branches = 0, []

    def skip(t, pos):
        if t in (2, 3):
            return pos + 1
        if t == 6:
            return pos + 2
        if t == 8:
            return pos + 4
        if t in (4, 10):
            return pos + 8
        if t == 11:
            return pos + 4 + struct.unpack_from(">i", raw, pos)[0]
        raise ValueError(t)
    while raw[pos] != 0:
        t, fid = raw[pos], struct.unpack_from(">h", raw, pos + 1)[0]
        pos += 3
        if fid == 10 and t == 8:
            current = struct.unpack_from(">i", raw, pos)[0]
            pos += 4
        elif fid == 20 and t == 15:
            n = struct.unpack_from(">i", raw, pos + 1)[0]
            pos += 5
            for _ in range(n):
                items = []
                while raw[pos] != 0:
                    t2, fid2 = raw[pos], struct.unpack_from(">h", raw, pos + 1)[0]
                    pos += 3
                    if fid2 == 20 and t2 == 15:
                        m = struct.unpack_from(">i", raw, pos + 1)[0]
                        pos += 5
                        for _ in range(m):
                            e = v = 0
                            while raw[pos] != 0:
                                t3, fid3 = raw[pos], struct.unpack_from(">h", raw, pos + 1)[0]
                                pos += 3
                                if t3 == 10 and fid3 == 10:
                                    e = struct.unpack_from(">q", raw, pos)[0]
                                elif t3 == 10 and fid3 == 20:
                                    v = struct.unpack_from(">q", raw, pos)[0]
                                pos = skip(t3, pos)
                            pos += 1
                            items.append((e, v))
                    else:
                        pos = skip(t2, pos)
                pos += 1
                branches.append(items)
        else:
            pos = skip(t, pos)
    return current, branches


def execution_field(raw: bytes, want: int) -> bytes:
    """A binary field of a sqlblobs.WorkflowExecutionInfo blob (its lists and maps hold strings only)."""
    pos = 0
    while raw[pos] != 0:
        t, fid = raw[pos], struct.unpack_from(">h", raw, pos + 1)[0]
        pos += 3
        if t == 11:
            n = struct.unpack_from(">i", raw, pos)[0]
            if fid == want:
                return raw[pos + 4:pos + 4 + n]
            pos += 4 + n
        elif t in (2, 3):
            pos += 1
        elif t == 8:
            pos += 4
        elif t in (4, 10):
            pos += 8
        elif t == 15:
            n = struct.unpack_from(">i", raw, pos + 1)[0]
            pos += 5
            for _ in range(n):
                pos += 4 + struct.unpack_from(">i", raw, pos)[0]
        elif t == 13:
            n = struct.unpack_from(">i", raw, pos + 2)[0]
            pos += 6
            for _ in range(2 * n):
                pos += 4 + struct.unpack_from(">i", raw, pos)[0]
        else:
            raise ValueError(t)
    return b""


def workload(n_wf: int, n_sample: int):
    """(encoded sample, its task states, how many got a second branch, sample tasks, sample incoming items, tiled
    blob set, tiled tasks, tiled incoming items)."""
    import numpy as np
    from cadence_amd import abi, persisted, synth_mixed
    from cadence_amd.flatten import flatten
    from oracle import oracle
    from prof_load_states import tile
    from resume_cases import KNOWN, split_histories

    hs = synth_mixed.mixed_histories(n_sample, 44, mean_len=120, multi_version=True, can_rate=0.3)
    pre, suf, split = split_histories(hs, 7, last_only=True)
    pre_b, one_b = flatten(pre, known_domains=KNOWN), flatten(hs, known_domains=KNOWN)
    pre_r, one_r = oracle.replay(pre_b, 0), oracle.replay(one_b, 0)

    def vh(batch, res):
        loaded = res.to_loaded(batch)
        c = loaded.counts("vh").astype(np.int64)
        return loaded.mask, c, np.cumsum(c) - c, loaded.rows["vh"]
    ok, lc_, lo, lrows = vh(pre_b, pre_r)
    ok1, ac, ao, arows = vh(one_b, one_r)
    sel = np.nonzero(ok & ok1 & np.asarray(split, bool) & (lc_ > 0))[0]
    rng = np.random.default_rng(9)
    second = set(int(w) for w in sel[rng.random(sel.size) < 0.3] if int(lrows["event_id"][lo[w]]) >= 2)
    branches = {w: ([None, (b"stale-branch-token", [(1, int(lrows["version"][lo[w]]))])], int(rng.random() < 0.5)) for w in second}
    sample = persisted.encode_states(pre_b, pre_r, pre, branches=branches)
    # one task per selected state: (wf, incoming range, first event of the last batch)
    s_tasks = np.zeros(sel.size, abi.REPL_TASK)
    s_tasks["wf"] = sel
    s_tasks["incoming_count"] = ac[sel]
    s_tasks["incoming_begin"] = np.cumsum(ac[sel]) - ac[sel]
    s_tasks["first_event_id"] = [suf[w].batches[0][0].id for w in sel]
    s_tasks["first_event_version"] = [suf[w].batches[0][0].version for w in sel]
    s_inc = np.concatenate([arows[int(ao[w]):int(ao[w] + ac[w])] for w in sel]) if sel.size else np.zeros(0, abi.VH_ITEM)
    sbs = tile(sample, n_wf)
    reps = -(-n_wf // sample.n_wf)
    tasks = np.tile(s_tasks, reps)
    tasks["wf"] = (np.arange(reps, dtype=np.int64)[:, None] * sample.n_wf + s_tasks["wf"][None, :]).reshape(-1)
    tasks["incoming_begin"] = (np.arange(reps, dtype=np.int64)[:, None] * s_inc.shape[0] + s_tasks["incoming_begin"][None, :]).reshape(-1)
    tasks = tasks[tasks["wf"] < sbs.n_wf]
    return sample, sel, len(second), s_tasks, s_inc, sbs, tasks, np.tile(s_inc, reps)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--wf", type=int, default=1_250_000)
    p.add_argument("--sample", type=int, default=20_000)
    p.add_argument("--reps", type=int, default=5)
    a = p.parse_args()
    import numpy as np
    import torch
    from cadence_amd import abi, ndc, persisted
    from cadence_amd.engine import ReplayEngine, _dev_bytes

    t0 = time.time()
    sample, sel, n_second, s_tasks, s_inc, sbs, tasks, inc = workload(a.wf, a.sample)
    setup_s = time.time() - t0

    eng = ReplayEngine(0)
    ld = persisted.StateLoader(eng)
    ds = ld.upload(sbs)
    ld.plan(ds)
    d_tasks, d_inc = _dev_bytes(torch, tasks, eng.dev), _dev_bytes(torch, inc, eng.dev)
    dev_ms = []
    for _ in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        br, out = ld._ndc_device(ds, d_tasks, tasks.shape[0], d_inc, inc.shape[0])
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    results = out["results"][:tasks.shape[0] * abi.NDC_RESULT.itemsize].cpu().numpy().view(abi.NDC_RESULT)
    routes = out["routes"][:tasks.shape[0] * abi.NDC_ROUTE.itemsize].cpu().numpy().view(abi.NDC_ROUTE)

    # the route without the branch table: parse on the host, pack, upload, decide -- on the sample
    exec_of = {}
    for w in sel:
        b0, nb = int(sample.wf["blob_begin"][w]), int(sample.wf["blob_count"][w])
        exec_of[int(w)] = next(b for b in range(b0, b0 + nb) if sample.blob["kind"][b] == abi.STATE_EXECUTION)
    host_s = []
    for _ in range(max(a.reps // 2, 1)):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        nts = []
        for k, w in enumerate(sel):
            cur, local = parse_version_histories(execution_field(sample.blob_bytes(exec_of[int(w)]), 122))
            o, n = int(s_tasks["incoming_begin"][k]), int(s_tasks["incoming_count"][k])
            nts.append(ndc.NdcTask(local, cur, [(int(x["event_id"]), int(x["version"])) for x in s_inc[o:o + n]],
                                   int(s_tasks["first_event_id"][k]), int(s_tasks["first_event_version"][k])))
        packed = ndc.pack(nts)
        h_res, _h_out = ndc.prepare_on_device(eng, packed)
        host_s.append(time.perf_counter() - t1)
    same = bool(all((h_res[f] == results[:sel.size][f]).all() for f in abi.NDC_RESULT.names))
    d_ms, h_s = float(np.median(dev_ms[1:])), float(np.median(host_s))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    P = br.plan
    print(json.dumps({
        "workload": f"config-3 shard shape prefix states: {sbs.n_wf} workflows tiled from {sample.n_wf} encoded ones, "
                    f"{n_second} of the sample's {sel.size} task states with a second branch, one task per such state",
        "commit": commit, "workflows": sbs.n_wf, "tasks": int(tasks.shape[0]), "branches": int(P.n_branches),
        "items": int(P.n_items), "incoming_items": int(inc.shape[0]), "out_item_room": int(P.n_out_items),
        "routes": {str(k): int(v) for k, v in enumerate(np.bincount(routes["route"], minlength=5))},
        "statuses": {str(k): int(v) for k, v in enumerate(np.bincount(results["status"])) if v},
        "device": {"plan_run_ms": d_ms, "tasks_per_s": tasks.shape[0] / d_ms * 1e3, "passes_ms": dev_ms,
                   "planning_call_syncs": 1},
        "host_parse_pack_upload_decide": {"sample_tasks": int(sel.size), "sample_ms": h_s * 1e3,
                                          "us_per_task": h_s * 1e6 / max(sel.size, 1),
                                          "scaled_linearly_to_all_tasks_ms": h_s * 1e3 * tasks.shape[0] / max(sel.size, 1),
                                          "results_equal_device": same},
        "setup_s": setup_s}), flush=True)


if __name__ == "__main__":
    main()
