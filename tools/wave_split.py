"""Profiling aid (not product code): where the wavefront path's time goes, by removing one part at a
time.  Builds variant libraries from patched copies of replay_kernel.hip (results are wrong by design;
only the kernel times are read, tools/prof_longtail.py --lib):

    python tools/wave_split.py noepi nowalk bare      ->  tools/variants/<name>.so

  noepi   the batch epilogue (timer re-selection) skipped
  nowalk  fast chunks visit nothing (only the lane-parallel passes run)
  bare    no chunk is walked or resolved (chunk loads, the VH prologue and the chunk bookkeeping only)
  nosort  GlobalTables::finalize without its selection sorts (passive replication, tools/prof_replication.py)
  nofinread  compact tiers' finalize building an activity row without re-reading its scheduled / started events
  rload   resumed compact workflows stopping after the arena load (tools/prof_replication.py --lib)

A patch anchors on source text; tests/test_tool_patches.py fails when an anchor stops matching.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PATCHES = {
    "noepi": [("          T.epilogue(L, G, K);  // :634-640 GenerateActivityTimerTasks / GenerateUserTimerTasks\n"
               "          if (!fast) {",
               "          if (0) T.epilogue(L, G, K);\n          if (!fast) {")],
    "nowalk": [("        vm = (OPS | EB) & le(stop - 1);", "        vm = 0;")],
    "bare": [("      u64 vm = le(lim - 1), OPS = 0;", "      u64 vm = 0, OPS = 0;"),
             ("      const bool fast = !K.on &&", "      const bool fast = false && !K.on &&")],
    # lane path over HBM rows (resume / wide segment): finalize without the in-place selection sorts
    "nosort": [("    for (i32 i = 0; i < n; ++i) {\n      i32 best = -1;\n      i64 bid = 0;",
                "    for (i32 i = 0; i < 0 * n; ++i) {\n      i32 best = -1;\n      i64 bid = 0;")],
    # compact tiers (config 3 traffic attribution): finalize building a new activity row without re-reading its
    # scheduled / started events
    "nofinread": [("      const crr_activity_side as = in->act_side[in->ev.aux[ix(ss)]];\n      crr_activity_row r;",
                   "      crr_activity_side as{}; as.schedule_to_start = 1; as.schedule_to_close = 2; as.start_to_close = 3;\n"
                   "      crr_activity_row r;"),
                  ("      r.scheduled_time = ev_ts(ss);\n", "      r.scheduled_time = (i64)ss;\n"),
                  ("      r.started_time = started ? ev_ts(st) : CRR_ZERO_TIME;\n",
                   "      r.started_time = started ? (i64)st : CRR_ZERO_TIME;\n")],
    # passive replication in the compact tiers (CompactTables<TIER, true>), tools/prof_replication.py --lib:
    # resumed compact workflows stopping early (the exec row written back as loaded) after the arena load
    "rload": [("      if (L.status != CRR_OK) goto done_events;  // a loaded state the policy cannot hold: general path\n",
               "      if (L.status != CRR_OK) goto done_events;  // a loaded state the policy cannot hold: general path\n"
               "      if constexpr (FusedMapOps<P>::value) { out.exec[w] = X; return; }\n")],
}


def main():
    for name in sys.argv[1:]:
        s = open(os.path.join(ROOT, "cadence_amd", "csrc", "replay_kernel.hip")).read()
        for old, new in PATCHES[name]:
            if old not in s:
                raise SystemExit(f"{name}: patch point not found: {old[:60]!r}")
            s = s.replace(old, new, 1)
        d = tempfile.mkdtemp()
        p = os.path.join(d, "replay_kernel.hip")
        open(p, "w").write(s)
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "build_variant.py"), name, "--src=" + p], check=True)


if __name__ == "__main__":
    main()
