"""bench.py's command line (a plain run is the headline alone, --full the rest) and --dump-outputs (no GPU:
the oracle's rows stand in for the device's)."""
import os
import sys

import numpy as np

from cadence_amd import abi, synth_native
from cadence_amd import dist as cdist
from cadence_amd.flatten import interleave
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_DUMP_WORKFLOWS = bench.DUMP_WORKFLOWS


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_alone(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.headline_only and a.no_cpu_baseline and a.no_e2e
    assert _parse(monkeypatch, "--steps", "20000", "--warmup", "600").steps == 20000   # no cap: --steps is the count
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"
    assert not (a.headline_only or a.no_cpu_baseline or a.no_e2e)
    a = _parse(monkeypatch, "--full", "--headline-only", "--no-cpu-baseline")
    assert a.headline_only and a.no_cpu_baseline and not a.no_e2e


def test_f64_columns_are_exact():
    a = np.zeros(3, abi.VH_ITEM)
    a["event_id"] = [-1, 2**53 + 1, -2**63]
    a["version"] = [0, 2**63 - 1, 7]
    c = bench.as_f64_columns(a)
    assert c.dtype == np.float64 and c.shape == (3, 4)
    back = c.astype(np.int64)
    assert ((back[:, 0] | (back[:, 1] << 32)) == a["event_id"]).all()
    assert ((back[:, 2] | (back[:, 3] << 32)) == a["version"]).all()
    assert bench.as_f64_columns(np.zeros(2, abi.CHILD_ROW)).shape == (2, 4 * 2 + 3)   # `reserved` left out


def test_dump_outputs_same_rows_whatever_the_layout(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_WORKFLOWS", 300)
    canon = synth_native.mixed(1000, shard=(cdist.NUM_SHARDS, 1, 0))
    batch = interleave(canon)
    digest = np.arange(7, dtype=np.int64) - 3
    bench.dump_outputs(str(tmp_path / "a"), canon, oracle.replay(canon, 2), digest)
    bench.dump_outputs(str(tmp_path / "b"), batch, oracle.replay(batch, 2), digest)
    names = sorted(os.listdir(tmp_path / "a"))
    # every table with live rows; none for an empty one (no tasks are emitted here)
    assert names == sorted(["exec.npy", "digest.npy"] + [t[0] + ".npy" for t in abi.TABLES if t[0] != "tasks"])
    rows = 0
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and x.size and np.array_equal(x, y), f
        rows += x.shape[0]
    assert np.load(tmp_path / "a" / "exec.npy").shape[0] == 300 and rows > 1000
    # the bound of a full-size dump: the sampled exec rows and every table at its cut
    ncol = bench.as_f64_columns(np.zeros(1, abi.EXEC_ROW)).shape[1]
    assert FULL_DUMP_WORKFLOWS * ncol * 8 + len(abi.TABLES) * bench.DUMP_TABLE_BYTES + 11 * 128 <= 64_000_000
