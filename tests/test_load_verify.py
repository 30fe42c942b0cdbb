"""CPU: the checksum verification of loaded states, host restatement (crr_load_states_verify_host,
include/cadence_load_verify.h): what mutableStateBuilder.Load checks right after materialising a state.

Expected values are oracle/checksum_py.encode_payload + zlib.crc32 of the values the cases put into the blobs
(verify_cases.py); the device runs the same cases in test_gpu_load_verify.py.
"""
import numpy as np
import pytest

from cadence_amd import abi, persisted
from cadence_amd.persisted import load_states_verify_host, stored_checksums

import asan_tool
import load_cases as lc
import verify_cases as vc

O = abi.VerifyOutcome


def _check(name, threads=1):
    sbs, payloads = vc.batch(name)
    want = vc.expected_computed(payloads)
    loaded = np.array([p is not None for p in payloads])
    got = load_states_verify_host(sbs, vc.right_checksums(payloads), threads=threads)
    for w in range(sbs.n_wf):
        assert got["computed"][w] == want["computed"][w] and got["payload_len"][w] == want["payload_len"][w], \
            f"{name}[{w}]: {got[w]} vs crc {want['computed'][w]:#x} of {want['payload_len'][w]} bytes"
    assert (got["outcome"][loaded] == O.MATCH).all() and (got["outcome"][~loaded] == O.NOT_LOADED).all()
    assert (got["reserved"] == 0).all()
    # compute only: the same values, nothing to compare them with
    alone = load_states_verify_host(sbs)
    assert (alone["computed"] == want["computed"]).all() and (alone["payload_len"] == want["payload_len"]).all()
    assert (alone["outcome"][loaded] == O.NONE).all() and (alone["outcome"][~loaded] == O.NOT_LOADED).all()
    return sbs, got


def test_plain_state():
    sbs, got = _check("plain")
    assert sbs.n_wf == 1 and got["outcome"][0] == O.MATCH and got["computed"][0] != 0


def test_sticky_task_list_names():
    sbs, _ = _check("sticky")
    flags = persisted.load_states_host(sbs).flags
    assert (flags == [0, abi.LOAD_FLAG_STICKY, abi.LOAD_FLAG_STICKY, abi.LOAD_FLAG_STICKY]).all()


def test_branch_shapes():
    sbs, _ = _check("branches")
    img = persisted.load_states_host(sbs)
    assert (img.status == 0).all() and (img.flags & abi.LOAD_FLAG_MULTI_BRANCH != 0).sum() >= 10


def test_pending_maps_out_of_id_order():
    sbs, got = _check("pending")
    assert got["payload_len"][1] > 65 * 8


@pytest.mark.parametrize("n", vc.SIZES)
def test_mixed_variants(n):
    _check("n_%d" % n)


def test_outcome_matrix():
    sbs, payloads, stored, want = vc.outcome_matrix()
    comp = vc.expected_computed(payloads)
    got = load_states_verify_host(sbs, stored)
    assert got["outcome"].tolist() == want.tolist()
    assert (got["computed"] == comp["computed"]).all() and (got["payload_len"] == comp["payload_len"]).all()
    assert got[7].tobytes() == np.array([(0, O.NOT_LOADED, 0, 0)], abi.VERIFY_ROW).tobytes()
    # the cut-off is time.Before: a state updated exactly at it is kept, one updated before it is invalidated --
    # ahead of the version and flavor checks, behind "nothing stored" and "not loaded"
    assert load_states_verify_host(sbs, stored, invalidate_before_ns=vc.LAST_UPDATED)["outcome"].tolist() == want.tolist()
    cut = load_states_verify_host(sbs, stored, invalidate_before_ns=vc.LAST_UPDATED + 1)
    keep = (want == O.NONE) | (want == O.NOT_LOADED)
    assert (cut["outcome"][keep] == want[keep]).all() and (cut["outcome"][~keep] == O.INVALIDATED).all()
    assert cut["outcome"][4] == O.INVALIDATED and want[4] == O.BAD_VERSION
    assert (cut["computed"] == comp["computed"]).all() and (cut["payload_len"] == comp["payload_len"]).all()
    # stored=None: compute only
    alone = load_states_verify_host(sbs, None, invalidate_before_ns=vc.LAST_UPDATED + 1)
    assert (alone["outcome"][want != O.NOT_LOADED] == O.NONE).all() and alone["outcome"][7] == O.NOT_LOADED
    assert (alone["computed"] == comp["computed"]).all()


def test_stored_checksums_helper():
    s = stored_checksums([(1, 1, b"\x01\x02\x03\x04"), (2, 0, b"\x01\x02\x03"), None, (1, 1, b"")])
    assert s.dtype == abi.STORED_CHECKSUM and s.dtype.itemsize == 16 and abi.VERIFY_ROW.itemsize == 16
    assert s.tolist() == [(1, 1, 0x01020304, 4), (2, 0, 0, 3), (0, 0, 0, 0), (1, 1, 0, 0)]
    with pytest.raises(ValueError):
        load_states_verify_host(vc.batch("plain")[0], s)


def test_replayed_states():
    sbs, payloads, _ok, _s, _m, _r = vc.replayed_case()
    got = load_states_verify_host(sbs, vc.right_checksums(payloads), threads=4)
    vc.check_replayed(got)
    assert load_states_verify_host(sbs, vc.right_checksums(payloads)).tobytes() == got.tobytes()


def test_libraries_export_the_verify_entry_points_and_reject_bad_arguments():
    import ctypes
    import os
    import re
    from cadence_amd import decode, engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r"\b(crr_load_\w+)\s*\(", open(os.path.join(root, "include", "cadence_load_verify.h")).read()))
    assert declared == {"crr_load_states_verify", "crr_load_states_verify_host"}
    dev = ctypes.CDLL(engine.LIB_PATH)
    assert hasattr(dev, "crr_load_states_verify") and hasattr(decode.lib(), "crr_load_states_verify_host")
    dev.crr_abi_version.restype = ctypes.c_int
    assert dev.crr_abi_version() == abi.ABI_VERSION == 8
    abi.check_layout(dev)
    dev.crr_sizeof.restype = ctypes.c_size_t
    assert dev.crr_sizeof(20) == abi.STORED_CHECKSUM.itemsize == 16 and dev.crr_sizeof(21) == abi.VERIFY_ROW.itemsize == 16
    S = abi.CLoadSummary()
    dev.crr_load_states_verify.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2 + [ctypes.c_int64] + [ctypes.c_void_p] * 2
    assert dev.crr_load_states_verify(None, None, 0, ctypes.byref(S), None, 0, None, None) == -1
    host = persisted._host_lib()
    out = np.zeros(2, abi.VERIFY_ROW)
    assert host.crr_load_states_verify_host(None, None, 0, out.ctypes.data, 1) == -1
    sbs = persisted.build_blob_set([lc.good_workflow(0), lc.good_workflow(1)])
    c = persisted._c_batch(sbs, lambda a: a.ctypes.data)
    assert host.crr_load_states_verify_host(ctypes.byref(c), None, 0, None, 1) == -1
    sbs.wf["blob_begin"][1] += 1            # ranges that are not consecutive
    c = persisted._c_batch(sbs, lambda a: a.ctypes.data)
    assert host.crr_load_states_verify_host(ctypes.byref(c), None, 0, out.ctypes.data, 1) == -1


def test_host_restatement_under_asan_and_ubsan(tmp_path):
    assert "128 full states match, 306 truncations not loaded" in asan_tool.build_and_run(tmp_path, "load_verify_asan")
