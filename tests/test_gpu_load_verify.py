"""GPU: the checksum verification of loaded states on the device (crr_load_states_verify,
include/cadence_load_verify.h): load_verify_kernel's result array equals the host restatement's byte for byte and
the independent expectation (verify_cases.py) directly; it neither depends on nor disturbs the loaded image.
"""
import numpy as np
import pytest

from cadence_amd import abi
from cadence_amd.persisted import StateLoader, load_states_host, load_states_verify_host

import verify_cases as vc

pytestmark = pytest.mark.gpu
O = abi.VerifyOutcome


@pytest.fixture(scope="module")
def engine():
    from cadence_amd.engine import ReplayEngine
    return ReplayEngine(0)


@pytest.fixture(scope="module")
def loader(engine):
    return StateLoader(engine)


def _both(loader, sbs, stored=None, cut=0, scratch_bytes=None):
    ds = loader.upload(sbs)
    loader.plan(ds, scratch_bytes)
    dev = loader.verify(ds, stored, cut)
    host = load_states_verify_host(sbs, stored, cut)
    assert dev.dtype == abi.VERIFY_ROW and dev.shape == (sbs.n_wf,)
    bad = np.nonzero(dev != host)[0]
    assert dev.tobytes() == host.tobytes(), f"workflows {bad[:5]}: device {dev[bad[:5]]} vs host {host[bad[:5]]}"
    return dev


@pytest.mark.parametrize("name", vc.BATCHES + ["n_%d" % n for n in vc.SIZES])
def test_device_equals_host_and_the_expectation(loader, name):
    sbs, payloads = vc.batch(name)
    want = vc.expected_computed(payloads)
    loaded = np.array([p is not None for p in payloads])
    got = _both(loader, sbs, vc.right_checksums(payloads))
    assert (got["computed"] == want["computed"]).all() and (got["payload_len"] == want["payload_len"]).all()
    assert (got["outcome"][loaded] == O.MATCH).all() and (got["outcome"][~loaded] == O.NOT_LOADED).all()
    alone = _both(loader, sbs)   # compute only
    assert (alone["computed"] == want["computed"]).all() and (alone["outcome"][loaded] == O.NONE).all()


def test_outcome_matrix_on_the_device(loader):
    sbs, payloads, stored, want = vc.outcome_matrix()
    assert _both(loader, sbs, stored)["outcome"].tolist() == want.tolist()
    assert _both(loader, sbs, stored, vc.LAST_UPDATED)["outcome"].tolist() == want.tolist()
    cut = _both(loader, sbs, stored, vc.LAST_UPDATED + 1)
    keep = (want == O.NONE) | (want == O.NOT_LOADED)
    assert (cut["outcome"][keep] == want[keep]).all() and (cut["outcome"][~keep] == O.INVALIDATED).all()
    assert (cut["computed"] == vc.expected_computed(payloads)["computed"]).all()
    alone = _both(loader, sbs, None, vc.LAST_UPDATED + 1)
    assert (alone["outcome"][want != O.NOT_LOADED] == O.NONE).all()
    assert alone[7].tobytes() == cut[7].tobytes() == np.array([(0, O.NOT_LOADED, 0, 0)], abi.VERIFY_ROW).tobytes()


def test_replayed_states_before_and_after_read_and_place(engine, loader):
    import dataclasses
    from cadence_amd.flatten import flatten, interleave
    import load_cases as lc
    from resume_cases import KNOWN
    sbs, payloads, _ok, _s, _m, _r = vc.replayed_case()
    stored = vc.right_checksums(payloads)
    host = load_states_verify_host(sbs, stored, threads=4)
    ds = loader.upload(sbs)
    loader.plan(ds)
    before = loader.verify(ds, stored)
    assert before.tobytes() == host.tobytes()
    vc.check_replayed(before)
    img = loader.read()
    _hs, _pre, suf, mask, _pre_b, _pre_r = lc.prefix_case(3000, 61)
    suf_b = interleave(flatten(suf, known_domains=KNOWN, loaded=img.resumable(mask)))
    db = engine.upload(dataclasses.replace(suf_b, init=None), live_ids=True)
    loader.place(db, perm=suf_b.perm)
    after = loader.verify(ds, stored)
    assert after.tobytes() == host.tobytes()
    vc.check_replayed(after)
    # the image is what it was
    host_img, dev_img = load_states_host(sbs, threads=4), loader.read()
    h, d = host_img.image_bytes(), dev_img.image_bytes()
    for k in h:
        assert d[k] == h[k], k
    assert dev_img.err_blob == host_img.err_blob


def test_verify_after_a_plan_that_grew_its_scratch(loader):
    sbs, payloads, _ok, _s, _m, _r = vc.replayed_case()
    stored = vc.right_checksums(payloads)
    loader.plan(loader.upload(sbs))
    short = int(loader.summary.scratch_needed) - 64
    got = _both(loader, sbs, stored, scratch_bytes=short)
    assert loader.grown == short + 64
    vc.check_replayed(got)
