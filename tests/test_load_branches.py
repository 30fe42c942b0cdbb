"""Every branch of every persisted state, extracted by the host restatement (crr_load_branches_host,
include/cadence_load_ndc.h), against the values the test wrote: branches, items, tokens and current indices of
200 replayed states with random branch sets and of hand-built ones (absent Items, absent tokens), and nothing
for the states that do not load.  ``encode_states(branches=...)`` is additive: without it the bytes are as before.
A stand-alone program runs the same extraction under AddressSanitizer / UndefinedBehaviorSanitizer.
"""
import numpy as np

from cadence_amd import abi, persisted
from cadence_amd.persisted import load_branches_host, load_states_host

import asan_tool
import load_cases as lc
import ndc_load_cases as nc


def test_host_extraction_returns_exactly_what_was_written():
    sbs, want = nc.replayed_branch_states()
    assert sbs.n_wf == len(want) >= 206   # 200 histories (their new-run histories beside them) + 6 hand-built
    br = load_branches_host(sbs)
    got = nc.table_of(sbs, br)
    n_none = sum(w is None for w in want)
    assert 3 <= n_none < 60
    assert any(w is not None and w[0] != 0 for w in want)
    for w, (g, e) in enumerate(zip(got, want)):
        assert g == e, f"workflow {w}: {g} vs {e}"
    # the table's shape: consecutive item ranges in stored order, totals as counted
    loaded = np.array([w is not None for w in want])
    assert (load_states_host(sbs).status[loaded] == 0).all() and (load_states_host(sbs).status[~loaded] != 0).all()
    assert int(br.branch_begin[-1]) == br.branches.shape[0] == br.tokens.shape[0] == sum(len(w[1]) for w in want if w)
    assert br.items.shape[0] == int(br.branches["item_count"].sum())
    begin = np.cumsum(br.branches["item_count"].astype(np.int64)) - br.branches["item_count"]
    assert (br.branches["item_begin"] == begin).all()
    assert load_branches_host(sbs, threads=4).image_bytes() == br.image_bytes()


def test_the_three_states_that_do_not_load_have_no_branches():
    sbs, want = nc.replayed_branch_states()
    st = load_states_host(sbs).status
    br = load_branches_host(sbs)
    seen = set()
    for w, e in enumerate(want):
        if e is None and sbs.wf["blob_count"][w]:
            seen.add(int(st[w]))
            assert br.branch_begin[w] == br.branch_begin[w + 1] and br.current[w] == 0
    assert {abi.LoadStatus.MALFORMED, abi.LoadStatus.VERSION_HISTORIES, abi.LoadStatus.EXECUTION_COUNT} <= seen


def test_empty_batch_has_an_empty_table():
    br = load_branches_host(persisted.build_blob_set([]))
    assert br.branch_begin.tolist() == [0] and br.branches.size == br.items.size == br.tokens.size == br.current.size == 0


def test_branches_argument_is_additive():
    _hs, pre, _suf, _mask, pre_b, pre_r = lc.prefix_case(200, 71)
    a = persisted.encode_states(pre_b, pre_r, pre, shuffle_seed=4, multi_branch=range(0, 200, 9))
    b = persisted.encode_states(pre_b, pre_r, pre, shuffle_seed=4, multi_branch=range(0, 200, 9), branches={})
    c = persisted.encode_states(pre_b, pre_r, pre, shuffle_seed=4, multi_branch=range(0, 200, 9), branches=[None] * 200)
    for f in ("bytes", "blob_off", "blob", "wf", "strings"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes() == getattr(c, f).tobytes(), f
    # an entry that is None stands for the state's own branch: [own] at index 0 is the default output again
    ok = np.nonzero(pre_r.to_loaded(pre_b).mask)[0]
    plain = persisted.encode_states(pre_b, pre_r, pre)
    own = persisted.encode_states(pre_b, pre_r, pre, branches={int(w): ([None], 0) for w in ok})
    assert own.bytes.tobytes() == plain.bytes.tobytes()
    # and a second branch behind it shows up in the table, the own branch unchanged in front
    two = persisted.encode_states(pre_b, pre_r, pre, branches={int(ok[0]): ([None, (b"other", [(1, 0)])], 0)})
    t_plain, t_two = nc.table_of(plain, load_branches_host(plain)), nc.table_of(two, load_branches_host(two))
    assert t_two[ok[0]] == (0, t_plain[ok[0]][1] + [([(1, 0)], b"other")])
    assert t_two[ok[1]] == t_plain[ok[1]]
    # encode_version_histories leaves out what is None, as the test's own writer does
    hs = [(None, [(1, 2)]), (b"t", None)]
    assert persisted.encode_version_histories(1, hs) == nc.version_histories_blob(1, hs)


def test_host_extraction_under_asan_and_ubsan(tmp_path):
    asan_tool.build_and_run(tmp_path, "load_branches_asan")
