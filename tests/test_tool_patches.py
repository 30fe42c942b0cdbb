"""CPU: the profiling tools that patch replay_kernel.hip as text still find every patch point.

tools/wave_split.py and tools/wave_prof.py build variant libraries from a copy of the kernel source with
(old, new) text pairs replaced.  An edit of the source that moves or rewords an anchor would otherwise go
unnoticed until somebody next runs the tool.  String checks only: nothing is compiled.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location("tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # both tools build only under their __main__ guard
    return mod


SOURCE = open(os.path.join(ROOT, "cadence_amd", "csrc", "replay_kernel.hip")).read()
VARIANTS = dict(_tool("wave_split").PATCHES)
VARIANTS["waveprof"] = _tool("wave_prof").PATCHES


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_anchors_occur_in_source(variant):
    """Every pair's old text occurs in the unpatched source, and replacing it changes something."""
    for old, new in VARIANTS[variant]:
        assert old in SOURCE, f"{variant}: patch point not found: {old[:70]!r}"
        assert old != new, f"{variant}: a patch that changes nothing: {old[:70]!r}"


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_patches_apply_in_order(variant):
    """The pairs applied one after another, as the tools do: an earlier replacement hides no later anchor."""
    s = SOURCE
    for old, new in VARIANTS[variant]:
        assert old in s, f"{variant}: patch point gone after the earlier patches: {old[:70]!r}"
        s = s.replace(old, new, 1)
    assert s != SOURCE
