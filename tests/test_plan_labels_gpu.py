"""The op labels of the engine's plans are pinned: tests/golden/plan_labels.json holds, per case, the ordered list of labels that
Engine.profile_unet / profile_vae / profile_vocoder report (tools/make_plan_labels.py: large UNet config, synthetic weights, default switches).
A label carries the op, its shape and the kernel family the planner picked, so a refactor of the dispatch code must leave every list as it is,
and a change of a routing threshold shows here as exactly the ops that flipped (regenerate the fixture with the tool when that is intended)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_plan_labels", os.path.join(ROOT, "tools", "make_plan_labels.py"))
make_plan_labels = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(make_plan_labels)

with open(os.path.join(ROOT, "tests", "golden", "plan_labels.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_the_cases():
    assert list(GOLDEN) == list(make_plan_labels.CASES)
    assert all(len(v) > 50 for v in GOLDEN.values())


@pytest.fixture(scope="module")
def labels(lib):
    return make_plan_labels.collect()


@pytest.mark.parametrize("case", list(make_plan_labels.CASES))
def test_plan_labels_are_unchanged(labels, case):
    got, want = labels[case], GOLDEN[case]
    flipped = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert len(got) == len(want) and not flipped, "%s: %d ops (fixture %d); first differences (index, fixture, now): %s" % (
        case, len(got), len(want), flipped[:8])
