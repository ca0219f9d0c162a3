"""The launch descriptions of every family, without a GPU, against a recording: the sweep of
tools/record_launch_descriptions.py (rollout, finalize and plan launchers over the models, horizons,
block sizes and switches) replayed through the capture diagnostics must name the same kernel and
the same launch geometry, row by row, as tests/golden/launch_descriptions.json -- recorded from the
launchers as they were while each kernel's symbol was still written out by hand.  Every recorded
symbol must be a kernel of one of the unit code objects next to the library."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT
from quadrotor_manipulator_mppi_amd import build as B

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_launch_descriptions as R  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "launch_descriptions.json")) as f:
        return R.decode(json.load(f))


@pytest.fixture(scope="module")
def replayed():
    return R.sweep()


def test_sweep_covers_what_it_should(recorded):
    assert len(recorded["rollout"]) == len(R.MODELS) * len(R.HORIZONS) * 2 * 3 * 3 * len(R.ROLL_FLAGS)
    assert len(recorded["finalize"]) == 11 * 6 * 5
    for fam in ("rollout", "finalize", "plan"):
        assert any(a != R.REFUSED for a in recorded[fam]), fam
    assert R.REFUSED in recorded["rollout"] and R.REFUSED in recorded["plan"]   # refusals are recorded as such


@pytest.mark.parametrize("family", ["rollout", "finalize", "plan"])
def test_replayed_sweep_equals_the_recording(recorded, replayed, family):
    assert len(recorded[family]) == len(replayed[family])
    for want, (args, got) in zip(recorded[family], replayed[family]):
        assert got == want, args


def _symbols(answers):
    return {lch[0] for a in answers if a != R.REFUSED for lch in a}


def test_no_answer_is_a_question_mark(recorded, replayed):
    for fam in ("rollout", "finalize", "plan"):
        for syms in (_symbols(recorded[fam]), _symbols(a for _, a in replayed[fam])):
            assert syms and all(s.startswith("_Z") and "?" not in s for s in syms)


def test_every_recorded_symbol_is_in_a_unit_code_object(recorded):
    blob = b""
    for unit in B.KERNEL_UNITS:
        with open(B.code_object_path(B.LIB, unit), "rb") as f:
            blob += f.read() + b"\0"
    for sym in sorted(set().union(*(_symbols(recorded[fam]) for fam in recorded))):
        assert (sym + ".kd").encode() in blob, sym
