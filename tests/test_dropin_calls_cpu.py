"""What the drop-in solver classes ask of their engine, without a GPU, against a recording: the
scenarios of tools/record_dropin_calls.py (the arm class through an fp32 state, a changed target, an
fp64 state and injected noise; the drone and the quadrotor class through a changed target, a kept
one and a larger n_samples with injected noise; all with a prewarm window) replayed on a stub engine must
make, event for event, the calls tests/golden/dropin_calls.json holds -- create (the real
make_config's bytes), close, get_u_prev, set_u_prev, set_prewarm, set_target, step with their
arguments -- and hand back the same values, ``u`` and public surface after every control call.
Recorded while each of the three classes carried its own engine lifecycle, warm start and target
write."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_dropin_calls as R  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "dropin_calls.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed():
    return json.loads(json.dumps(R.record()))


@pytest.mark.parametrize("cls", ["arm", "drone", "quadrotor"])
def test_replayed_scenario_equals_the_recording(recorded, replayed, cls):
    want, got = recorded[cls], replayed[cls]
    for i, (w, g) in enumerate(zip(want, got)):
        assert g == w, f"{cls} event {i}"
    assert len(got) == len(want)


def test_recording_is_not_vacuous(recorded):
    assert sorted(recorded) == ["arm", "drone", "quadrotor"]
    for cls, log in recorded.items():
        names = [e[0] for e in log]
        creates = [i for i, n in enumerate(names) if n == "create"]
        # the arm: fp32, fp64, injected; the others: philox, (injected, 64 samples)
        assert len(creates) == (3 if cls == "arm" else 2), cls
        assert len({log[i][1] for i in creates}) == len(creates), cls           # a new config each time
        for k, i in enumerate(creates):   # read the old warm start, close, create, warm start, prewarm, target, step
            assert names[i + 1:i + 5] == ["set_u_prev", "set_prewarm", "set_target", "step"], (cls, i)
            assert names[i - 2:i] == ["get_u_prev", "close"] if k else "close" not in names[:i], (cls, i)
        steps = [i for i, n in enumerate(names) if n == "step"]
        assert len(steps) == names.count("returned") == 4, cls
        # the target: once per engine and once more where the scenario changes it on a live engine,
        # and not with the call that follows with the target as it was
        assert names.count("set_target") == len(creates) + (0 if cls == "arm" else 1), cls
        assert names[steps[1] - 1] != "set_target" if cls == "arm" else names[steps[2] - 1] != "set_target", cls
        # last_stats appears with the first call and param_gamma is the drone's alone
        faces = [e[1] for e in log if e[0] == "surface"]
        assert "last_stats" not in faces[0] and all("last_stats" in f for f in faces[1:]), cls
        assert all(("param_gamma" in f) == (cls == "drone") for f in faces), cls
        assert all(("params" in f) == (cls == "quadrotor") for f in faces), cls
        # the arm returns copies in the state's dtype, the others two views of one tensor
        rets = [e for e in log if e[0] == "returned"]
        assert all(e[3] == (cls != "arm") and e[4] == "" for e in rets), cls
        if cls == "arm":
            assert [e[1][0] for e in rets] == ["float32", "float32", "float64", "float64"]
            assert log[-1] == ["cnt", 4]
        else:
            assert {tuple(e[1][1]) for e in rets} == {(3,) if cls == "drone" else (6,)}
