"""What engine creation derives from a configuration, without a GPU, against a recording: the sweep
of tools/record_engine_layouts.py (every model, K, H, V, block size, blocks per vehicle; shards, cost
terms, a full Sigma, the state width, the three layout switches; the limits) replayed through
mppi_debug_layout must give, row by row, what tests/golden/engine_layouts.json holds -- recorded on
an MI355X from the engines of mppi_create as it was while it derived all of this in one pass behind
the device check.  The stored words are compared per row; the block and group counts, the pitch,
the output offsets, the trajectory size and the hash over DevParams and FinParams through the
recording's digests of 32 rows each (a refusal: its status and message).

The launch geometry of every row is tied to its restatement in tests/noise_stream.py here, not only
on the GPU.  For the quadrotor, geometry() returns the 16 rollouts of a dynamics wave as R, where
DevParams::R is 64 / L as for every model (k_rollout_quad does not read it): L, nch, nb and iters
are compared there."""
import json
import os
import sys

import pytest

from conftest import GOLDEN, ROOT
from noise_stream import geometry

sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_engine_layouts as R  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "engine_layouts.json")) as f:
        return R.decode(json.load(f))


@pytest.fixture(scope="module")
def replayed():
    return R.sweep()


@pytest.fixture(scope="module")
def pinned(recorded, replayed):
    """The replayed rows as {word: value} (None: refused), once their digests are the recording's:
    what the recording holds in digests only is then known row by row."""
    assert R.digests([a for _, _, a in replayed]) == recorded[1]
    return [(what, shape, None if R.refused(a) else dict(zip(R.WORDS, a))) for what, shape, a in replayed]


def test_replayed_sweep_equals_the_recording(recorded, replayed):
    rows, digests = recorded
    assert len(rows) == len(replayed) == len(list(R.sweep_rows()))
    for want, (what, _, got) in zip(rows, replayed):
        assert R.stored(got) == want, what
    got = R.digests([a for _, _, a in replayed])
    assert len(got) == len(digests)
    for i in range(0, len(got), 2):
        first = i // 2 * R.CHUNK
        assert got[i:i + 2] == digests[i:i + 2], f"rows {first}..{first + R.CHUNK - 1}, from: {replayed[first][0]}"


def test_recording_is_not_vacuous(recorded, pinned):
    rows, _ = recorded
    accepted = [(shape, w) for _, shape, w in pinned if w]
    common = [(shape, w) for shape, w in accepted if shape[0] != "quadrotor"]
    assert len(accepted) > len(rows) // 2
    assert any(w["iters"] == 1 for _, w in common) and any(w["iters"] > 1 for _, w in common)
    assert {w["iters"] for shape, w in accepted if shape[0] == "quadrotor"} == {1, 4}
    # the cost-run cap bites: fewer groups per block than the blocks asked for would give
    bites = 0
    for (_, K, _, _, _, bpv), w in common:
        per = w["threads"] // 64 * w["R"]
        groups = -(-K // per)
        cap = max(1, 4096 // ((per + 3) & ~3))
        if bpv > 0 and -(-groups // min(bpv, groups)) > cap:
            assert w["iters"] == cap and w["nb"] == -(-groups // cap)
            bites += 1
    assert bites > 0
    assert {r["chain_fast"] for r in rows if isinstance(r, dict)} == {0, 1, 2}
    assert {r["j0"] for r in rows if isinstance(r, dict)} >= {0, 1}
    assert {r["generic"] for r in rows if isinstance(r, dict)} == {0, 1, 2, 4, 8, 15}
    assert {r["fin_tsz"] for r in rows if isinstance(r, dict)} == {1, 4, 8, 16, 56}
    messages = [r[1] for r in rows if not isinstance(r, dict)]
    for part in ("supported horizons are", "too many rollout blocks", "exceeds 4 GiB", "exceed 2^31",
                 "bad SavGol window/order", "Sigma is singular"):
        assert any(part in m for m in messages), part
    assert all(r[0] == -1 for r in rows if not isinstance(r, dict))   # MPPI_ERR_INVALID_ARG, never a device error


def test_geometry_is_the_restatement(pinned):
    n = 0
    for what, (model, K, H, V, bt, bpv), w in pinned:
        if not w:
            continue
        g = geometry(model, K, H, V=V, block_threads=bt, blocks_per_vehicle=bpv)
        names = ("L", "nch", "nb", "iters") + (() if model == "quadrotor" else ("R",))
        assert {k: w[k] for k in names} == {k: g[k] for k in names}, what
        assert w["threads"] == (256 if model == "quadrotor" else g["nw"] * 64), what
        n += 1
    assert n > 4000


def test_output_offsets(pinned):
    for what, (model, _, _, V, _, _), w in pinned:
        if not w:
            continue
        A = R.MODEL_A[model]
        offs = [w["off_u0"], w["off_stats"], w["off_flags"], w["off_xerr"]]
        assert all(o % 16 == 0 for o in offs), what
        assert V * w["out_dim"] * 8 <= offs[0] and offs[0] + V * A * 4 <= offs[1], what
        assert offs[1] + V * 16 == offs[2] and offs[2] + V * (2 * A + 1) * 16 == offs[3], what
        assert 0 < offs[0] < offs[1] < offs[2] < offs[3], what
        assert w["off_xerr"] + 16 == w["out_bytes"], what
