"""Record the launches the step paths hand to the launchers, over a sweep (tools/, not shipped).

    python tools/record_step_launches.py [--out tests/golden/step_launches.json]

No GPU: mppi_debug_step_launches(config, switches, buf, len) builds an engine on the host from the
layout stage (device pointers null or fixed stand-in addresses, the zero state) and describes, for one
path -- mppi_run_steps or mppi_step through HIP, the native batch, the native control call -- every
launch of a step before the last and of the last step: the rollout, a shard's PACK, the finalize.
The fixture pins each launch's kernel symbol, grid, block, dynamic LDS, argument size and a 64-bit
FNV-1a digest of the argument bytes, so a change to how the paths assemble DevParams and FinParams can
be shown to hand over the same bytes (tests/test_capi_step_launches_cpu.py replays the sweep).  It
was recorded from the library as it was while rollout_impl, finalize_impl, step_params and
run_steps_aql each assembled their parameters by hand.  MPPI_HIP_LIB names the library to record
from (default: the one in the tree).

The fixture's layout: encode() below.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from quadrotor_manipulator_mppi_amd import _capi as capi  # noqa: E402
from quadrotor_manipulator_mppi_amd.engine import make_config  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "step_launches.json")
REFUSED = "refused"
SWITCHES = ("MPPI_FIN_TSZ", "MPPI_NO_KINOVA_PATH", "MPPI_GENERIC_KERNELS")   # (read by the layout stage)

# (model, fp64 state): the rows of tools/record_launch_descriptions.py MODELS
MODELS = (("drone", False), ("arm", False), ("arm", True), ("wholebody", False), ("quadrotor", False))
HORIZONS = (32, 64)
SAMPLES = 256
VEHICLES = (1, 3)
HIP_BATCH, HIP_CALL, NATIVE_BATCH, NATIVE_CALL = 0, 1, 2, 3
# (path, n steps): a batch of one step and of several, a control call
PATHS = ((HIP_BATCH, 1), (HIP_BATCH, 3), (HIP_CALL, 1), (NATIVE_BATCH, 1), (NATIVE_BATCH, 3), (NATIVE_CALL, 1))
# name -> (make_config keywords, {switch of mppi_debug_step_launches: value})
VARIANTS = {
    "plain": ({}, {}),
    "store_noise": (dict(store_noise=True), {}),
    "injected": (dict(noise="injected"), {}),
    "shard 1/2": (dict(shard_rank=1, shard_count=2), {}),
    "peer 1/2": (dict(shard_rank=1, shard_count=2), dict(peer=1)),
    "generic": ({}, dict(generic=15)),
    "timing": ({}, dict(timing=1)),
    "communicator": ({}, dict(comm=1)),
    "debug_out": ({}, dict(out_dbg=1)),
}
SW_ORDER = ("path", "n", "peer", "comm", "timing", "generic", "out_dbg")
LINE = re.compile(r"(early|last) (rollout|pack|finalize) (\S+) grid (\d+) block (\d+) lds (\d+) args (\d+) fnv ([0-9a-f]{16})")


def sweep_rows():
    """(description, make_config keywords, switches of mppi_debug_step_launches) per row, in the
    fixture's order.  INJECTED noise: the HIP paths only."""
    for (model, f64), H, V, (name, (kw, sw)), (path, n) in itertools.product(MODELS, HORIZONS, VEHICLES,
                                                                             VARIANTS.items(), PATHS):
        if name == "injected" and path in (NATIVE_BATCH, NATIVE_CALL):
            continue
        yield (f"{model}{' f64' if f64 else ''} H={H} V={V} {name} path {path} n={n}",
               dict(model=model, n_samples=SAMPLES, n_horizon=H, n_vehicles=V, state_f64=f64, **kw),
               dict(path=path, n=n, **sw))


def launches(cfg, sw):
    """mppi_debug_step_launches of a configuration: REFUSED, or a tuple of (step, kind, symbol, grid.x,
    block threads, dynamic LDS bytes, argument bytes, digest) per launch."""
    f = capi.lib().mppi_debug_step_launches
    f.restype, f.argtypes = capi.DEBUG_PROTOTYPES["mppi_debug_step_launches"]
    buf = C.create_string_buffer(4096)
    if f(C.byref(cfg), (C.c_int32 * len(SW_ORDER))(*[sw.get(k, 0) for k in SW_ORDER]), buf, len(buf)) != capi.OK:
        return REFUSED
    out = []
    for line in buf.value.decode().splitlines():
        m = LINE.fullmatch(line)
        out.append(m.group(1, 2, 3) + tuple(int(x) for x in m.group(4, 5, 6, 7)) + (m.group(8),))
    return tuple(out)


def sweep():
    """[(description, answer)] over sweep_rows()."""
    rows = []
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        for what, kw, sw in sweep_rows():
            rows.append((what, launches(make_config(**kw), sw)))
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return rows


def encode(rows):
    """The sweep as the fixture holds it.  The arguments are not stored (the sweep regenerates them,
    in order).  "symbols": the kernels' names.  "launches": every distinct launch of the sweep as
    [step, kind, symbol index, grid.x, block threads, LDS bytes, argument bytes, digest].  "rows": per
    row of the sweep its launches' indices in order, or REFUSED."""
    answers = [a for _, a in rows]
    syms = sorted({lch[2] for a in answers if a != REFUSED for lch in a})
    table = sorted({lch for a in answers if a != REFUSED for lch in a})
    at = {lch: i for i, lch in enumerate(table)}
    return {"symbols": syms,
            "launches": [[lch[0], lch[1], syms.index(lch[2])] + list(lch[3:]) for lch in table],
            "rows": [a if a == REFUSED else [at[lch] for lch in a] for a in answers]}


def decode(doc):
    """[answer per row] of a fixture, in sweep()'s form."""
    table = [(s, k, doc["symbols"][i], *rest) for s, k, i, *rest in doc["launches"]]
    return [r if r == REFUSED else tuple(table[i] for i in r) for r in doc["rows"]]


def _wrap(items, width=116):
    """JSON items, comma separated, in lines of at most `width` characters."""
    lines, cur = [], ""
    for it in (json.dumps(x, separators=(",", ":")) for x in items):
        if cur and len(cur) + len(it) + 1 > width:
            lines.append(cur + ",")
            cur = it
        else:
            cur = f"{cur},{it}" if cur else it
    return "\n".join("  " + ln for ln in lines + [cur])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    rows = sweep()
    doc = encode(rows)
    assert decode(doc) == [ans for _, ans in rows]
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": [\n{_wrap(doc[k])}\n ]' for k in ("symbols", "launches", "rows")) + "\n}\n")
    print(f"{a.out}: {len(rows)} rows ({sum(1 for _, x in rows if x == REFUSED)} refused), "
          f"{len(doc['launches'])} distinct launches, {len(doc['symbols'])} symbols")


if __name__ == "__main__":
    main()
