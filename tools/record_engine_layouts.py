"""Record what engine creation derives from a configuration, over a sweep (tools/, not shipped).

    python tools/record_engine_layouts.py [--out tests/golden/engine_layouts.json] [--raw rows.json]

No GPU: mppi_debug_layout(config, out, n) runs the library's pure layout stage (csrc/mppi_layout.cpp
layout_of) and reports the integers below, with a hash over the kernels' parameter structs
(DevParams, then FinParams, device pointers null).  The fixture was recorded from the library as it
was while mppi_create still derived all of this in one pass behind the device check: there, the same
words were taken from the engine at the end of mppi_create, on the GPU.
tests/test_capi_layout_cpu.py replays the sweep.  MPPI_HIP_LIB names the library to record from
(default: the one in the tree).

The fixture's layout: encode() below.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from quadrotor_manipulator_mppi_amd import _capi as capi  # noqa: E402
from quadrotor_manipulator_mppi_amd.engine import make_config  # noqa: E402
from quadrotor_manipulator_mppi_amd.robot.urdf_chain import load_chain  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "engine_layouts.json")
# the words of mppi_debug_layout, in order
NAMED = ("threads", "L", "R", "nch", "nb", "iters", "P", "C", "hp", "fin_tsz", "fin_ts", "j0", "chain_fast",
         "sigma_diag", "nq", "qoff", "state_dim", "out_dim", "generic")
WORDS = NAMED + ("off_u0", "off_stats", "off_flags", "off_xerr", "out_bytes", "traj_floats_lo", "traj_floats_hi",
                 "hash_lo", "hash_hi")
# stored row by row; every word of every row (and a refusal's status and message) is in the chunk digests
STORED = tuple(w for w in NAMED if w not in ("nb", "iters", "hp"))
CHUNK = 32
SWITCHES = ("MPPI_FIN_TSZ", "MPPI_NO_KINOVA_PATH", "MPPI_GENERIC_KERNELS")

MODELS = ("drone", "arm", "wholebody", "quadrotor")
MODEL_A = {"drone": 3, "arm": 7, "wholebody": 10, "quadrotor": 4}
SAMPLES = (1, 16, 77, 100, 4096, 8192, 65536)
HORIZONS = (2, 20, 32, 33, 64, 65, 100, 128, 129, 193, 256)
VEHICLES = (1, 3, 64)
BLOCK_THREADS = (0, 128, 256)
BLOCKS_PER_VEHICLE = (0, 3)
ALL_COSTS = 0x1F


def _full_sigma(model):
    A = MODEL_A[model]
    return [[(0.1 + 0.05 * i) if i == j else 0.01 for j in range(A)] for i in range(A)]


def _chain(kind):
    """The shipped chain, or a variant of it that leaves the fast FK paths."""
    chain = [dict(j) for j in load_chain()]
    act = [j for j in chain if j["type"] != "fixed"]
    if kind == "tilted":          # a Kinova-shaped chain whose first origin is off the table: chain_fast 1
        act[0]["rpy"] = [0.0, 3.0, 0.0]
    elif kind == "x_axis":        # a revolute joint about x: chain_fast 0
        act[2]["axis"] = [1.0, 0.0, 0.0]
    elif kind == "prismatic":
        act[6]["type"] = "prismatic"
    elif kind == "no_fixed":      # nothing to fold: j0 = 0
        chain = act
    elif kind == "fixed_last":    # a fixed joint after the actuated ones: not nq joints in q order
        chain = chain + [{"name": "tool", "type": "fixed", "xyz": [0, 0, 0.1], "rpy": [0, 0, 0], "axis": None,
                          "q_index": -1}]
    return chain


def sweep_rows():
    """(description, make_config keywords, {switch: value}) per row, in the fixture's order.
    Trajectories are not stored in the large shapes (their size is reported either way): the
    recording creates every accepted engine on a GPU."""
    # the launch geometry: every model, K, H, V, block size and blocks per vehicle
    for H, model, bt, bpv, V, K in itertools.product(HORIZONS, MODELS, BLOCK_THREADS, BLOCKS_PER_VEHICLE, VEHICLES,
                                                     SAMPLES):
        yield (f"{model} K={K} H={H} V={V} bt={bt} bpv={bpv}",   # (H = 2 holds a 3-tap window only)
               dict(model=model, n_samples=K, n_horizon=H, n_vehicles=V, block_threads=bt, blocks_per_vehicle=bpv,
                    store_trajectory=False, savgol_window=3 if H == 2 else None), {})
    # what fills the parameter structs: shards, cost terms, a full Sigma, the state width, the switches
    switches = ({}, {"MPPI_FIN_TSZ": "4"}, {"MPPI_NO_KINOVA_PATH": "1"}, {"MPPI_GENERIC_KERNELS": "1"})
    for sw, model, H, f64, full, cost, (rank, count), V, K in itertools.product(
            switches, MODELS, (20, 64, 128), (False, True), (False, True), (0, ALL_COSTS), ((0, 1), (2, 4)), (1, 3),
            (16, 4096)):
        yield (f"{model} K={K} H={H} V={V} shard {rank}/{count} costs={cost:#x} full={full} f64={f64} {sw}",
               dict(model=model, n_samples=K, n_horizon=H, n_vehicles=V, shard_rank=rank, shard_count=count,
                    cost_terms=cost, sigma=_full_sigma(model) if full else None, state_f64=f64,
                    store_noise=bool(full), vehicle_offset=5 * rank), sw)
    # the remaining switch values, chains off the fast paths, and the limits
    for g in ("finalize", "quiet", "rollout", "quiet_rollout", "0"):
        yield (f"arm generic={g}", dict(model="arm", n_samples=256), {"MPPI_GENERIC_KERNELS": g})
    for tz in ("1", "16", "56", "57", "0"):   # (57 + 2 * 4 > 64 and 0 are ignored)
        yield (f"arm fin_tsz={tz}", dict(model="arm", n_samples=256, n_horizon=64), {"MPPI_FIN_TSZ": tz})
    for kind, model in itertools.product(("tilted", "x_axis", "prismatic", "no_fixed", "fixed_last"), ("arm", "wholebody")):
        yield f"{model} chain {kind}", dict(model=model, n_samples=64, chain=_chain(kind)), {}
    yield "arm tilted, no Kinova path", dict(model="arm", n_samples=64, chain=_chain("tilted")), {"MPPI_NO_KINOVA_PATH": "1"}
    yield "wholebody 8192 blocks", dict(model="wholebody", n_samples=131072, n_horizon=64, blocks_per_vehicle=8192,
                                        store_trajectory=False), {}
    yield "quadrotor 15625 blocks", dict(model="quadrotor", n_samples=1000000, store_trajectory=False), {}
    yield "wholebody 4 GiB trajectory", dict(model="wholebody", n_samples=200000, n_horizon=256), {}
    yield "wholebody 2^31 record floats", dict(model="wholebody", n_samples=65536, n_horizon=256, n_vehicles=256,
                                               blocks_per_vehicle=4096, store_trajectory=False), {}
    yield "arm SavGol order -1", dict(model="arm", savgol_order=-1), {}
    yield "arm singular Sigma", dict(model="arm", sigma=[0.1] * 6 + [0.0], cost_terms=ALL_COSTS), {}
    yield "arm singular Sigma, no cost terms", dict(model="arm", sigma=[0.1] * 6 + [0.0]), {}
    yield "arm stored trajectory and noise", dict(model="arm", n_samples=100, n_horizon=100, n_vehicles=3,
                                                  store_noise=True), {}
    yield "quadrotor stored trajectory", dict(model="quadrotor", n_samples=77, n_horizon=33, n_vehicles=3), {}


def layout(cfg):
    """mppi_debug_layout of a configuration: the tuple of WORDS, or (status, message) of a refusal."""
    L = capi.lib()
    L.mppi_debug_layout.restype = C.c_int32
    L.mppi_debug_layout.argtypes = [C.POINTER(capi.Config), C.POINTER(C.c_int32), C.c_int32]
    out = (C.c_int32 * len(WORDS))()
    st = L.mppi_debug_layout(C.byref(cfg), out, len(WORDS))
    return tuple(out) if st == capi.OK else (st, L.mppi_last_error().decode())


def sweep():
    """[(description, shape, answer)]: the shape is (model, K, H, V, block_threads, blocks_per_vehicle)
    of the configuration; an answer is the tuple of WORDS, or (status, message) of a refusal."""
    rows = []
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        for what, kw, sw in sweep_rows():
            os.environ.update(sw)
            cfg = make_config(**kw)
            ans = layout(cfg)
            for k in sw:
                del os.environ[k]
            rows.append((what, (kw["model"], cfg.n_samples, cfg.n_horizon, cfg.n_vehicles, cfg.block_threads,
                                cfg.blocks_per_vehicle), ans))
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    return rows


def refused(ans):
    return len(ans) == 2


def _runs(col):
    out = []
    for x in col:
        if out and out[-2] == x:
            out[-1] += 1
        else:
            out += [x, 1]
    return out


def _fnv(data, h=0xCBF29CE484222325):
    for b in data:
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def digests(answers):
    """One 64-bit FNV-1a per CHUNK consecutive rows, over every word of each row as 4 little-endian
    bytes (a refusal: its status, then its message), as [low word, high word, ...]."""
    out = []
    for i in range(0, len(answers), CHUNK):
        h = 0xCBF29CE484222325
        for ans in answers[i:i + CHUNK]:
            if refused(ans):
                h = _fnv((ans[0] & 0xFFFFFFFF).to_bytes(4, "little") + ans[1].encode(), h)
            else:
                h = _fnv(b"".join((w & 0xFFFFFFFF).to_bytes(4, "little") for w in ans), h)
        out += [h & 0xFFFFFFFF, h >> 32]
    return out


def encode(answers):
    """The sweep's answers as the fixture holds them.  The configurations are not stored (the sweep
    regenerates them, in order).  "refusals": the distinct "status|message" strings; "refused": per
    row the index of its refusal, -1 for an accepted row; "columns": the STORED words per row (a
    refused row repeats the row before it, and means nothing); each of these run-length coded over
    the rows as value, count, value, count, ...  "digests": digests() of all the words -- the block
    and group counts, the pitch, the output offsets, the trajectory size and the parameter hash
    change from row to row and are held there only."""
    msgs = sorted({f"{a[0]}|{a[1]}" for a in answers if refused(a)})
    cols = {w: [] for w in STORED}
    for a in answers:
        for w, col in cols.items():
            col.append((col[-1] if col else 0) if refused(a) else a[WORDS.index(w)])
    return {"rows": len(answers), "refusals": msgs,
            "refused": _runs([msgs.index(f"{a[0]}|{a[1]}") if refused(a) else -1 for a in answers]),
            "columns": {w: _runs(col) for w, col in cols.items()}, "digests": digests(answers)}


def _expand(runs):
    return [v for v, n in zip(runs[0::2], runs[1::2]) for _ in range(n)]


def decode(doc):
    """([per row: (status, message) of a refusal, or {word: value} of the STORED words], digests)."""
    ref = _expand(doc["refused"])
    cols = {w: _expand(doc["columns"][w]) for w in STORED}
    rows = []
    for i, r in enumerate(ref):
        if r >= 0:
            st, msg = doc["refusals"][r].split("|", 1)
            rows.append((int(st), msg))
        else:
            rows.append({w: cols[w][i] for w in STORED})
    assert len(rows) == doc["rows"]
    return rows, doc["digests"]


def stored(ans):
    """An answer of sweep() in decode()'s per-row form."""
    return ans if refused(ans) else {w: ans[WORDS.index(w)] for w in STORED}


def _wrap(items, width=116):
    """JSON items, comma separated, in lines of at most `width` characters."""
    lines, cur = [], ""
    for it in (json.dumps(x, separators=(",", ":")) for x in items):
        if cur and len(cur) + len(it) + 1 > width:
            lines.append(cur + ",")
            cur = it
        else:
            cur = f"{cur},{it}" if cur else it
    return "\n".join("   " + ln for ln in lines + [cur])


def write(doc, path):
    parts = [f' "rows": {doc["rows"]}'] + [f' "{k}": [\n{_wrap(doc[k])}\n ]' for k in ("refusals", "refused")]
    parts.append(' "columns": {\n' + ",\n".join(f'  "{c}": [\n{_wrap(r)}\n  ]' for c, r in doc["columns"].items()) + "\n }")
    parts.append(f' "digests": [\n{_wrap(doc["digests"])}\n ]')
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")


# One control step per model at its smallest shape, three vehicles, every cost term: what an engine
# computes on the GPU (tests/test_gpu_layout.py), recorded like the layouts from the library as it
# was before the split.  The kernels draw their own noise (Philox), so a case is its configuration.
STEP_FIXTURE = os.path.join(ROOT, "tests", "golden", "engine_layout_steps.json")
STEP_CASES = {"drone": dict(model="drone", n_samples=16, n_horizon=20),
              "arm": dict(model="arm", n_samples=16, n_horizon=32),
              "wholebody": dict(model="wholebody", n_samples=16, n_horizon=64),
              "quadrotor": dict(model="quadrotor", n_samples=16, n_horizon=64),
              "arm_v3": dict(model="arm", n_samples=16, n_horizon=32, n_vehicles=3),
              "arm_costs": dict(model="arm", n_samples=16, n_horizon=32, cost_terms=ALL_COSTS)}
HOME = [1.57, 1.7, 0.0, 4.4, 0.0, 4.71, 0.0]


def run_step(name):
    """(engine, {array name: value}) after one control step of STEP_CASES[name] on the GPU."""
    import numpy as np
    from quadrotor_manipulator_mppi_amd.engine import Engine
    kw = STEP_CASES[name]
    e = Engine(make_config(device=0, seed=23, **kw))
    base = {"drone": [0.0, 0.0, 1.0] + [0.0] * 3, "quadrotor": [0.0, 0.0, 1.0] + [0.0] * 9,
            "arm": [0, 0, 1, 0, 0, 0, 1] + HOME + [0.0] * 7, "wholebody": [0, 0, 1, 0, 0, 0, 1] + HOME + [0.0] * 10}
    state = np.tile(np.array(base[kw["model"]], np.float64), (e.V, 1))
    state[:, 0] += 0.01 * np.arange(e.V)
    for v in range(e.V):
        if kw["model"] in ("drone", "quadrotor"):
            e.set_target([1.0, 2.0, 3.4], vehicle=v)
        else:
            e.set_target([0.1029, 0.4055, 1.6498], [-0.5, -0.5, 0.5, -0.5], vehicle=v)
    out, u0, stats = e.step(state)
    return e, {"out": np.array(out), "u0": np.array(u0), "u_prev": e.get_u_prev(), "S": e.get_costs(),
               "stats": np.array([[s.rho, s.eta, s.ess] for s in stats], np.float32)}


def write_steps(arrays, path):
    """{"case.array": [dtype, shape, the array's bytes (little-endian, C order) in hex]}: exact."""
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": ["{v.dtype.name}", {list(v.shape)}, "{v.tobytes().hex()}"]'
                                   for k, v in arrays.items()) + "\n}\n")


def load_steps(path=STEP_FIXTURE):
    import numpy as np
    with open(path) as f:
        return {k: np.frombuffer(bytes.fromhex(h), np.dtype(dt)).reshape(shape) for k, (dt, shape, h) in json.load(f).items()}


def record_steps(path):
    arrays = {}
    for name in STEP_CASES:
        e, got = run_step(name)
        arrays.update({f"{name}.{k}": v for k, v in got.items()})
        e.close()
    write_steps(arrays, path)
    print(f"{path}: {len(STEP_CASES)} cases, {os.path.getsize(path)} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--steps", help="record the step fixture here instead (needs the GPU)")
    ap.add_argument("--raw", help="also write every row's description and answer here (JSON)")
    a = ap.parse_args()
    if a.steps:
        return record_steps(a.steps)
    rows = sweep()
    answers = [ans for _, _, ans in rows]
    doc = encode(answers)
    got, dig = decode(doc)
    assert got == [stored(x) for x in answers] and dig == digests(answers)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write(doc, a.out)
    if a.raw:
        with open(a.raw, "w") as f:
            json.dump(rows, f)
    print(f"{a.out}: {len(rows)} rows, {sum(map(refused, answers))} refused ({len(doc['refusals'])} distinct), "
          f"{os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
