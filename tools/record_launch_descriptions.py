"""Record what the launchers describe for a sweep of configurations (tools/, not shipped).

    python tools/record_launch_descriptions.py [--out tests/golden/launch_descriptions.json]

No GPU: the three capture diagnostics of the library (mppi_debug_rollout_kernels with
mppi_debug_rollout_launch, mppi_debug_finalize_kernels with mppi_debug_finalize_launch,
mppi_debug_plan_kernel) describe each launch instead of making it.  The fixture pins the kernel
symbol and the launch geometry of every configuration, so a change to the launch path can be
shown to describe the same launches (tests/test_capi_launch_table_cpu.py replays the sweep).
MPPI_HIP_LIB names the library to record from (default: the one in the tree).

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

FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_descriptions.json")
REFUSED = "refused"

HORIZONS = (8, 20, 32, 48, 64, 128, 200, 256)
# (model, action dimension, fp64 state): each model at its action dimension, the arm at both widths
MODELS = ((capi.MODEL_DRONE, 3, 0), (capi.MODEL_ARM, 7, 0), (capi.MODEL_ARM, 7, 1), (capi.MODEL_WHOLEBODY, 10, 0),
          (capi.MODEL_QUADROTOR, 4, 0))
# one switch at a time over the plain configuration: (noise mode, store_noise, cost_terms, full
# Sigma, peer exchange, MPPI_GENERIC_KERNELS)
ROLL_FLAGS = ((capi.NOISE_PHILOX, 0, 0, 0, 0, 0), (capi.NOISE_PHILOX, 1, 0, 0, 0, 0),
              (capi.NOISE_INJECTED, 0, 0, 0, 0, 0), (capi.NOISE_PHILOX, 0, capi.COST_CENTER, 0, 0, 0),
              (capi.NOISE_PHILOX, 0, 0, 1, 0, 0), (capi.NOISE_PHILOX, 0, 0, 0, 1, 0), (capi.NOISE_PHILOX, 0, 0, 0, 0, 1))
# finalize shapes (A, H, tsz, half, window): the four table geometries (mppi_finalize.hip FinGeo),
# then the off-table shapes of tests/test_capi_specialized_cpu.py
FIN_SHAPES = ((7, 32, 8, 4, 9), (3, 32, 8, 2, 5), (4, 32, 8, 2, 5), (10, 64, 8, 4, 9),
              (3, 20, 8, 2, 5), (7, 32, 8, 2, 5), (3, 32, 8, 4, 9), (7, 32, 16, 4, 9), (7, 64, 8, 4, 9),
              (10, 32, 8, 4, 9), (7, 32, 8, 3, 7))
FIN_NREC = (4, 128, 129, 256, 257, 4096)
# (mode, peer exchange, MPPI_GENERIC_KERNELS): FINAL, PACK, READBACK, a peer FINAL, the generic switch
FIN_FLAGS = ((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1))


def rollout_args():
    """g of mppi_debug_rollout_kernels: {model, A, H, L, nch, iters, block threads, V, state_f64,
    noise mode, store_noise, cost_terms, full Sigma, peer exchange, MPPI_GENERIC_KERNELS}."""
    for (model, A, f64), H, V, iters, threads, fl in itertools.product(MODELS, HORIZONS, (1, 3), (1, 2, 4),
                                                                        (128, 256, 512), ROLL_FLAGS):
        yield (model, A, H, 32 if H <= 32 else 64, (H + 63) // 64, iters, threads, V, f64) + fl


def finalize_args():
    """g of mppi_debug_finalize_kernels: {A, H, tsz, half, ts, window, nrec, mode, peer exchange,
    MPPI_GENERIC_KERNELS}."""
    for (A, H, tsz, half, window), nrec, fl in itertools.product(FIN_SHAPES, FIN_NREC, FIN_FLAGS):
        yield (A, H, tsz, half, (H + tsz - 1) // tsz, window, nrec) + fl


def plan_args():
    """g of mppi_debug_plan_kernel: {model, A, H, V, state_f64, quad_literal_jinv}; then the
    shapes the launcher has no kernel for."""
    for (model, A, f64), H, V in itertools.product(MODELS, HORIZONS, (1, 3)):
        for lit in ((0, 1) if model == capi.MODEL_QUADROTOR else (0,)):
            yield (model, A, H, V, f64, lit)
    yield from ((capi.MODEL_ARM, 6, 32, 1, 0, 0), (capi.MODEL_DRONE, 3, 257, 1, 0, 0), (capi.MODEL_DRONE, 3, 0, 1, 0, 0))


def _pair(L, kernels, launch, g):
    """((full symbol, block, grid.x, lds), (quiet symbol, ...)) of a two-launch diagnostic, or REFUSED."""
    full, quiet, geo = C.create_string_buffer(192), C.create_string_buffer(192), (C.c_int32 * 6)()
    if kernels((C.c_int32 * len(g))(*g), full, quiet, 192) != 0:
        return REFUSED
    launch(geo)
    return (full.value.decode(), *geo[0:3]), (quiet.value.decode(), *geo[3:6])


def _bind(L):
    for name in ("mppi_debug_rollout_kernels", "mppi_debug_finalize_kernels"):
        f = getattr(L, name)
        f.restype, f.argtypes = C.c_int32, [C.POINTER(C.c_int32), C.c_char_p, C.c_char_p, C.c_int32]
    for name in ("mppi_debug_rollout_launch", "mppi_debug_finalize_launch"):
        f = getattr(L, name)
        f.restype, f.argtypes = None, [C.POINTER(C.c_int32)]
    L.mppi_debug_plan_kernel.restype = C.c_int32
    L.mppi_debug_plan_kernel.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_int32]


def sweep():
    """{family: [(arguments, answer)]}: an answer is REFUSED or a tuple of (symbol, block threads,
    grid.x, dynamic LDS bytes) per described launch (the plan's has no LDS figure)."""
    L = capi.lib()
    _bind(L)
    out = {"rollout": [(g, _pair(L, L.mppi_debug_rollout_kernels, L.mppi_debug_rollout_launch, g))
                       for g in rollout_args()],
           "finalize": [(g, _pair(L, L.mppi_debug_finalize_kernels, L.mppi_debug_finalize_launch, g))
                        for g in finalize_args()],
           "plan": []}
    buf = C.create_string_buffer(256)
    for g in plan_args():
        if L.mppi_debug_plan_kernel((C.c_int32 * 6)(*g), buf, 256) != 0:
            out["plan"].append((g, REFUSED))
            continue
        m = re.fullmatch(r"(\S+) grid (\d+) block (\d+)", buf.value.decode())
        out["plan"].append((g, ((m.group(1), int(m.group(3)), int(m.group(2))),)))
    return out


COLUMNS = ("symbol", "block", "grid", "lds")


def _runs(col):
    out = []
    for x in col:
        if out and out[-2] == x:
            out[-1] += 1
        else:
            out += [x, 1]
    return out


def encode(sw):
    """The sweep as the fixture holds it.  The arguments are not stored (the sweep regenerates them,
    in order).  A symbol is its head and the index of its parameter list ("signatures").  Each
    family is stored by column -- per described launch (two, the plan one): symbol index, block
    threads, grid.x and (not the plan) dynamic LDS bytes -- and each column run-length coded over
    the sweep's rows as value, count, value, count, ...; a refused row is -1 in every column."""
    names = sorted({lch[0] for rows in sw.values() for _, ans in rows if ans != REFUSED for lch in ans})
    sigs = sorted({n[n.index("Ev") + 1:] for n in names})
    doc = {"signatures": sigs, "symbols": [f"{n[:n.index('Ev') + 1]}|{sigs.index(n[n.index('Ev') + 1:])}" for n in names]}
    for fam, rows in sw.items():
        n_l, w = (1, 3) if fam == "plan" else (2, 4)
        flat = [[-1] * (n_l * w) if ans == REFUSED else [x for lch in ans for x in (names.index(lch[0]),) + tuple(lch[1:])]
                for _, ans in rows]
        doc[fam] = {f"{COLUMNS[c % w]}{c // w}": _runs([r[c] for r in flat]) for c in range(n_l * w)}
    return doc


def decode(doc):
    """{family: [answer per row]} of a fixture, in sweep()'s form."""
    names = [h + doc["signatures"][int(k)] for h, k in (s.split("|") for s in doc["symbols"])]
    out = {}
    for fam in ("rollout", "finalize", "plan"):
        n_l, w = (1, 3) if fam == "plan" else (2, 4)
        cols = [[v for v, n in zip(r[0::2], r[1::2]) for _ in range(n)]
                for r in (doc[fam][f"{COLUMNS[c % w]}{c // w}"] for c in range(n_l * w))]
        out[fam] = [REFUSED if r[0] < 0 else tuple((names[r[i]],) + r[i + 1:i + w] for i in range(0, n_l * w, w))
                    for r in zip(*cols)]
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    sw = sweep()
    doc = encode(sw)
    assert decode(doc) == {fam: [ans for _, ans in rows] for fam, rows in sw.items()}
    parts = [f' "{k}": [\n{_wrap(doc[k])}\n ]' for k in ("signatures", "symbols")]
    parts += [f' "{k}": {{\n' + ",\n".join(f'  "{c}": [\n{_wrap(r)}\n  ]' for c, r in doc[k].items()) + "\n }" for k in sw]
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")
    print(f"{a.out}: {len(doc['symbols'])} symbols; " +
          ", ".join(f"{len(rows)} {k} ({sum(1 for _, x in rows if x == REFUSED)} refused)" for k, rows in sw.items()))


if __name__ == "__main__":
    main()
