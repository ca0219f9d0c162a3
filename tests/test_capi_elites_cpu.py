"""The elite readback (mppi_get_elites, csrc/mppi_elites.hip), CPU side: the header declares the
entry point and the library exports it at ABI 10, the unit has its own gfx950 code object, the
launcher -- described into a capture target, without a GPU (mppi_debug_elite_kernel) -- names
kernels that code object holds at in-bounds geometry, the order of the elites (its host twin over
the kernels' own key function, mppi_debug_elite_order) is numpy's stable argsort in every corner,
and distributed.merge_elites merges shards' elites into the unsplit array's.  The GPU side is
tests/test_gpu_elites.py."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from conftest import ROOT
from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B
from quadrotor_manipulator_mppi_amd.distributed import merge_elites
from quadrotor_manipulator_mppi_amd.engine import Elites

DRONE, ARM, WB, QUAD = capi.MODEL_DRONE, capi.MODEL_ARM, capi.MODEL_WHOLEBODY, capi.MODEL_QUADROTOR
UNIT = "mppi_elites.hip"
S_A = 4096   # samples of one stage-A block (csrc/mppi_elites.h kEliteShare)


def _code_object():
    assert UNIT in B.KERNEL_UNITS
    path = B.code_object_path(B.LIB, UNIT)
    assert os.path.exists(path), f"{path} missing (python -m quadrotor_manipulator_mppi_amd.build)"
    return path


def test_header_declares_and_library_exports_get_elites():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mppi_hip.h")).read(), flags=re.S)
    assert re.search(r"mppi_status\s+mppi_get_elites\s*\(\s*mppi_engine\s*\*\s*e\s*,\s*int32_t\s+n\s*,\s*int32_t\s*\*\s*idx\s*,"
                     r"\s*float\s*\*\s*S\s*,\s*float\s*\*\s*w\s*,\s*float\s*\*\s*traj\s*\)\s*;", src)
    assert re.search(r"#define\s+MPPI_MAX_ELITES\s+64\b", src)
    assert "#define MPPI_ABI_VERSION 10" in src
    L = capi.lib()
    assert hasattr(L, "mppi_get_elites") and "mppi_get_elites" in capi.PROTOTYPES
    assert L.mppi_abi_version() == 10 and capi.ABI_VERSION == 10 and capi.MAX_ELITES == 64


def test_elites_unit_has_a_gfx950_code_object():
    with open(_code_object(), "rb") as f:
        head = f.read(64)
    assert head[:4] == b"\x7fELF"
    (e_machine,) = struct.unpack_from("<H", head, 18)
    assert e_machine == 224   # EM_AMDGPU
    (flags,) = struct.unpack_from("<I", head, 48)
    assert flags & 0xFF == 0x4F, f"not gfx950 (mach {flags & 0xFF:#x})"


def _elite_kernel(model, K, H, V, n):
    f = capi.lib().mppi_debug_elite_kernel
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_int32]
    buf = C.create_string_buffer(1024)
    rc = f((C.c_int32 * 5)(model, K, H, V, n), buf, 1024)
    if rc != 0:
        return None
    out = []
    for one in buf.value.decode().split("; "):
        m = re.fullmatch(r"(\S+) grid (\d+)x(\d+) block (\d+)", one)
        assert m, buf.value
        out.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return out


@pytest.mark.parametrize("model,H", [(DRONE, 20), (ARM, 32), (WB, 64), (QUAD, 32)])
def test_elite_launch_symbols_and_geometry(model, H):
    """Every launch's symbol is in the unit's code object, the first grid is B x V with B the
    stage-A blocks (1 while K fits one block's share), the selection that sorts is one block per
    vehicle, the gather one block per elite and vehicle, and no block exceeds 1024 threads."""
    with open(_code_object(), "rb") as f:
        blob = f.read()
    for K in (1, 32, 100, 4096, 5000, 65536):
        for V in (1, 3, 64):
            for n in (1, 7, 64):
                if n > K:
                    assert _elite_kernel(model, K, H, V, n) is None
                    continue
                launches = _elite_kernel(model, K, H, V, n)
                assert launches, (model, K, V, n)
                Bk = (K + S_A - 1) // S_A
                assert len(launches) == (3 if Bk > 1 else 2)
                for sym, gx, gy, block in launches:
                    assert (sym + ".kd").encode() in blob, f"{sym}.kd not in the elites unit's code object"
                    assert "k_elite" in sym and gy == V and 64 <= block <= 1024 and block % 64 == 0
                assert launches[0][1] == Bk
                assert launches[-2][1] == 1 and "k_elite_select" in launches[-2][0]
                assert launches[-1][1] == n and "k_elite_gather" in launches[-1][0]


def test_elite_launcher_refuses_what_it_has_no_kernel_for():
    for model, K, H, V, n in [(ARM, 64, 32, 1, 0), (ARM, 128, 32, 1, 65), (ARM, 32, 32, 1, 33), (ARM, 0, 32, 1, 1),
                              (DRONE, 64, 20, 0, 4), (DRONE, 64, 0, 1, 4), (DRONE, 64, 20, 1, -1)]:
        assert _elite_kernel(model, K, H, V, n) is None, (model, K, H, V, n)


# ---------------------------------------------------------------- the order (host twin of the key)
def _order(S, n):
    S = np.ascontiguousarray(S, np.float32)
    f = capi.lib().mppi_debug_elite_order
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    idx = np.full(n, -7, np.int32)
    assert f(capi.fptr(S), S.size, n, idx.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    return idx


def _ref(S, n):
    with np.errstate(invalid="ignore"):   # (a signalling NaN in the sum)
        return np.argsort(np.asarray(S, np.float32) + np.float32(0.0), kind="stable")[:n]   # (-0 -> +0)


def _check(S):
    K = len(S)
    for n in sorted({1, min(K, 7), min(K, 64)}):
        np.testing.assert_array_equal(_order(S, n), _ref(S, n), err_msg=f"K={K} n={n}")


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 100, 4097])
def test_order_random_costs(K):
    _check(np.random.default_rng(K).uniform(0.0, 50.0, K).astype(np.float32))


def test_order_ties():
    for K in (1, 64, 100):
        S = np.full(K, 3.25, np.float32)   # all equal: 0 .. n-1
        for n in sorted({1, min(K, 7), min(K, 64)}):
            np.testing.assert_array_equal(_order(S, n), np.arange(n))
    S = np.random.default_rng(1).choice(np.array([1.0, 2.0, 4.0], np.float32), 300)   # ties span past n
    _check(S)


def test_order_is_decided_by_each_byte_of_the_cost():
    rng = np.random.default_rng(2)
    base = np.float32(17.5).view(np.uint32)
    low = (base & np.uint32(0xFFFFFF00)) | rng.integers(0, 256, 500).astype(np.uint32)   # the low byte alone differs
    _check(low.view(np.float32))
    high = (rng.integers(0x10, 0x7F, 500).astype(np.uint32) << 24) | np.uint32(0x00345678)  # the top byte alone
    _check(high.view(np.float32))
    for shift in (8, 16):   # and the middle bytes
        mid = (base & ~np.uint32(0xFF << shift)) | (rng.integers(0, 256, 500).astype(np.uint32) << shift)
        _check(mid.view(np.float32))


def test_order_non_finite_and_signed_zero():
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FC12345], np.uint32).view(np.float32)
    S = np.concatenate([np.array([5.0, np.inf, -0.0, 0.0, 2.0, -np.inf, 1e-45, -1e-45], np.float32), nans,
                        np.array([0.0, -0.0, np.inf, 3.0], np.float32)])
    assert np.isnan(S).sum() == 5
    for n in range(1, len(S) + 1):
        np.testing.assert_array_equal(_order(S, n), _ref(S, n), err_msg=f"n={n}")
    rng = np.random.default_rng(3)
    S = rng.uniform(0, 1, 200).astype(np.float32)
    S[rng.choice(200, 40, replace=False)] = np.nan
    S[rng.choice(200, 20, replace=False)] = np.inf
    S[::7] = -0.0
    S[3::11] = 0.0
    for n in (1, 64, 150, 200):
        np.testing.assert_array_equal(_order(S, n), _ref(S, n))


def test_order_negative_costs():
    S = np.random.default_rng(4).normal(0.0, 100.0, 1000).astype(np.float32)
    assert (S < 0).sum() > 100
    _check(S)
    _check(-np.abs(S))


def test_order_rejects_bad_arguments():
    f = capi.lib().mppi_debug_elite_order
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_float), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    S = np.zeros(4, np.float32)
    idx = np.zeros(8, np.int32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    assert f(capi.fptr(S), 4, 0, ip) != 0 and f(capi.fptr(S), 4, 5, ip) != 0 and f(capi.fptr(S), 0, 1, ip) != 0


# ------------------------------------------------------------------------------ merge_elites
def _numpy_elites(S, rows, n, offset=0):
    """A shard's elites as the engine would return them for one vehicle (V = 1), indices global."""
    o = _ref(S, n)
    return Elites((o + offset)[None].astype(np.int64), S[o][None], np.zeros((1, n), np.float32), rows[o][None], None)


@pytest.mark.parametrize("G", [1, 2, 8])
def test_merge_elites_equals_the_unsplit_selection(G):
    rng = np.random.default_rng(10 + G)
    K, n = 64 * G, 16
    S = rng.uniform(0, 10, K).astype(np.float32)
    S[rng.choice(K, K // 4, replace=False)] = np.float32(2.5)   # ties within and across shards
    S[5] = np.nan
    rows = rng.normal(size=(K, 4, 3)).astype(np.float32)
    Ks = K // G
    parts = [_numpy_elites(S[g * Ks:(g + 1) * Ks], rows[g * Ks:(g + 1) * Ks], n, g * Ks) for g in range(G)]
    m = merge_elites(parts, n)
    o = _ref(S, n)
    np.testing.assert_array_equal(m.idx[0], o)
    np.testing.assert_array_equal(m.S[0], S[o])
    np.testing.assert_array_equal(m.traj[0], rows[o])
    assert m.ee_path is None
    one = merge_elites([p.vehicle(0) for p in parts], n)   # without the vehicle axis
    np.testing.assert_array_equal(one.idx, o)
    np.testing.assert_array_equal(one.traj, rows[o])


def test_merge_elites_tie_across_a_shard_boundary():
    S = np.array([9, 1, 9, 1, 1, 9, 1, 9], np.float32)   # shards [0,4) and [4,8): the 1s at 1, 3 | 4, 6
    rows = np.arange(8, dtype=np.float32).reshape(8, 1, 1)
    parts = [_numpy_elites(S[:4], rows[:4], 3, 0), _numpy_elites(S[4:], rows[4:], 3, 4)]
    m = merge_elites(parts[::-1], 3)   # (the order the parts come in does not matter)
    np.testing.assert_array_equal(m.idx[0], [1, 3, 4])
    np.testing.assert_array_equal(m.traj[0, :, 0, 0], [1, 3, 4])
    with pytest.raises(ValueError):
        merge_elites(parts, 7)


class _StandInEngine:
    """An engine's get_elites over a fixed cost array (the host protocol only)."""
    def __init__(self, S, rows):
        self.S, self.rows, self.K = S, rows, len(S)

    def get_elites(self, n, traj=True):
        e = _numpy_elites(self.S, self.rows, n)
        e.idx = e.idx.astype(np.int32)
        return e


def _sharded_elites_main(rank, world, port, q):
    import torch.distributed as dist
    from quadrotor_manipulator_mppi_amd.distributed import ShardedEngine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rng = np.random.default_rng(99)
        S = rng.uniform(0, 10, 128).astype(np.float32)
        rows = rng.normal(size=(128, 2, 3)).astype(np.float32)
        se = object.__new__(ShardedEngine)   # (no Engine, no HIP stream)
        se.group, se.rank, se.world, se.local, se.mode = None, rank, world, 0, "torch"
        se.engine = _StandInEngine(S[rank * 64:(rank + 1) * 64], rows[rank * 64:(rank + 1) * 64])
        m = se.get_elites(8)
        se.mode = "vehicles"
        own = se.get_elites(8)
        q.put((rank, m.idx, m.S, m.traj, own.idx))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_sharded_get_elites():
    """ShardedEngine.get_elites over stand-in engines: every rank returns the global elites with
    global indices; mode="vehicles" returns the rank's own, without a collective."""
    from test_distributed_cpu import _run2
    rng = np.random.default_rng(99)
    S = rng.uniform(0, 10, 128).astype(np.float32)
    rows = rng.normal(size=(128, 2, 3)).astype(np.float32)
    o = _ref(S, 8)
    for rank, idx, Sm, traj, own in _run2(_sharded_elites_main):
        np.testing.assert_array_equal(idx[0], o)
        np.testing.assert_array_equal(Sm[0], S[o])
        np.testing.assert_array_equal(traj[0], rows[o])
        np.testing.assert_array_equal(own[0], _ref(S[rank * 64:(rank + 1) * 64], 8))
