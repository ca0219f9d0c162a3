"""The finalize launcher's kernel choice, without a GPU: mppi_launch_finalize describes its launch
into a capture target (mppi_device.h go(), as native dispatch uses it) and
mppi_debug_finalize_kernels returns the symbols a batch's two finalize descriptions would name --
the last step's and the earlier steps'.  Table geometries get a role kernel (k_finalize_s<block
size, role, table index>) and a quiet FINAL; every other shape, READBACK and MPPI_GENERIC_KERNELS
get the kernel of every role (k_finalize<CW, WIN, block size>) twice."""
import ctypes as C

import pytest

from quadrotor_manipulator_mppi_amd import _capi as capi
from quadrotor_manipulator_mppi_amd import build as B

SIG = "EEvPKfS1_PKN4mppi7FinTailEjjiiiiijNS2_9FinParamsE"
FINAL, QUIET, PACK, PEER = 1, 2, 3, 4   # mppi_finalize.hip kRole*


def _kernels(A, H, tsz=8, half=4, window=9, nrec=256, mode=0, peer=0, generic=0):
    L = capi.lib()
    f = L.mppi_debug_finalize_kernels
    f.restype = C.c_int32
    f.argtypes = [C.POINTER(C.c_int32), C.c_char_p, C.c_char_p, C.c_int32]
    g = (C.c_int32 * 10)(A, H, tsz, half, (H + tsz - 1) // tsz, window, nrec, mode, peer, generic)
    full, quiet = C.create_string_buffer(192), C.create_string_buffer(192)
    assert f(g, full, quiet, 192) == 0
    return full.value.decode(), quiet.value.decode()


def _role(nt, role, gid):
    return f"_Z12k_finalize_sILi{nt}ELi{role}ELi{gid}{SIG}"


def _generic(cw, win, nt):
    return f"_Z10k_finalizeILi{cw}ELi{win}ELi{nt}{SIG}"


# (A, H, SavGol window) of the table: arm, drone, quadrotor, whole-body (mppi_finalize.hip FinGeo)
TABLE = {1: (7, 32, 9), 2: (3, 32, 5), 3: (4, 32, 5), 4: (10, 64, 9)}


@pytest.mark.parametrize("gid", sorted(TABLE))
def test_table_shapes_get_their_role_kernels(gid):
    A, H, win = TABLE[gid]
    g = dict(A=A, H=H, half=win // 2, window=win)
    for nrec, nt in ((4, 128), (128, 128), (129, 256), (256, 256), (257, 512), (4096, 512)):
        full, quiet = _kernels(nrec=nrec, **g)
        assert (full, quiet) == (_role(nt, FINAL, gid), _role(nt, QUIET, gid))   # two descriptions per batch
    assert _kernels(mode=1, **g) == (_role(256, PACK, gid),) * 2        # PACK has no quiet form
    assert _kernels(peer=1, **g) == (_role(256, PEER, gid),) * 2        # nor has the peer exchange
    assert _kernels(mode=2, **g) == (_generic(16, win, 256),) * 2       # READBACK: the kernel of every role
    assert _kernels(generic=1, **g) == (_generic(16, win, 256),) * 2    # MPPI_GENERIC_KERNELS


@pytest.mark.parametrize("kw,want", [
    (dict(A=3, H=20, half=2, window=5), (16, 5, 256)),      # drone H = 20: not in the table
    (dict(A=7, H=32, half=2, window=5), (16, 5, 256)),      # the arm with the drone's 5 taps
    (dict(A=3, H=32), (16, 9, 256)),                        # the drone with the arm's 9
    (dict(A=7, H=32, tsz=16), (32, 9, 512)),                # another slice length (MPPI_FIN_TSZ): 24 columns
    (dict(A=7, H=64), (16, 9, 256)),                        # arm at H = 64
    (dict(A=10, H=32), (16, 9, 256)),
    (dict(A=7, H=32, half=3, window=7), (16, 0, 256)),      # run-time taps
])
def test_other_shapes_keep_the_generic_kernel(kw, want):
    assert _kernels(**kw) == (_generic(*want),) * 2


def test_every_named_kernel_is_in_the_code_object():
    with open(B.code_object_path(B.LIB, "mppi_finalize.hip"), "rb") as f:
        blob = f.read()
    for gid, (A, H, win) in TABLE.items():
        for nrec in (4, 256, 4096):
            for kw in (dict(), dict(mode=1), dict(peer=1)):
                for sym in _kernels(A, H, half=win // 2, window=win, nrec=nrec, **kw):
                    assert (sym + ".kd").encode() in blob, sym
