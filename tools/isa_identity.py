"""Do two builds of the library run the same GPU code?  (tools/, not shipped.)

    python tools/isa_identity.py <lib_a.so> <lib_b.so>

Disassembles every kernel unit's gfx950 code object next to each library
(<stem>.<unit>.co, the objects native dispatch loads; build.py KERNEL_UNITS) with llvm-objdump and
compares the instruction text, and with it -- what native dispatch reads besides the code -- the
kernel descriptors (.rodata), the kernels' metadata (.note: argument layouts, register and LDS
budgets) and the symbol table (names, sizes, addresses; the compilation unit id
__hip_cuid_<hash>, a hash over the source path, left out).  Exit status 0 when every unit is
identical.  Used in round 6 to
show that source edits which only add experiment knobs (off by default) leave the production
kernels bit for bit as the build the round's GPU evidence was taken on.
"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quadrotor_manipulator_mppi_amd.build import KERNEL_UNITS, code_object_path  # noqa: E402

OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "llvm-objdump")


def isa(co: str) -> list:
    out = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
    return [ln for ln in out.splitlines()[3:]]   # (the first lines name the file)


def tables(co: str) -> list:
    out = [ln for sec in (".rodata", ".note") for ln in
           subprocess.run([OBJDUMP, "-s", "-j", sec, co], capture_output=True, text=True, check=True).stdout.splitlines()[3:]]
    syms = subprocess.run([OBJDUMP, "-t", co], capture_output=True, text=True, check=True).stdout.splitlines()[3:]
    return out + sorted(ln for ln in syms if "__hip_cuid_" not in ln)


def main() -> int:
    a, b = sys.argv[1], sys.argv[2]
    same = True
    for unit in KERNEL_UNITS:
        ca, cb = code_object_path(a, unit), code_object_path(b, unit)
        if not os.path.exists(ca) or not os.path.exists(cb):   # a unit one build does not have (e.g. a new one)
            print(f"{unit:28s} only in {'the second' if os.path.exists(cb) else 'the first' if os.path.exists(ca) else 'neither'}"
                  " build: not compared")
            continue
        la, lb = isa(ca), isa(cb)
        nd = sum(1 for x, y in zip(la, lb) if x != y) + abs(len(la) - len(lb))
        ta, tb = tables(ca), tables(cb)
        same &= nd == 0 and ta == tb
        print(f"{unit:28s} {len(lb):7d} lines  {'identical' if nd == 0 else f'{nd} lines differ'}"
              f"; descriptors, metadata, symbols {'identical' if ta == tb else 'DIFFER'}")
    print("identical GPU code" if same else "GPU code differs")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
