"""Do two builds of the library run the same GPU code?  (tools/, not shipped.)

    python tools/isa_identity.py <lib_a.so> <lib_b.so>
    python tools/isa_identity.py --per-kernel <lib_a.so> <lib_b.so>

Disassembles every kernel unit's gfx950 code object next to each library
(<stem>.<unit>.co, the objects native dispatch loads; build.py KERNEL_UNITS) with llvm-objdump and
compares the instruction text, and with it -- what native dispatch reads besides the code -- the
kernel descriptors (.rodata), the kernels' metadata (.note: argument layouts, register and LDS
budgets) and the symbol table (names, sizes, addresses; the compilation unit id
__hip_cuid_<hash>, a hash over the source path, left out).  Exit status 0 when every unit is
identical.  --per-kernel compares kernel by kernel instead, for a change that ADDS kernels to
existing units (the units then differ as wholes): every kernel the first build has must be in the
second with the same instructions (the text without addresses: branches are relative), the same
64-byte kernel descriptor and the same metadata entry; kernels only the second build has are
listed as new.  Exit status 0 when every kernel of the first build is identical in the second.  Used in round 6 to
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


def functions(co: str) -> dict:
    """symbol -> its instructions, addresses and encodings stripped"""
    out, cur = {}, None
    for ln in isa(co):
        if ln.endswith(">:") and "<" in ln:
            cur = out.setdefault(ln[ln.index("<") + 1:-2], [])
        elif cur is not None and ln.strip():
            cur.append(ln.split("//")[0].strip())
    for body in out.values():   # the padding between functions and at the end of .text
        while body and (body[-1].startswith("s_nop") or body[-1].startswith("s_code_end") or body[-1] == "..."):
            body.pop()
    return out


def descriptors(co: str) -> dict:
    """kernel -> its 64-byte descriptor (<kernel>.kd in .rodata) without the entry offset, as hex"""
    mem = {}
    for ln in subprocess.run([OBJDUMP, "-s", "-j", ".rodata", co], capture_output=True, text=True,
                             check=True).stdout.splitlines()[4:]:
        f = ln[1:].split(" ")
        try:
            addr = int(f[0], 16)
        except ValueError:
            continue
        for i, ch in enumerate("".join(f[1:5])[:32]):
            mem[2 * addr + i] = ch
    out = {}
    for ln in subprocess.run([OBJDUMP, "-t", co], capture_output=True, text=True, check=True).stdout.splitlines():
        f = ln.split()
        if f and f[-1].endswith(".kd"):
            a = int(f[0], 16)
            # (bytes 16..23, the code's offset from the descriptor, move with the unit's layout)
            out[f[-1][:-3]] = "".join(mem.get(2 * a + i, "?") for i in range(128) if not 32 <= i < 48)
    return out


def metadata(co: str) -> dict:
    """kernel -> its amdhsa.kernels entry (argument layout, register and LDS budgets), as text"""
    readobj = os.path.join(os.path.dirname(OBJDUMP), "llvm-readobj")
    text = subprocess.run([readobj, "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for item in text.split("\n  - .agpr_count")[1:]:
        item = item.split("\namdhsa.target")[0]
        name = [ln.split()[-1] for ln in item.splitlines() if ln.strip().startswith(".name:")]
        if name:
            out[name[0]] = item
    return out


def per_kernel(a: str, b: str) -> int:
    same, n_same, n_new = True, 0, 0
    for unit in KERNEL_UNITS:
        ca, cb = code_object_path(a, unit), code_object_path(b, unit)
        if not os.path.exists(ca):
            print(f"{unit}: not in the first build (a new unit): not compared")
            continue
        if not os.path.exists(cb):
            print(f"{unit}: MISSING from the second build")
            same = False
            continue
        fa, fb, da, db, ma, mb = functions(ca), functions(cb), descriptors(ca), descriptors(cb), metadata(ca), metadata(cb)
        bad = [k for k in fa if fa[k] != fb.get(k) or da.get(k) != db.get(k) or ma.get(k) != mb.get(k)]
        new = [k for k in fb if k not in fa]
        n_same += len(fa) - len(bad)
        n_new += len(new)
        same &= not bad
        print(f"{unit:28s} {len(fa):3d} kernels of the first build: {len(fa) - len(bad)} identical "
              f"(instructions, descriptor, metadata), {len(bad)} differ; {len(new)} new")
        for k in bad:
            why = [w for w, x, y in (("instructions", fa[k], fb.get(k)), ("descriptor", da.get(k), db.get(k)),
                                     ("metadata", ma.get(k), mb.get(k))) if x != y]
            print(f"    DIFFERS ({', '.join(why)}): {k}")
        for k in new:
            print(f"    new: {k}")
    print(f"{n_same} kernels identical, {n_new} new; " + ("every kernel of the first build is unchanged"
                                                           if same else "some kernels of the first build changed"))
    return 0 if same else 1


def main() -> int:
    if sys.argv[1] == "--per-kernel":
        return per_kernel(sys.argv[2], sys.argv[3])
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
